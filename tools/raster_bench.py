#!/usr/bin/env python3
"""First measurements of the mesh depth rasteriser (pnr.recon.render_depth) on one MI355X -> profiles/raster.json.

Renders 64 views at 500 x 500, focal 300 (calc_2d_metric's camera, one of its view batches) of two meshes: the
~2M-face height field tools/recon_bench.py samples, seen from above (sub-pixel triangles: the small path), and
a box of six triangles per wall seen from inside (screen-filling triangles: the large path, the ground-truth
case).  Each figure is the median of five calls after a warm-up call, wall time (host clock) ending in a device
synchronise; a call includes its one host read of the pair count.  The shares of count, fill and tile come from
device events around the three library calls of one further pass (the scan and the allocations lie between them
and are the remainder).  (face, view) setups per second count F x views once, over the whole call: the count and
fill passes each run that many setups and the tile pass one per (tile, face) pair.
No target is set; the numbers are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pointnerf-slam_amd'))
import pnr  # noqa: E402
from pnr import _lib  # noqa: E402

ROUNDS = 5
H = W = 500
K = (300.0, 300.0, 249.5, 249.5)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def height_field(side, dev):
    """tools/recon_bench.py's mesh: a side x side height field over the unit square, two triangles per cell"""
    ii, jj = torch.meshgrid(torch.arange(side), torch.arange(side), indexing='ij')
    verts = torch.stack([ii / side, jj / side, 0.05 * torch.sin(ii / 40.0) * torch.cos(jj / 55.0)], -1)
    v00 = (ii[:-1, :-1] * side + jj[:-1, :-1]).reshape(-1)
    faces = torch.cat([torch.stack([v00, v00 + 1, v00 + side], 1), torch.stack([v00 + 1, v00 + side + 1, v00 + side], 1)])
    return verts.reshape(-1, 3).double().to(dev), faces.to(dev)


def box(dev, lo=(-3.0, -2.0, -1.2), hi=(3.0, 2.0, 1.2)):
    """a room of six triangles per wall: every wall is three strips of two triangles"""
    verts, faces = [], []
    for axis in range(3):
        a, b = [c for c in range(3) if c != axis]
        for side in (lo, hi):
            for s in range(3):
                q = np.zeros((4, 3))
                q[:, axis] = side[axis]
                q[:, a] = [lo[a] + (hi[a] - lo[a]) * (s + d) / 3 for d in (0, 1, 1, 0)]
                q[:, b] = [lo[b], lo[b], hi[b], hi[b]]
                n = len(verts) * 4
                verts.append(q)
                faces += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
    return torch.from_numpy(np.concatenate(verts)).to(dev), torch.tensor(faces, device=dev)


def views(origin, target, dev):
    c2w = pnr.recon._viewmatrix(target - origin, np.array([0.0, 0.0, -1.0]), origin)
    return torch.from_numpy(c2w).to(dev)


def phases(v, f, c2w):
    """device-event ms of count, fill and tile of one pass, and its (tile, face) pair count"""
    lib, dev = _lib.load(), v.device
    r = _lib.Raster(verts=_lib.ptr(v), V=v.shape[0], faces=_lib.ptr(f), F=f.shape[0], c2w=_lib.ptr(c2w),
                    n_views=c2w.shape[0], H=H, W=W, fx=K[0], fy=K[1], cx=K[2], cy=K[3], z_near=0.01, z_far=20.0)
    st = _lib.stream_of(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    counts = torch.empty(lib.pnr_raster_counters(r), dtype=torch.int32, device=dev)
    out = torch.empty((c2w.shape[0], H, W), dtype=torch.float32, device=dev)
    ev[0].record()
    _lib.check(lib.pnr_raster_count(r, _lib.ptr(counts), st), 'raster_count')
    ev[1].record()
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    pairs = int(ends[-1])
    nbytes = lib.pnr_raster_workspace_bytes(r, pairs)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ev[2].record()
    _lib.check(lib.pnr_raster_fill(r, _lib.ptr(counts), _lib.ptr(ends), pairs, _lib.ptr(ws), nbytes, st), 'raster_fill')
    ev[3].record()
    _lib.check(lib.pnr_raster_tiles(r, _lib.ptr(counts), _lib.ptr(ends), pairs, _lib.ptr(out), _lib.ptr(ws), nbytes, st),
               'raster_tiles')
    ev[4].record()
    torch.cuda.synchronize()
    return {'count_ms': ev[0].elapsed_time(ev[1]), 'fill_ms': ev[2].elapsed_time(ev[3]),
            'tile_ms': ev[3].elapsed_time(ev[4])}, pairs


def measure(name, v, f, c2w):
    render = lambda: pnr.recon.render_depth(v, f, c2w, H, W, *K)  # noqa: E731
    img = render()  # warm-up
    times = [wall_ms(render) for _ in range(ROUNDS)]
    ms, n = statistics.median(times), c2w.shape[0]
    phases(v, f, c2w)
    ph, pairs = phases(v, f, c2w)
    res = {'faces': f.shape[0], 'views': n, 'ms': round(ms, 3), 'ms_per_view': round(ms / n, 4),
           'face_view_setups_per_s': f.shape[0] * n / (ms * 1e-3), 'pairs_per_view': pairs / n,
           'all_ms': [round(t, 3) for t in times], 'covered_share': float((img > 0).float().mean()),
           **{k: round(x, 3) for k, x in ph.items()},
           **{k.replace('_ms', '_share_of_call'): round(x / ms, 3) for k, x in ph.items()}}
    print(name, res, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'raster.json'))
    ap.add_argument('--scale', type=float, default=1.0, help='shrinks the height field (a rehearsal, not a measurement)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('raster_bench: needs the GPU; there is no CPU path')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    n = 64
    res = {'what': __doc__.split('\n\n')[1].replace('\n', ' '), 'scale': args.scale, 'H': H, 'W': W, 'focal': K[0]}
    v, f = height_field(max(2, int(1001 * args.scale ** 0.5)), dev)
    above = np.concatenate([rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.3, 0.6, (n, 1))], 1)
    on_field = np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), np.zeros((n, 1))], 1)
    res['height_field'] = measure('height_field', v, f, views(above, on_field, dev))
    v, f = box(dev)
    inside = rng.uniform([-2, -1.3, -0.8], [2, 1.3, 0.8], (n, 3))
    res['box'] = measure('box', v, f, views(inside, np.round(rng.uniform(-10000, 10000, (n, 3)), 2), dev))
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
