"""Fusing keyframe depth into the block-sparse TSDF volume (pnr.TSDFVolume, csrc/tsdf.hip) on one MI355X.

  python tools/tsdf_bench.py [--iters K] [--out profiles/tsdf.json] [--mesh-out profiles/tsdf_mesh.json]

Eight synthetic 680x1200 keyframes as tools/mesh_eval_bench.py makes them (the scene pose yawed round the
circle, depth 0.3 + 0.3 rand), fused over the scene bound at the reference's settings (voxel 4 scale / 512,
truncation 0.04 scale, scale 1).  Timed apart, as wall time ending in a device synchronise, median of --iters
runs after one warm-up, each on a volume reset before the run:
  allocate       pnr_tsdf_integrate of the eight frames into a volume whose blocks all exist already is the
                 integrate pass alone; the allocate pass is the call on an empty volume minus that
  integrate_8    one call over the eight frames (an empty volume: allocate + integrate)
  integrate_1x8  eight single-frame calls
  extract        extract_points (count, scan, its host read, emit)
  mesh           extract_triangle_mesh (count, two scans, its host read, emit), to --mesh-out; the count and the
                 emit calls also apart, between device events
Algorithmic bytes of a call: 20 B read + 20 B written per voxel of an allocated block (tsdf, weight, rgb) and
4 B per valid depth pixel.  Reported against the 8 TB/s HBM peak; no target was set: a first measurement.
"""
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
sys.path.insert(0, REPO)

from bench import load_scene  # noqa: E402

HBM_BYTES_PER_S = 8e12
H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5
K = 8


def median_ms(fn, iters, before=None):
    out = []
    for i in range(iters + 1):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--max-blocks', type=int, default=16384)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'tsdf.json'))
    ap.add_argument('--mesh-out', default=os.path.join(REPO, 'profiles', 'tsdf_mesh.json'))
    args = ap.parse_args()
    import pnr
    dev = torch.device('cuda:0')
    bound, pose, _ = load_scene()
    g = torch.Generator().manual_seed(0)
    c2w0 = torch.as_tensor(pose, dtype=torch.float32).reshape(4, 4)
    depth, c2w = [], []
    for k in range(K):
        a = 2 * np.pi * k / K
        rot = torch.eye(4)
        rot[0, 0], rot[0, 2], rot[2, 0], rot[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        m = c2w0.clone()
        m[:3, :3] = rot[:3, :3] @ c2w0[:3, :3]
        c2w.append(m)
        depth.append(0.3 + 0.3 * torch.rand((H, W), generator=g))
    depth, c2w = torch.stack(depth).to(dev), torch.stack(c2w).to(dev)
    color = torch.rand((K, H, W, 3), generator=g).to(dev)
    vol = pnr.TSDFVolume(bound, 4.0 / 512.0, 0.04, H, W, FX, FY, CX, CY, args.max_blocks, device=dev)
    t_first = median_ms(lambda: vol.integrate(depth, color, c2w), args.iters, before=vol.reset)
    n_blocks, dropped = vol.n_blocks, vol.dropped_blocks
    t_again = median_ms(lambda: vol.integrate(depth, color, c2w), args.iters)      # every block exists: no new slot
    t_single = median_ms(lambda: [vol.integrate(depth[k], color[k], c2w[k]) for k in range(K)], args.iters,
                         before=vol.reset)
    vol.reset()
    vol.integrate(depth, color, c2w)
    t_extract = median_ms(vol.extract_points, args.iters)
    n_points = int(vol.extract_points()[0].shape[0])
    valid = int((torch.isfinite(depth) & (depth > 0) & (depth <= 1000.0)).sum())
    call_bytes = n_blocks * 4096 * 40 + valid * 4
    res = {
        'frames': [K, H, W], 'voxel_length': 4.0 / 512.0, 'sdf_trunc': 0.04, 'directory': [int(x) for x in vol.dims],
        'max_blocks': args.max_blocks, 'blocks': n_blocks, 'dropped_blocks': dropped, 'surface_points': n_points,
        'iters': args.iters,
        'ms': {'allocate': max(t_first - t_again, 0.0), 'integrate_8_empty_volume': t_first,
               'integrate_8_existing_blocks': t_again, 'integrate_1x8': t_single, 'extract': t_extract},
        'algorithmic_bytes_per_call': call_bytes,
        'integrate_8_hbm_fraction': call_bytes / (t_again * 1e-3) / HBM_BYTES_PER_S,
        'integrate_1x8_bytes': K * n_blocks * 4096 * 40 + valid * 4,
    }
    mesh = mesh_leg(vol, args.iters)
    mesh.update(frames=[K, H, W], blocks=n_blocks, max_blocks=args.max_blocks, iters=args.iters)
    for path, r in ((args.out, res), (args.mesh_out, mesh)):
        print(json.dumps(r))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(r, f, indent=1)
            f.write('\n')


def mesh_leg(vol, iters):
    """extract_triangle_mesh on the fused volume: the whole call as wall time, and the two C calls between
    device events (count: k_tsdf_mesh<count>, two scans, the totals; emit: k_tsdf_mesh<emit>)."""
    from pnr import _lib
    t_wall = median_ms(vol.extract_triangle_mesh, iters)
    verts, faces, _ = vol.extract_triangle_mesh()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    rgb = torch.empty_like(verts)
    counts = torch.zeros(2, dtype=torch.int64, device=vol.device)
    st, ws = _lib.stream_of(vol.device), vol.mesh_ws
    calls = {
        'count': lambda: vol.lib.pnr_tsdf_mesh_count(vol._ref(), _lib.ptr(ws), ws.numel(), _lib.ptr(counts),
                                                     _lib.ptr(counts[1:]), st),
        'emit': lambda: vol.lib.pnr_tsdf_mesh_emit(vol._ref(), _lib.ptr(ws), ws.numel(), _lib.ptr(verts), _lib.ptr(rgb),
                                                   _lib.ptr(faces), st),
    }
    ms = {'extract_triangle_mesh': t_wall}
    for name, call in calls.items():
        out = []
        for i in range(iters + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _lib.check(call(), 'tsdf_mesh_' + name)
            ev[1].record()
            torch.cuda.synchronize()
            out.append(ev[0].elapsed_time(ev[1]))
        ms[name + '_device'] = statistics.median(out[1:])
    assert counts.tolist() == [V, F]
    # each pass reads tsdf and weight of every live voxel once (the halo's second reads hit the cache and are not
    # counted); the count writes the rank rows, the emit reads two colours and writes xyz, rgb per vertex and a face
    n = vol.n_blocks
    nbytes = {'count': n * 4096 * 8 + n * 256 * 8, 'emit': n * 4096 * 8 + V * (24 + 24) + F * 12}
    return {'vertices': V, 'faces': F, 'ms': ms, 'algorithmic_bytes': nbytes,
            'hbm_fraction': {k: nbytes[k] / (ms[k + '_device'] * 1e-3) / HBM_BYTES_PER_S for k in nbytes}}


if __name__ == '__main__':
    main()
