#!/usr/bin/env python3
"""First measurements of pnr.recon on one MI355X -> profiles/recon.json.

Times `nearest` at 200k x 200k and 20k x 1M, `sample_surface` at 200k samples of a ~2M-face mesh, and one ICP
iteration (`pnr_icp_step`) at the vertex count of tools/mesh_eval_bench.py --extract (1,220,202).  Each figure is
the median of five calls after a warm-up call, wall time (host clock) ending in a device synchronise.  Pair
rates count Q R pairs; the share of peak charges 8 flops a pair (its 4 multiply-adds of a 16x16x4 MFMA) against
the part's published float64 matrix peak, 78.6 TFLOP/s -- a whole-call rate, not a kernel's.
Baseline: torch.cdist(q, r).min(1) in float64 at 32768 x 32768 (the 8 GiB distance matrix is the largest
power-of-two square that fits beside the rest), in the same process, alternating rounds with `nearest`.
No target is set; the numbers are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pointnerf-slam_amd'))
import pnr  # noqa: E402
from pnr import _lib  # noqa: E402

F64_MATRIX_PEAK = 78.6e12
ROUNDS = 5


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn):
    fn()  # warm-up
    times = [wall_ms(fn) for _ in range(ROUNDS)]
    return statistics.median(times), times


def pair_figures(ms, pairs):
    rate = pairs / (ms * 1e-3)
    return {'ms': round(ms, 3), 'pairs': pairs, 'pairs_per_s': rate,
            'share_of_f64_mfma_peak': round(rate * 8 / F64_MATRIX_PEAK, 4)}


def cloud(n, seed, dev):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.rand((n, 3), generator=g, dtype=torch.float64) * 2 - 1).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'recon.json'))
    ap.add_argument('--scale', type=float, default=1.0, help='shrinks every size (a rehearsal, not a measurement)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('recon_bench: needs the GPU; there is no CPU path')
    dev = torch.device('cuda:0')
    n = lambda v: max(1, int(v * args.scale))  # noqa: E731
    res = {'what': __doc__.split('\n\n')[1].replace('\n', ' '), 'scale': args.scale, 'nearest': {}}

    for name, (Q, R) in {'200k_x_200k': (n(200000), n(200000)), '20k_x_1M': (n(20000), n(1000000))}.items():
        q, r = cloud(Q, 1, dev), cloud(R, 2, dev)
        ms, times = median_ms(lambda: pnr.recon.nearest(q, r))
        res['nearest'][name] = {**pair_figures(ms, Q * R), 'Q': Q, 'R': R, 'all_ms': [round(t, 3) for t in times]}
        print(name, res['nearest'][name], flush=True)

    B = n(32768)
    q, r = cloud(B, 3, dev), cloud(B, 4, dev)
    ours, base = [], []
    pnr.recon.nearest(q, r)
    torch.cdist(q, r).min(1)
    for _ in range(ROUNDS):  # alternating rounds
        ours.append(wall_ms(lambda: pnr.recon.nearest(q, r)))
        base.append(wall_ms(lambda: torch.cdist(q, r).min(1)))
    d, i = pnr.recon.nearest(q, r)
    bd, bi = torch.cdist(q, r).min(1)
    res['baseline'] = {'Q': B, 'R': B, 'nearest': pair_figures(statistics.median(ours), B * B),
                       'torch_cdist_min': pair_figures(statistics.median(base), B * B),
                       'index_agreement': float((i == bi).double().mean()),
                       'max_abs_dist_difference': float((d - bd).abs().max())}
    print('baseline', res['baseline'], flush=True)
    del bd, bi

    # a mesh of ~2M faces: a 1000 x 1000 height field, two triangles per cell
    side = max(2, int(1001 * args.scale ** 0.5))
    ii, jj = torch.meshgrid(torch.arange(side), torch.arange(side), indexing='ij')
    verts = torch.stack([ii / side, jj / side, 0.05 * torch.sin(ii / 40.0) * torch.cos(jj / 55.0)], -1)
    verts = verts.reshape(-1, 3).double().to(dev)
    v00 = (ii[:-1, :-1] * side + jj[:-1, :-1]).reshape(-1)
    faces = torch.cat([torch.stack([v00, v00 + 1, v00 + side], 1),
                       torch.stack([v00 + 1, v00 + side + 1, v00 + side], 1)]).to(dev)
    S = n(200000)
    ms, times = median_ms(lambda: pnr.recon.sample_surface(verts, faces, S, seed=1))
    res['sample_surface'] = {'faces': faces.shape[0], 'samples': S, 'ms': round(ms, 3),
                             'samples_per_s': S / (ms * 1e-3), 'all_ms': [round(t, 3) for t in times]}
    print('sample_surface', res['sample_surface'], flush=True)

    N = n(1220202)
    src, dst = cloud(N, 5, dev), cloud(N, 6, dev)
    lib = _lib.load()
    nbytes = lib.pnr_icp_workspace_bytes(N, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    T_in = torch.eye(4, dtype=torch.float64, device=dev)
    T_out, stats = torch.empty_like(T_in), torch.empty(3, dtype=torch.float64, device=dev)

    def icp_step():
        _lib.check(lib.pnr_icp_step(_lib.ptr(src), N, _lib.ptr(dst), N, _lib.ptr(T_in), 0.1, _lib.ptr(T_out),
                                    _lib.ptr(stats), _lib.ptr(ws), nbytes, _lib.stream_of(dev)), 'icp_step')
    ms, times = median_ms(icp_step)
    res['icp_iteration'] = {**pair_figures(ms, N * N), 'N': N, 'M': N, 'fitness': float(stats[0]),
                            'all_ms': [round(t, 3) for t in times]}
    print('icp_iteration', res['icp_iteration'], flush=True)

    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
