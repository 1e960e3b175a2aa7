"""Two-way descriptor matching (pnr.match_two_way, csrc/match.hip) on one MI355X.

  python tools/match_bench.py [--iters K] [--out profiles/match.json]

D = 256 (SuperPoint) with N = M = 1,024 and 4,096: unit Gaussian descriptors, two thirds of desc2 noisy
copies of columns of desc1 (the recipe of tests/test_gpu_match.py), nn_thresh = 0.7.
  call      pnr.match_two_way as the Tracker would call it: three launches and the host read of the count,
            wall time ending in a synchronise
  torch     the same result from torch in the same process: desc1.T @ desc2, clamp, sqrt, two argmins,
            the gather of the scores, the mutual test and the boolean compaction (its own host read)
  launches  the three launches alone (reused buffers, no host read), device time between two events over
            --reps back-to-back calls; 2 N M D FLOP over it against the 157.3 TF fp32-MFMA peak that
            bench.py uses for room0_iter_fp32 (the clear and finalize launches are inside the figure)
call and torch are timed in alternating rounds, one call each per round after a warm-up of both; the
median of --iters rounds is reported and every round is kept.  No target was set for these.
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

FP32_MFMA_PEAK_TF = 157.3
D, THRESH = 256, 0.7


def descriptors(n, dev):
    rng = np.random.RandomState(n)

    def unit(x):
        return (x / np.linalg.norm(x, axis=0, keepdims=True)).astype(np.float32)
    a, b = unit(rng.randn(D, n)), unit(rng.randn(D, n))
    k = 2 * n // 3
    pos, src = rng.choice(n, k, replace=False), rng.randint(0, n, k)
    b[:, pos] = unit(a[:, src] + rng.uniform(0, 0.08, k) * rng.randn(D, k))
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)


def torch_match(d1, d2, thresh):
    dmat = torch.sqrt(2 - 2 * torch.clamp(d1.T @ d2, -1, 1))
    rows = torch.arange(dmat.shape[0], device=d1.device)
    idx = torch.argmin(dmat, dim=1)
    scores = dmat[rows, idx]
    keep = (scores < thresh) & (rows == torch.argmin(dmat, dim=0)[idx])
    return rows[keep], idx[keep], scores[keep]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def run(pnr, dev, n, iters, reps):
    from pnr import _lib
    d1, d2 = descriptors(n, dev)
    ours = lambda: pnr.match_two_way(d1, d2, THRESH)
    base = lambda: torch_match(d1, d2, THRESH)
    for _ in range(3):
        got, ref = ours(), base()
    same = bool(torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]))
    t_call, t_torch = [], []
    for _ in range(iters):
        t_call.append(timed(ours)[0])
        t_torch.append(timed(base)[0])
    b = pnr.matching.MatchBuffers(n, n, dev)
    lib, st = _lib.load(), _lib.stream_of(dev)
    args = (_lib.ptr(d1), _lib.ptr(d2), D, n, n, THRESH, _lib.ptr(b.idx1), _lib.ptr(b.idx2), _lib.ptr(b.score),
            _lib.ptr(b.count), _lib.ptr(b.workspace), b.workspace.numel(), st)
    t_dev = []
    for it in range(iters + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            _lib.check(lib.pnr_match_two_way(*args), 'match_two_way')
        e1.record()
        torch.cuda.synchronize()
        if it:
            t_dev.append(e0.elapsed_time(e1) * 1e3 / reps)
    flop = 2.0 * n * n * D
    call, tor, devt = statistics.median(t_call), statistics.median(t_torch), statistics.median(t_dev)
    return {'N': n, 'M': n, 'D': D, 'matches': int(got[0].numel()), 'same_pairs_as_torch': same,
            'call_us': round(call, 1), 'call_us_runs': [round(x, 1) for x in t_call],
            'torch_us': round(tor, 1), 'torch_us_runs': [round(x, 1) for x in t_torch],
            'torch_over_call': round(tor / call, 2),
            'launches_us': round(devt, 2), 'launches_us_runs': [round(x, 2) for x in t_dev], 'launches_reps': reps,
            'flop': flop, 'launches_tflops': round(flop / devt / 1e6, 2),
            'share_of_fp32_mfma_peak': round(flop / (devt * 1e-6) / (FP32_MFMA_PEAK_TF * 1e12), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pnr
    dev = torch.device('cuda:0')
    out = {'what': 'tools/match_bench.py on 1x MI355X: pnr.match_two_way against the torch form of '
                   f'nn_match_two_way in the same process, alternating rounds, median of {args.iters} (wall time per '
                   'call ending in a device synchronise); launches_us = the three launches alone, device events '
                   f'over {args.reps} back-to-back calls; peak = {FP32_MFMA_PEAK_TF} TF fp32 MFMA; no target was set.',
           'n1024': run(pnr, dev, 1024, args.iters, args.reps),
           'n4096': run(pnr, dev, 4096, args.iters, args.reps),
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
