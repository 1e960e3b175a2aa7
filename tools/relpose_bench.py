"""Time pnr.estimate_pose on one GPU: L = 256 and 1,024 matches, 1,024 samples, median of five rounds.
Per call ending in a synchronise, and the three launches alone (events around a batch of raw C calls).
Writes profiles/relpose.json."""
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

S, ROUNDS, CALLS = 1024, 5, 50


def matches(L, dev):
    rng = np.random.RandomState(0)
    X = np.c_[rng.uniform(-1.5, 1.5, (L, 2)), rng.uniform(2, 5, L)]
    X2 = X + np.array([0.2, 0.1, -0.2])
    x1, x2 = X[:, :2] / X[:, 2:] + 5e-5 * rng.randn(L, 2), X2[:, :2] / X2[:, 2:] + 5e-5 * rng.randn(L, 2)
    x2[: L * 3 // 10] = rng.uniform(-0.5, 0.5, (L * 3 // 10, 2))
    return torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)


def main():
    dev = torch.device('cuda:0')
    out = {'samples': S, 'rounds': ROUNDS, 'calls_per_round': CALLS, 'cases': []}
    lib = _lib.load()
    for L in (256, 1024):
        cur, ref = matches(L, dev)
        b = pnr.relpose.PoseBuffers(L, S, dev)
        call = lambda: pnr.estimate_pose(ref, cur, samples=S, buffers=b)  # noqa: E731
        raw = lambda: lib.pnr_relpose_estimate(  # noqa: E731
            _lib.ptr(cur), _lib.ptr(ref), L, S, 0, 0.0003, _lib.ptr(b.pose), _lib.ptr(b.mask), _lib.ptr(b.count),
            _lib.ptr(b.workspace), b.workspace.numel(), _lib.stream_of(dev))
        inliers = int(call().num_inliers)
        wall, launches = [], []
        for _ in range(ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
                torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / CALLS * 1e6)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                raw()
            e1.record()
            torch.cuda.synchronize()
            launches.append(e0.elapsed_time(e1) / CALLS * 1e3)
        out['cases'].append({'L': L, 'inliers': inliers, 'call_us': statistics.median(wall),
                             'launches_us': statistics.median(launches)})
    with open(os.path.join(REPO, 'profiles', 'relpose.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
