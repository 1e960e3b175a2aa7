"""The room0 Mapper iteration with and without bundle adjustment (mapping.BA) on one MI355X.

  python tools/ba_bench.py [--iters K] [--warmup W] [--rounds R] [--out profiles/ba_step.json]

bench.py's flagship workload (1,000 rays = 5-frame window x 200 pixels on the room0 camera, the whole
iteration replayed from one HIP graph, pnr.MapGraph(batch_fn=WindowSampler)) twice in one process:
plain, and with `ba=pnr.BundleAdjust(sampler, BA_cam_lr)` -- the map pass also emits the ray
gradients (k_map_ray_grads) and the pose step (k_pose_step) closes the iteration.  The two graphs are
timed in alternating rounds of --iters replays, so clock and thermal drift reach both alike.  Prints
one JSON line: per-round and median ms per iteration of each, and the difference.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pointnerf-slam_amd'))
sys.path.insert(0, REPO)

from bench import ROOM0_CAM, ROOM0_PIXELS, ROOM0_WINDOW, load_scene, make_decoder, room0_window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cam-lr', type=float, default=1e-3)  # mapping.BA_cam_lr (configs/nice_slam.yaml)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pnr
    from pnr.mapping import MapGraph, MapStep, WindowSampler
    dev = torch.device('cuda:0')
    bound, _, params = load_scene()
    cfg = pnr.ROOM0_CFG
    per = ROOM0_PIXELS // ROOM0_WINDOW
    graphs = {}
    for name in ('plain', 'ba'):
        slam, frames = room0_window(pnr, params, bound, dev)
        sampler = WindowSampler(frames, per, ROOM0_CAM['fx'], ROOM0_CAM['fy'], ROOM0_CAM['cx'], ROOM0_CAM['cy'],
                                n_samples=cfg['rendering']['N_samples'], seed=0)
        ba = pnr.BundleAdjust(sampler, args.cam_lr) if name == 'ba' else None
        mstep = MapStep(pnr.Renderer(cfg, None, slam), make_decoder(pnr, cfg, params, dev),
                        lr=cfg['mapping']['imap_decoders_lr'], w_color_loss=cfg['mapping']['w_color_loss'], ba=ba)
        graphs[name] = (MapGraph(mstep, batch_fn=sampler), mstep)
        for _ in range(args.warmup):
            graphs[name][0]()
    torch.cuda.synchronize()
    ms = {'plain': [], 'ba': []}
    for _ in range(args.rounds):
        for name in ('plain', 'ba'):
            g = graphs[name][0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                g()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.iters * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {'workload': 'room0 Mapper iteration, 1,000 rays over a 5-frame window, one replayed HIP graph; '
                       'ba: camera tensors of frames 1..4 stepped by Adam (frame 0 fixed)',
           'rays_per_iter': per * ROOM0_WINDOW, 'iters_per_round': args.iters, 'rounds': args.rounds,
           'decoder_precision': graphs['plain'][1].renderer.precision,
           'tail_fused': {k: bool(v[1].tail_fused) for k, v in graphs.items()},
           'ms_per_iter_rounds': {k: [round(x, 4) for x in v] for k, v in ms.items()},
           'ms_per_iter_median': {k: round(v, 4) for k, v in med.items()},
           'ba_cost_ms': round(med['ba'] - med['plain'], 4), 'ba_cost_rel': round(med['ba'] / med['plain'] - 1, 4),
           'device': torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
