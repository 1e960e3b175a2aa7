"""SuperPoint on the device (pnr.SuperPointFrontend, csrc/conv.hip + csrc/keypoints.hip) on one MI355X.

  python tools/superpoint_bench.py [--iters K] [--reps R] [--out profiles/superpoint.json]

480 x 640 and 680 x 1200 grey images, random weights (uniform +-1/sqrt(fan-in)).  Random weights give a nearly flat
heatmap, so conf_thresh is set once per size to the heatmap's 99.5th percentile: about 0.5 % of the pixels are
candidates, as with trained weights; both sides use it.
  run       SuperPointFrontend.run as the Tracker would call it: 12 convolution launches, the keypoint launches,
            the host read of the count, torch's sort of the keys, the descriptor sample; wall time ending in a
            synchronise
  torch     the same network in torch float32 on the device (conv2d, relu, max_pool2d, norm), then the reference's
            post-processing where the reference runs it: the logits copied to the host, softmax / depth-to-space /
            threshold / greedy NMS / border cut in numpy, grid_sample on the device, normalisation in numpy
  layers    the 12 convolution launches alone: device events around every launch, --reps forwards, per layer and
            summed; the algorithmic FLOP (2 K Cout H W per layer) over the sum against the 157.3 TF fp32-MFMA peak
            that bench.py uses for room0_iter_fp32
  torch_net the torch network alone, device events around the whole forward
run and torch are timed in alternating rounds, one call each per round after a warm-up of both; the median of
--iters rounds is reported and every round is kept.  No target was set for these.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pointnerf-slam_amd'))
sys.path.insert(0, REPO)

FP32_MFMA_PEAK_TF = 157.3
SPEC = dict(conv1a=(1, 64, 3), conv1b=(64, 64, 3), conv2a=(64, 64, 3), conv2b=(64, 64, 3), conv3a=(64, 128, 3),
            conv3b=(128, 128, 3), conv4a=(128, 128, 3), conv4b=(128, 128, 3), convPa=(128, 256, 3),
            convPb=(256, 65, 1), convDa=(128, 256, 3), convDb=(256, 256, 1))


def random_state_dict(seed=0):
    gen, sd = torch.Generator().manual_seed(seed), {}
    for name, (cin, cout, k) in SPEC.items():
        s = 1.0 / np.sqrt(k * k * cin)
        sd[name + '.weight'] = (torch.rand((cout, cin, k, k), generator=gen) * 2 - 1) * s
        sd[name + '.bias'] = (torch.rand(cout, generator=gen) * 2 - 1) * s
    return sd


def torch_net(sd, img):
    def conv(x, name):
        return F.conv2d(x, sd[name + '.weight'], sd[name + '.bias'], padding=sd[name + '.weight'].shape[2] // 2)
    x = img[None, None]
    for blk in '123':
        x = F.max_pool2d(F.relu(conv(F.relu(conv(x, f'conv{blk}a')), f'conv{blk}b')), 2)
    x = F.relu(conv(F.relu(conv(x, 'conv4a')), 'conv4b'))
    semi = conv(F.relu(conv(x, 'convPa')), 'convPb')
    desc = conv(F.relu(conv(x, 'convDa')), 'convDb')
    return semi, desc / torch.norm(desc, p=2, dim=1, keepdim=True)


def host_post(semi, coarse, H, W, thresh, nms_dist, border=4):
    """the reference's post-processing (demo_superpoint.py:246-293), restated: numpy on the host but grid_sample"""
    semi = semi.cpu().numpy()[0]
    dense = np.exp(semi)
    dense = dense / (dense.sum(0) + .00001)
    Hc, Wc = H // 8, W // 8
    heat = dense[:-1].transpose(1, 2, 0).reshape(Hc, Wc, 8, 8).transpose(0, 2, 1, 3).reshape(H, W)
    ys, xs = np.nonzero(heat >= thresh)
    alive = np.zeros((H + 2 * nms_dist, W + 2 * nms_dist), bool)
    alive[ys + nms_dist, xs + nms_dist] = True
    kept = []
    for k in np.argsort(-heat[ys, xs], kind='stable'):
        y, x = ys[k], xs[k]
        if alive[y + nms_dist, x + nms_dist]:
            alive[y:y + 2 * nms_dist + 1, x:x + 2 * nms_dist + 1] = False
            kept.append((x, y, heat[y, x]))
    pts = np.array(kept, np.float32).reshape(-1, 3).T
    pts = pts[:, (pts[0] >= border) & (pts[0] < W - border) & (pts[1] >= border) & (pts[1] < H - border)]
    grid = torch.from_numpy(np.stack([pts[0] / (W / 2.) - 1., pts[1] / (H / 2.) - 1.], 1)).float().view(1, 1, -1, 2)
    desc = F.grid_sample(coarse, grid.to(coarse.device), align_corners=False).cpu().numpy().reshape(256, -1)
    return pts, desc / np.linalg.norm(desc, axis=0)[None], heat


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(pnr, dev, H, W, iters, reps):
    sd = random_state_dict()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    img = torch.rand((H, W), generator=torch.Generator().manual_seed(H)).to(dev)
    fe = pnr.SuperPointFrontend(sd, nms_dist=4, conf_thresh=0.015)
    fe.net.forward(img)
    fe.conf_thresh = float(torch.quantile(fe.net.heat.flatten()[::7], 0.995))
    ours = lambda: fe.run(img)
    base = lambda: host_post(*torch_net(sd_dev, img), H, W, fe.conf_thresh, fe.nms_dist)
    for _ in range(2):
        got, ref = ours(), base()
    t_run, t_torch = [], []
    for _ in range(iters):
        t_run.append(timed(ours)[0])
        t_torch.append(timed(base)[0])
    # the convolution launches alone, per layer
    names = [n for n, _, _ in pnr.superpoint.LAYERS]
    per = {n: [] for n in names}
    for it in range(iters + 1):
        ev = {n: [] for n in names}

        def hook(name, before):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev[name].append(e)
        for _ in range(reps):
            fe.net.forward(img, on_layer=hook)
        torch.cuda.synchronize()
        if it:
            for n in names:
                per[n].append(sum(a.elapsed_time(b) for a, b in zip(ev[n][0::2], ev[n][1::2])) * 1e3 / reps)
    t_net = []
    for it in range(iters + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            torch_net(sd_dev, img)
        e1.record()
        torch.cuda.synchronize()
        if it:
            t_net.append(e0.elapsed_time(e1) * 1e3 / reps)
    shapes, flop, layers = {'img': (H, W)}, {}, {}
    for name, src, epi in pnr.superpoint.LAYERS:
        h, w = shapes[src]
        cin, cout, k = SPEC[name]
        flop[name] = 2.0 * k * k * cin * cout * h * w
        shapes[name] = (h // 2, w // 2) if epi == pnr.superpoint.RELU_POOL2 else (h, w)
        us = statistics.median(per[name])
        layers[name] = {'us': round(us, 1), 'gflop': round(flop[name] / 1e9, 3), 'tflops': round(flop[name] / us / 1e6, 2)}
    conv_us = sum(statistics.median(per[n]) for n in names)
    total = sum(flop.values())
    same = got[0].shape == ref[0].shape and bool(np.array_equal(got[0][:2].cpu().numpy(), ref[0][:2]))
    return {'H': H, 'W': W, 'conf_thresh': fe.conf_thresh, 'keypoints': int(got[0].shape[1]),
            'torch_keypoints': int(ref[0].shape[1]), 'same_keypoint_positions_as_torch': same,
            'run_ms': round(statistics.median(t_run), 3), 'run_ms_runs': [round(x, 3) for x in t_run],
            'torch_ms': round(statistics.median(t_torch), 3), 'torch_ms_runs': [round(x, 3) for x in t_torch],
            'torch_over_run': round(statistics.median(t_torch) / statistics.median(t_run), 2),
            'layers': layers, 'conv_us': round(conv_us, 1), 'conv_gflop': round(total / 1e9, 2),
            'conv_tflops': round(total / conv_us / 1e6, 2),
            'conv_share_of_fp32_mfma_peak': round(total / (conv_us * 1e-6) / (FP32_MFMA_PEAK_TF * 1e12), 4),
            'torch_net_us': round(statistics.median(t_net), 1), 'torch_net_us_runs': [round(x, 1) for x in t_net],
            'reps': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pnr
    dev = torch.device('cuda:0')
    out = {'what': 'tools/superpoint_bench.py on 1x MI355X: pnr.SuperPointFrontend.run against the torch float32 network '
                   'plus the reference\'s host post-processing in the same process, alternating rounds, median of '
                   f'{args.iters} (wall ms per call ending in a device synchronise); layers = device events around each '
                   f'convolution launch over {args.reps} forwards; peak = {FP32_MFMA_PEAK_TF} TF fp32 MFMA; random weights, '
                   'conf_thresh = the 99.5th percentile of the heatmap; no target was set.',
           's480x640': run(pnr, dev, 480, 640, args.iters, args.reps),
           's680x1200': run(pnr, dev, 680, 1200, args.iters, args.reps),
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
