"""Growing the neural-point map from one keyframe (pnr.NeuralPoints.add_frame) on one MI355X.

  python tools/points_grow_bench.py [--iters K] [--out profiles/points_grow.json]

A 680x1200 frame at stride 1 with three depth offsets (2,448,000 candidates) is added into a
200k-point cloud (float32 features, radius 0.01: the C3 size) and into a 1M-point cloud (float16
features, radius 0.008: the C5 size).  The scene is the room0 bound seen from its centre; the depth is
the room's wall (the ray's box exit, 3% short of it); the existing cloud lies on the walls all round the
room except in the right half of the view, so about half of the candidates are rejected as near and
the rest thinned and added.
Timed apart, as wall time ending in a device synchronise, median of --iters runs after one warm-up:
  insert   add_frame: the insertion pass (five launches and the scan) and its one host read
  rebuild  the index rebuild (pnr_points_build) for the grown cloud
Bytes model of the insertion pass: per candidate 4 B depth + 16 B position + 1 B flag written, then
the position and flag read back by the thinning and emit passes (4 B keep / rank words each way);
per valid candidate 8 x 16 B bucket headers; 16 B per point of the probed cells of a free candidate
(it scans them all) and 16 B for a rejected one (a lower bound: its scan stops at the first point
inside the ball); per survivor 140 B (12 B xyz + 128 B features).  Reported against the 8 TB/s HBM
peak, as the mesh extraction rows are (the headers and points are re-read by neighbouring candidates
and mostly come from the caches); no target was set.
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

HBM_BYTES_PER_S = 8e12
H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5
RHO = (-0.02, 0.0, 0.02)


def wall_depth(bound, c2w, dev):
    """z-depth (H,W) float32 of the room's wall along every pixel's ray, 3% short of the box exit."""
    v, u = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    dirs = torch.stack([(u - CX) / FX, -(v - CY) / FY, -torch.ones_like(u, dtype=torch.float32)], -1)
    rd = (dirs[..., None, :] * c2w[:3, :3]).sum(-1).double()
    ro = c2w[:3, 3].double()
    t = torch.maximum((bound[:, 0] - ro) / rd, (bound[:, 1] - ro) / rd).amin(-1)
    return (0.97 * t).float().contiguous(), ro, rd


def wall_cloud(n, bound, c2w, dev, seed):
    """n points on the room's walls (3% inside, 2% of depth scatter, 1 mm of noise) in every direction
    from the camera but the right half of its view."""
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.randn((2 * n, 3), device=dev, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    ro = c2w[:3, 3].double()
    t = torch.maximum((bound[:, 0] - ro) / d, (bound[:, 1] - ro) / d).amin(-1)
    t = 0.97 * t * (1.0 + 0.02 * (2 * torch.rand(2 * n, device=dev, generator=g, dtype=torch.float64) - 1))
    cam = (d * t[:, None]) @ c2w[:3, :3].double()          # R^T (p - ro)
    u = FX * cam[:, 0] / -cam[:, 2] + CX
    v = -FY * cam[:, 1] / -cam[:, 2] + CY
    right = (cam[:, 2] < 0) & (u >= W / 2) & (u < W + 8) & (v > -8) & (v < H + 8)
    p = (ro + d * t[:, None])[~right][:n]
    assert p.shape[0] == n
    return (p.float() + 0.001 * torch.randn((n, 3), device=dev, generator=g)).contiguous()


def probed_points(pts, cand):
    """Per candidate, the points in its 2x2x2 probe cells (the hash's own float32 cell arithmetic)."""
    o = torch.tensor(pts.origin, device=cand.device)
    inv = torch.tensor(1.0, device=cand.device) / torch.tensor(pts.cell, device=cand.device)

    def key(c):
        return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    off = 1 << 20
    cells, counts = torch.unique(key(torch.floor((pts.xyz[:pts.n_points] - o) * inv).long() + off), return_counts=True)
    t = (cand - o) * inv
    f = torch.floor(t)
    base = f.long() - (t - f < 0.5).long() + off
    total = torch.zeros(cand.shape[0], dtype=torch.int64, device=cand.device)
    for n in range(8):
        k = key(base + torch.tensor([n & 1, (n >> 1) & 1, n >> 2], device=cand.device))
        at = torch.searchsorted(cells, k).clamp(max=cells.numel() - 1)
        total += torch.where(cells[at] == k, counts[at], torch.zeros_like(at))
    return total


def run(pnr, dev, n_points, radius, feat_dtype, iters):
    bound = torch.from_numpy(np.load(os.path.join(REPO, 'tests', 'golden', 'scene.npz'))['bound']).to(dev)
    yaw = 0.6
    c2w = torch.eye(4, device=dev)
    c2w[:3, :3] = torch.tensor([[np.cos(yaw), 0., np.sin(yaw)], [0., 1., 0.], [-np.sin(yaw), 0., np.cos(yaw)]])
    c2w[:3, 3] = bound.float().mean(1)
    depth, ro, rd = wall_depth(bound.double(), c2w, dev)
    xyz = wall_cloud(n_points, bound.double(), c2w, dev, seed=n_points)
    n_cand = H * W * len(RHO)
    pts = pnr.NeuralPoints(xyz, 0.1 * torch.randn((n_points, 32), device=dev), mode='idw', radius=radius, k=8,
                           capacity=n_points + n_cand, bound=bound.cpu(), feat_dtype=feat_dtype).to(dev)
    t_ins, t_idx, last = [], [], None
    for it in range(iters + 1):
        pts._n = n_points          # back to the cloud before the frame
        pts.index()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts.add_frame(depth, c2w, H, W, FX, FY, CX, CY, bound.cpu(), rho=RHO, return_candidates=(it == 0))
        t1 = time.perf_counter()   # (add_frame ends in its host read of the counters)
        if it == 0:
            cand, flags = pts.last_candidates
            pts.last_candidates = None
        pts.index()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert last is None or last == pts.last_add
        last = dict(pts.last_add)
        if it:
            t_ins.append((t1 - t0) * 1e3)
            t_idx.append((t2 - t1) * 1e3)
    pts._n = n_points
    per_cand = probed_points(pts, cand)
    free, near = (flags & 2) != 0, (flags & 3) == 1
    probed = int(per_cand[free].sum()) + int(near.sum())
    nbytes = n_cand * (4 + 16 + 1 + (16 + 1) + 3 * 4 + (4 + 4)) + last['valid'] * 128 + probed * 16 + last['added'] * 140
    ms = statistics.median(t_ins)
    return {'points': n_points, 'feat_dtype': feat_dtype, 'radius_add': radius, 'thin': radius, 'cell': pts.cell,
            'table_bits': pts.table_bits, 'counters': last,
            'insert_ms': round(ms, 3), 'insert_ms_runs': [round(x, 3) for x in t_ins],
            'rebuild_ms': round(statistics.median(t_idx), 3), 'rebuild_ms_runs': [round(x, 3) for x in t_idx],
            'rebuild_points': n_points + last['added'],
            'points_read_model': probed, 'probed_cell_points_mean': round(float(per_cand.float().mean()), 2), 'bytes': int(nbytes), 'gbytes_per_s': round(nbytes / ms / 1e6, 1),
            'share_of_8TBps': round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pnr
    dev = torch.device('cuda:0')
    out = {'what': 'tools/points_grow_bench.py on 1x MI355X: one 680x1200 frame at stride 1 with rho = (-0.02, 0, '
                   '0.02) (2,448,000 candidates) added into a 200k-point (C3) and a 1M-point float16 (C5) cloud. '
                   f'Wall time (host clock, each ending in a device synchronise), median of {args.iters} after one '
                   'warm-up; no target was set for these.',
           'candidates': H * W * len(RHO),
           'bytes_model': 'per candidate 4 B depth + 16 B position + 1 B flag written, 17 B read back by the thinning '
                          'pass, 12 B of slot / keep words, 8 B of scan words; per valid candidate 8 x 16 B headers + '
                          '16 B per point of a free candidate\'s probed cells and 16 B for a rejected one (lower bound: '
                          'its scan stops at the first hit); 140 B per survivor; rate = those bytes over the whole call, share of the 8 TB/s HBM peak',
           'C3_200k': run(pnr, dev, 200_000, 0.01, 'float32', args.iters),
           'C5_1M_f16': run(pnr, dev, 1_000_000, 0.008, 'float16', args.iters),
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
