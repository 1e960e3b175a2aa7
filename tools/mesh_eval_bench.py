"""Dense-grid decoder query of the Mesher (Mesher.get_grid_uniform
+ Mesher.eval_points, src/utils/Mesher.py:281-347, 427-430) on one MI355X.

  python tools/mesh_eval_bench.py [--resolution R] [--precision P] [--iters K]

Grid: R^3 float32 points over the room0 bound padded by 0.05 (np.linspace per axis, meshgrid,
ravel, as get_grid_uniform), queried through pnr.Renderer.eval_points in 500,000-point chunks
(points_batch_size), as the Mesher does.  Parity: 4,096 random grid points against the oracle's
eval_points (CPU).  Prints one JSON line with the decoder FLOP rate (443,438 FLOP per point).

--extract adds the device geometry between the query and the colouring (pnr.mesher: point masks,
marching cubes, cleaning) at the same resolution, with synthetic keyframes (--keyframes poses yawed
about the scene pose, 680x1200 depth images in 0.3-0.6 scene units) under an 'extract' key.  Each
step is a child process of its own under `timeout` (--step-timeout seconds); after a child that
fails or runs out of time no further child is started and the tool exits non-zero.  The
marching-cubes bytes are the traffic the algorithm needs: the volume read once (4 B/sample), the
per-sample word written and read once (4 + 4 B), 24 B per vertex and 12 B per face written; the rate
is those bytes over the time of the whole call (three launches and the host read of the counts).
The `bound` step builds the mesh bound of the same keyframes (pnr.mesher.get_bound_from_frames) and
writes profiles/mesh_bound.json: the whole hull build, its support launches alone (the build's own
direction sets replayed without the host work between them), rounds / directions / facets, and
`contains` over the grid -- each a wall time ending in a synchronise, the median of five.  The support
pass is VALU work: 8 lane operations (5 arithmetic, one compare, two selects) per point and direction,
reported against 78.6e12 lane operations/s (256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz).
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pointnerf-slam_amd'))
sys.path.insert(0, REPO)

from bench import load_scene, FLOP_PER_POINT_FWD  # noqa: E402


EXTRACT_STEPS = ('masks', 'mc', 'clean', 'bound')
HBM_BYTES_PER_S = 8e12
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
SUPPORT_LANE_OPS = 8    # per point and direction: 5 arithmetic, one compare, two selects


def median_of(fn, n=5):
    """(median seconds, last result) of fn() over `n` calls after one warm-up call; every call ends in
    a device synchronise."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def bound_step(m, keyframes, points, dev):
    """The mesh bound of the keyframes: build, support launches alone, containment over the grid."""
    import pnr
    t_build, fb = median_of(lambda: m.get_bound_from_frames(keyframes, m.scale, device=dev))
    depth = torch.stack([kf['depth'] for kf in keyframes]).float()
    c2w = torch.stack([kf['est_c2w'] for kf in keyframes]).to(dev).float()
    fp = pnr.mesher.FramePoints(depth, c2w, m.fx, m.fy, m.cx, m.cy, extra=c2w[:, :3, 3])
    calls = []

    def recording(dirs):
        calls.append(torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32)).to(dev))
        return fp.support_np(dirs)

    hull = pnr.bound.build_hull(recording, fp.points_np, fb.eps)
    assert np.array_equal(hull.faces, fb.faces)

    def replay():
        for d in calls:
            fp.support(d)

    launches0 = fp.support_launches
    t_support, _ = median_of(replay)
    launches = (fp.support_launches - launches0) // 6
    t_contains, inside = median_of(lambda: fb.contains(points))
    slots = depth.numel() + c2w.shape[0]
    dirs = sum(int(d.shape[0]) for d in calls)
    lane_ops = SUPPORT_LANE_OPS * slots * dirs
    return {'build_ms': round(t_build * 1e3, 3), 'support_ms': round(t_support * 1e3, 3),
            'support_calls': len(calls), 'support_launches': launches, 'rounds': fb.stats['rounds'],
            'directions': dirs, 'facets': fb.stats['facets'], 'hull_vertices': fb.stats['vertices'],
            'capped': bool(fb.capped), 'eps': fb.eps, 'point_slots': slots,
            'support_lane_ops': lane_ops, 'support_lane_ops_per_s': float(f'{lane_ops / t_support:.4g}'),
            'share_of_valu_rate': float(f'{lane_ops / t_support / VALU_LANE_OPS_PER_S:.3g}'),
            'contains_ms': round(t_contains * 1e3, 3), 'contains_points': int(points.shape[0]),
            'contains_inside': int(inside.sum())}


def timed(fn, iters):
    """Mean seconds of fn() over `iters` calls after one warm-up call; every call ends in a device
    synchronise."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters, out


def extract_step(step, args):
    """One --extract step in this process: prints its JSON line."""
    import pnr
    dev = torch.device('cuda:0')
    bound, pose, params = load_scene()
    slam = types.SimpleNamespace(bound=bound, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5)
    r = pnr.Renderer(dict(pnr.ROOM0_CFG), None, slam)
    dec = pnr.get_model(pnr.ROOM0_CFG, nice=False)
    dec.load_state_dict(params)
    dec = dec.to(dev)
    slam.renderer = r
    cfg = dict(pnr.ROOM0_CFG, meshing={'resolution': args.resolution})
    cfg['mapping'] = dict(cfg['mapping'], marching_cubes_bound=(bound.numpy() / cfg['scale']).tolist())
    m = pnr.Mesher(cfg, None, slam)
    g = torch.Generator().manual_seed(0)
    c2w0 = torch.as_tensor(pose, dtype=torch.float32).reshape(4, 4)
    keyframes = []
    for k in range(args.keyframes):
        a = 2 * np.pi * k / args.keyframes
        rot = torch.eye(4)
        rot[0, 0], rot[0, 2], rot[2, 0], rot[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        c2w = c2w0.clone()
        c2w[:3, :3] = rot[:3, :3] @ c2w0[:3, :3]
        keyframes.append({'est_c2w': c2w, 'depth': (0.3 + 0.3 * torch.rand((680, 1200), generator=g)).to(dev)})
    est = torch.stack([kf['est_c2w'] for kf in keyframes])
    grid = m.get_grid_uniform(m.resolution)
    points = grid['grid_points'].to(dev)
    n = points.shape[0]
    out = {'points': n, 'keyframes': args.keyframes}
    if step == 'masks':
        for name, kw in (('poses', dict(get_mask_use_all_frames=True)), ('maxdepth', {}), ('depthtest', {})):
            m.depth_test = name == 'depthtest'
            t, (seen, fore, unseen) = timed(lambda: m.point_masks(points, keyframes, est, len(keyframes) - 1, dev, **kw),
                                            args.iters)
            out[name] = {'ms': round(t * 1e3, 3), 'seen': int(seen.sum()), 'forecast': int(fore.sum()),
                         'unseen': int(unseen.sum())}
    elif step == 'bound':
        out.update(bound_step(m, keyframes, points, dev))
    else:
        z = m.eval_points(points, dec, None, 'fine', dev)[:, -1].contiguous()
        t, (v, f) = timed(lambda: pnr.mesher.marching_cubes(z, grid['xyz'], m.level_set), args.iters)
        out.update({'vertices': v.shape[0], 'faces': f.shape[0]})
        if step == 'mc':
            nbytes = 12 * n + 24 * v.shape[0] + 12 * f.shape[0]
            out.update({'ms': round(t * 1e3, 3), 'bytes': nbytes, 'gbytes_per_s': round(nbytes / t / 1e9, 1),
                        'share_of_8TBps': float(f'{nbytes / t / HBM_BYTES_PER_S:.3g}')})
        else:
            seen = m.point_masks(v, keyframes, est, len(keyframes) - 1, dev)[0]
            thr = m.remove_small_geometry_threshold * m.scale * m.scale
            t, (cv, cf) = timed(lambda: pnr.mesher.clean_mesh(v, f, seen, threshold=thr), args.iters)
            out.update({'ms': round(t * 1e3, 3), 'seen_vertices': int(seen.sum()), 'kept_vertices': cv.shape[0],
                        'kept_faces': cf.shape[0]})
    print(json.dumps({'extract_step': step, **out}))


def run_extract(args):
    """Each step in a child process under its own `timeout`; stops at the first failure."""
    res = {}
    for step in EXTRACT_STEPS:
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               '--extract-step', step, '--resolution', str(args.resolution), '--iters', str(args.iters),
               '--keyframes', str(args.keyframes)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stdout.write(p.stdout)
            raise SystemExit(f'mesh_eval_bench: extract step {step!r} ended with status {p.returncode}; '
                             'no further step started')
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('{"extract_step"')][-1]
        res[step] = {k: v for k, v in json.loads(line).items() if k != 'extract_step'}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--precision', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--extract', action='store_true', help='also time the masks, marching cubes and cleaning')
    ap.add_argument('--extract-step', choices=EXTRACT_STEPS, help='(child of --extract) run one step here')
    ap.add_argument('--keyframes', type=int, default=8)
    ap.add_argument('--step-timeout', type=int, default=180)
    args = ap.parse_args()
    if args.extract_step:
        return extract_step(args.extract_step, args)
    import pnr
    from oracle import ref_render as ref
    dev = torch.device('cuda:0')
    bound, pose, params = load_scene()
    slam = types.SimpleNamespace(bound=bound, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5)
    cfg = dict(pnr.ROOM0_CFG)
    if args.precision:
        cfg['pnr'] = {'precision': args.precision}
    r = pnr.Renderer(cfg, None, slam)
    dec = pnr.get_model(pnr.ROOM0_CFG, nice=False)
    dec.load_state_dict(params)
    dec = dec.to(dev)
    b = bound.numpy()
    pad, R = 0.05, args.resolution
    x, y, z = (np.linspace(b[a][0] - pad, b[a][1] + pad, R) for a in range(3))
    xx, yy, zz = np.meshgrid(x, y, z)
    grid = torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float)
    gd = grid.to(dev)
    bs = 500000

    def query():
        return torch.cat([r.eval_points(pi, dec, None, 'color', dev) for pi in torch.split(gd, bs)], 0)

    out = query()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = query()
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / args.iters
    n = grid.shape[0]
    sel = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:4096]
    rr = ref.eval_points(params, grid[sel], bound)
    og = out[sel.to(dev)].cpu()
    err = float((og - rr).abs().max() / rr.abs().max())
    res = {'metric': 'Mesher dense-grid decoder query points/sec', 'value': round(n / t, 1),
           'unit': 'points/s', 'ms': round(t * 1e3, 3), 'points': n, 'resolution': R,
           'tflops': round(n * FLOP_PER_POINT_FWD / t / 1e12, 1), 'precision': r.precision,
           'parity': {'points': 4096, 'max_abs_err_over_max': float(f'{err:.3g}')}}
    if args.extract:
        del out, gd
        torch.cuda.empty_cache()
        res['extract'] = run_extract(args)
        b = res['extract']['bound']
        print(f"bound: hull build {b['build_ms']} ms (support launches alone {b['support_ms']} ms, {b['rounds']} rounds, "
              f"{b['directions']} directions, {b['facets']} facets), contains over the grid {b['contains_ms']} ms; "
              f"the grid query of this run {res['ms']} ms")
        os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
        with open(os.path.join(REPO, 'profiles', 'mesh_bound.json'), 'w') as fh:
            json.dump({'resolution': R, 'keyframes': args.keyframes, 'frame': [680, 1200], 'timing':
                       'wall time ending in a synchronise, median of five', 'grid_query_ms': res['ms'], **b}, fh, indent=1)
            fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
