"""Scoring a reconstruction on the device (src/tools/eval_recon.py: `calc_3d_metric`, `accuracy`, `completion`,
`completion_ratio`, `get_align_transformation`, `calc_2d_metric`, `check_proj`; src/tools/cull_mesh.py).

The reference aligns with open3d's point-to-point ICP, samples both surfaces with trimesh and measures with two
scipy KD-tree queries.  Here all of it is float64 on the device (csrc/recon.hip, include/pnr.h): an exact
brute-force nearest-neighbour search on the float64 MFMA, trimesh's sampling rule over a counter-based
generator, fixed-order reductions and Kabsch.  Float32 inputs are widened on entry.  Deviations, stated: the
samples follow trimesh's rule but not numpy's random stream; the ICP moves the source by the composed transform
each iteration instead of moving it step by step; the trajectory error is not built.

`calc_2d_metric` renders both meshes with the tiled depth rasteriser of csrc/raster.hip where the reference drives
open3d's OpenGL window: homogeneous edge functions in float64, the least depth per pixel (include/pnr.h "mesh depth
rasteriser" states the rule and its deviations: z_near a parameter, background 0, no anti-aliasing, no top-left
rule).  The view draw takes axis-aligned bounds where trimesh takes oriented ones, and numpy's random stream
where the reference mixes trimesh's and `random`.  There is no CPU path.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib


def _cloud(name, t):
    _lib.require_cuda(t)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'pnr.recon.{name}: point sets are (n,3) float32 or float64 tensors')
    return t.double().contiguous()


def nearest(query, ref, max_dist=None, slices=None):
    """For every query point the nearest ref point by exact brute force: (dist (Q,) float64, idx (Q,) int64) on
    the device, no host synchronisation.  `pnr_nn_search` in include/pnr.h states the contract: dist is the
    float64 distance to ref[idx]; idx is the argmin up to the rounding bound given there; bitwise reproducible.
    With max_dist, queries whose nearest point is farther get idx -1 and dist inf.  `slices` forces the number
    of ref slices the search is split into (the result does not depend on it)."""
    q, r = _cloud('nearest', query), _cloud('nearest', ref)
    if q.device != r.device:
        raise ValueError('pnr.recon.nearest: the point sets are on different devices')
    Q, R, dev = q.shape[0], r.shape[0], q.device
    limit = math.inf if max_dist is None else float(max_dist)
    if not limit >= 0.0:
        raise ValueError("'max_dist' should be non-negative")
    if Q == 0 or R == 0:
        return (torch.full((Q,), math.inf, dtype=torch.float64, device=dev),
                torch.full((Q,), -1, dtype=torch.int64, device=dev))
    lib = _lib.load()
    nbytes = lib.pnr_nn_workspace_bytes(Q, R)
    if nbytes == 0:
        raise ValueError(f'pnr.recon.nearest: sizes Q = {Q}, R = {R} are out of range')
    dist = torch.empty(Q, dtype=torch.float64, device=dev)
    idx = torch.empty(Q, dtype=torch.int64, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pnr_nn_search(_lib.ptr(q), Q, _lib.ptr(r), R, limit, int(slices or 0), _lib.ptr(dist), _lib.ptr(idx),
                                 _lib.ptr(ws), nbytes, _lib.stream_of(dev)), 'nn_search')
    return dist, idx


def _mesh(name, verts, faces):
    v = _cloud(name, verts)
    _lib.require_cuda(faces)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64) or \
            faces.device != v.device:
        raise ValueError(f'pnr.recon.{name}: faces are an (F,3) int32 or int64 tensor on the vertices\' device')
    return v, faces.long().contiguous()


def sample_surface(verts, faces, count, seed=0, uniforms=None):
    """`trimesh.sample.sample_surface(mesh, count)`: (points (count,3) float64, face_idx (count,) int64), faces
    drawn in proportion to their area, points uniform inside them.  The uniforms are an explicit (count,3)
    float64 tensor or, by default, the device's counter-based generator keyed by `seed` and the sample number
    (include/pnr.h `pnr_sample_surface` states the rule; trimesh's own random stream is not reproduced).
    Zero-area faces are never chosen."""
    v, f = _mesh('sample_surface', verts, faces)
    V, F, dev = v.shape[0], f.shape[0], v.device
    if F < 1 or count < 0:
        raise ValueError('pnr.recon.sample_surface: the mesh needs a face and count is non-negative')
    if uniforms is not None:
        _lib.require_cuda(uniforms)
        if uniforms.shape != (count, 3) or uniforms.dtype != torch.float64 or uniforms.device != dev:
            raise ValueError('pnr.recon.sample_surface: uniforms are a (count,3) float64 tensor on the mesh\'s device')
        uniforms = uniforms.contiguous()
    lib = _lib.load()
    area = torch.empty(F, dtype=torch.float64, device=dev)
    _lib.check(lib.pnr_face_areas(_lib.ptr(v), V, _lib.ptr(f), F, _lib.ptr(area), _lib.stream_of(dev)), 'face_areas')
    cum = torch.cumsum(area, 0)
    points = torch.empty((count, 3), dtype=torch.float64, device=dev)
    face_idx = torch.empty(count, dtype=torch.int64, device=dev)
    _lib.check(lib.pnr_sample_surface(_lib.ptr(v), _lib.ptr(f), _lib.ptr(cum), F, count, int(seed) & (2 ** 64 - 1),
                                      _lib.ptr(uniforms), _lib.ptr(points), _lib.ptr(face_idx), _lib.stream_of(dev)),
               'sample_surface')
    return points, face_idx


def _dist_stats(dist, dist_th):
    """(sum of dist, number below dist_th) as a (2,) float64 device tensor, summed in a fixed order."""
    lib = _lib.load()
    nbytes = lib.pnr_dist_stats_workspace_bytes()
    out = torch.empty(2, dtype=torch.float64, device=dist.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dist.device)
    _lib.check(lib.pnr_dist_stats(_lib.ptr(dist), dist.shape[0], float(dist_th), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                  _lib.stream_of(dist.device)), 'dist_stats')
    return out


def _score(query, ref, dist_th=0.0):
    """(mean nearest distance from query to ref, share of them below dist_th) as Python floats"""
    dist, _ = nearest(query, ref)
    total, below = _dist_stats(dist, dist_th).tolist()
    return total / dist.shape[0], below / dist.shape[0]


def accuracy(gt_points, rec_points):
    """Mean distance from every reconstructed point to its nearest ground-truth point (a Python float)."""
    return _score(rec_points, gt_points)[0]


def completion(gt_points, rec_points):
    """Mean distance from every ground-truth point to its nearest reconstructed point (a Python float)."""
    return _score(gt_points, rec_points)[0]


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """Share of the ground-truth points with a reconstructed point closer than dist_th (a Python float)."""
    return _score(gt_points, rec_points, dist_th)[1]


def transform_points(points, T):
    """R p + t of (n,3) points for a (4,4) transform, float64 on the device."""
    p = _cloud('transform_points', points)
    T = torch.as_tensor(T, dtype=torch.float64).to(p.device).contiguous()
    if T.shape != (4, 4):
        raise ValueError('pnr.recon.transform_points: T is (4,4)')
    out = torch.empty_like(p)
    _lib.check(_lib.load().pnr_transform_points(_lib.ptr(p), p.shape[0], _lib.ptr(T), _lib.ptr(out),
                                                _lib.stream_of(p.device)), 'transform_points')
    return out


def icp(src, dst, threshold=0.1, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """Point-to-point ICP as open3d's `registration_icp(src, dst, threshold, init)` defines it, with its default
    convergence criteria: (T (4,4) float64 on the device, fitness, inlier_rmse).  Each iteration is one
    `pnr_icp_step`: the source under the current transform, its nearest dst points within `threshold`, their
    fixed-order sums, Kabsch with the reflection fix, the composed transform.  The loop runs on the host and reads
    fitness and RMSE once per iteration for the stop test: fine for an offline tool, not for a captured graph."""
    s, d = _cloud('icp', src), _cloud('icp', dst)
    N, M, dev = s.shape[0], d.shape[0], s.device
    lib = _lib.load()
    nbytes = lib.pnr_icp_workspace_bytes(N, M)
    if nbytes == 0 or d.device != dev:
        raise ValueError(f'pnr.recon.icp: sizes N = {N}, M = {M} are out of range, or the devices differ')
    T = torch.eye(4, dtype=torch.float64) if init is None else torch.as_tensor(init, dtype=torch.float64)
    T = T.to(dev).contiguous().clone()
    if T.shape != (4, 4):
        raise ValueError('pnr.recon.icp: init is (4,4)')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def step(T_in):
        T_out = torch.empty_like(T_in)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        _lib.check(lib.pnr_icp_step(_lib.ptr(s), N, _lib.ptr(d), M, _lib.ptr(T_in), float(threshold), _lib.ptr(T_out),
                                    _lib.ptr(stats), _lib.ptr(ws), nbytes, _lib.stream_of(dev)), 'icp_step')
        fitness, rmse, _ = stats.tolist()
        return T_out, fitness, rmse

    T_next, fitness, rmse = step(T)
    for _ in range(max_iteration):
        T, before = T_next, (fitness, rmse)
        T_next, fitness, rmse = step(T)
        if abs(before[0] - fitness) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
            break
    return T, fitness, rmse


def read_ply(path, device='cuda'):
    """The binary little-endian PLY that `pnr.mesher.write_ply` writes (float x y z, optional uchar colours,
    faces as `list uchar int` triangles): (verts (V,3) float64, faces (F,3) int64) on `device`."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if end < 0 or not data.startswith(b'ply\nformat binary_little_endian 1.0\n'):
        raise ValueError(f'pnr.recon.read_ply: {path} is not a binary little-endian PLY')
    lines = data[:end].decode('ascii').split('\n')
    nv = nf = None
    props = []
    for line in lines:
        w = line.split()
        if w[:2] == ['element', 'vertex']:
            nv = int(w[2])
        elif w[:2] == ['element', 'face']:
            nf = int(w[2])
        elif w[:1] == ['property'] and nf is None:
            props.append((w[2], {'float': '<f4', 'uchar': 'u1'}.get(w[1])))
        elif w[:1] == ['property'] and w[1:] != ['list', 'uchar', 'int', 'vertex_indices']:
            raise ValueError(f'pnr.recon.read_ply: face property {line!r} is not the one write_ply writes')
    if nv is None or nf is None or [p[0] for p in props[:3]] != ['x', 'y', 'z'] or any(p[1] is None for p in props):
        raise ValueError(f'pnr.recon.read_ply: {path} does not have the layout write_ply writes')
    off = end + len(b'end_header\n')
    vert = np.frombuffer(data, dtype=np.dtype(props), count=nv, offset=off)
    face = np.frombuffer(data, dtype=[('n', 'u1'), ('idx', '<i4', (3,))], count=nf, offset=off + vert.nbytes)
    if nf and not (face['n'] == 3).all():
        raise ValueError(f'pnr.recon.read_ply: {path} has faces that are not triangles')
    v = np.stack([vert['x'], vert['y'], vert['z']], axis=1).astype(np.float64)
    return torch.from_numpy(v).to(device), torch.from_numpy(face['idx'].astype(np.int64)).to(device)


def calc_3d_metric(rec, gt, align=True, n_points=200000, seed=0):
    """`calc_3d_metric(rec_meshfile, gt_meshfile, align)`: rec and gt are (verts, faces) device tensors or paths
    of PLY files as `pnr.mesher.write_ply` writes them.  With align, the reconstruction is first moved by the
    ICP of its vertices onto the ground truth's (threshold 0.1, identity start).  Both surfaces are sampled at
    n_points points (seeds `seed` and `seed + 1`) and scored.  Returns {'accuracy_cm', 'completion_cm',
    'completion_ratio_pct', 'transformation'}: three Python floats and the (4,4) device transform."""
    rv, rf = read_ply(rec) if isinstance(rec, str) else rec
    gv, gf = read_ply(gt) if isinstance(gt, str) else gt
    rv, rf = _mesh('calc_3d_metric', rv, rf)
    gv, gf = _mesh('calc_3d_metric', gv, gf)
    T = torch.eye(4, dtype=torch.float64, device=rv.device)
    if align:
        T, _, _ = icp(rv, gv, threshold=0.1)
        rv = transform_points(rv, T)
    rec_pc, _ = sample_surface(rv, rf, n_points, seed=seed)
    gt_pc, _ = sample_surface(gv, gf, n_points, seed=seed + 1)
    comp, ratio = _score(gt_pc, rec_pc, 0.05)  # completion and its ratio share one search
    return {'accuracy_cm': accuracy(gt_pc, rec_pc) * 100.0, 'completion_cm': comp * 100.0,
            'completion_ratio_pct': ratio * 100.0, 'transformation': T}


def _poses(name, c2w, dev):
    c = torch.as_tensor(c2w, dtype=torch.float64).to(dev).contiguous()
    if c.dim() != 3 or c.shape[1:] != (4, 4):
        raise ValueError(f'pnr.recon.{name}: c2w is (n,4,4)')
    return c


def render_depth(verts, faces, c2w, H, W, fx, fy, cx, cy, z_near=0.01, z_far=20.0, view_batch=None):
    """Depth images (n, H, W) float32 of a triangle mesh from n OpenCV camera-to-world poses, on the device, by
    the rule of include/pnr.h "mesh depth rasteriser": least depth in [z_near, z_far] per pixel centre, two-sided,
    watertight, 0 where nothing is hit; bitwise reproducible and independent of `view_batch` (views rendered per
    pass; by default as many as keep the tile counters and lists inside the library's bounds, at most 64).  Each
    batch is count -> scan -> fill -> tiles and reads its (tile, face) pair count on the host once."""
    v, f = _mesh('render_depth', verts, faces)
    dev = v.device
    c = _poses('render_depth', c2w, dev)
    n, H, W = c.shape[0], int(H), int(W)
    out = torch.zeros((n, H, W), dtype=torch.float32, device=dev)
    if n == 0 or f.shape[0] == 0:
        return out
    lib = _lib.load()
    r = _lib.Raster(verts=_lib.ptr(v), V=v.shape[0], faces=_lib.ptr(f), F=f.shape[0], H=H, W=W, fx=fx, fy=fy, cx=cx,
                    cy=cy, z_near=z_near, z_far=z_far)
    batch = min(n, 64) if view_batch is None else int(view_batch)
    if batch < 1:
        raise ValueError('pnr.recon.render_depth: view_batch is positive')
    st = _lib.stream_of(dev)
    i = 0
    while i < n:
        b = min(batch, n - i)
        r.c2w, r.n_views = _lib.ptr(c[i:]), b
        nc = lib.pnr_raster_counters(r)
        pairs, nbytes = 0, 0
        if nc:
            counts = torch.empty(nc, dtype=torch.int32, device=dev)
            _lib.check(lib.pnr_raster_count(r, _lib.ptr(counts), st), 'raster_count')
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            pairs = int(ends[-1])
            nbytes = lib.pnr_raster_workspace_bytes(r, pairs)
        if nbytes == 0:  # counters or lists past the library's bounds: fewer views per pass
            if view_batch is not None or b == 1:
                raise ValueError(f'pnr.recon.render_depth: {b} view(s) of {H} x {W} with {f.shape[0]} faces are out '
                                 'of range')
            batch = (b + 1) // 2
            continue
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.pnr_raster_fill(r, _lib.ptr(counts), _lib.ptr(ends), pairs, _lib.ptr(ws), nbytes, st),
                   'raster_fill')
        _lib.check(lib.pnr_raster_tiles(r, _lib.ptr(counts), _lib.ptr(ends), pairs, _lib.ptr(out[i:]), _lib.ptr(ws),
                                        nbytes, st), 'raster_tiles')
        i += b
    return out


def depth_l1(a, b):
    """Per image the mean |a - b| of two (n, H, W) float32 device stacks: (n,) float64, differences and sums in
    float64 in a fixed order (bitwise reproducible)."""
    _lib.require_cuda(a, b)
    if a.dim() != 3 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32 or \
            a.device != b.device:
        raise ValueError('pnr.recon.depth_l1: a and b are (n,H,W) float32 tensors of one shape on one device')
    a, b = a.contiguous(), b.contiguous()
    n, hw, dev = a.shape[0], a.shape[1] * a.shape[2], a.device
    out = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    lib = _lib.load()
    nbytes = lib.pnr_depth_l1_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pnr_depth_l1(_lib.ptr(a), _lib.ptr(b), n, hw, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                _lib.stream_of(dev)), 'depth_l1')
    return out


def _seen(name, points, c2w, H, W, fx, fy, cx, cy, per_view):
    p = _cloud(name, points)
    c = _poses(name, c2w, p.device)
    flags = torch.zeros(c.shape[0] if per_view else p.shape[0], dtype=torch.uint8, device=p.device)
    if flags.shape[0]:
        _lib.check(_lib.load().pnr_frustum_seen(_lib.ptr(p), p.shape[0], _lib.ptr(c), c.shape[0], int(H), int(W), fx, fy,
                                                cx, cy, _lib.ptr(flags) if per_view else None,
                                                None if per_view else _lib.ptr(flags), _lib.stream_of(p.device)),
                   'frustum_seen')
    return flags.bool()


def views_seeing(points, c2w, H, W, fx, fy, cx, cy):
    """(n,) bool: does view i see any of the points, by `check_proj`'s test (include/pnr.h `pnr_frustum_seen`)."""
    return _seen('views_seeing', points, c2w, H, W, fx, fy, cx, cy, True)


def points_seen(points, c2w, H, W, fx, fy, cx, cy):
    """(P,) bool: does any view see point i, by the same test."""
    return _seen('points_seen', points, c2w, H, W, fx, fy, cx, cy, False)


def cull_mesh(verts, faces, c2w, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5):
    """src/tools/cull_mesh.py: drop the faces whose three vertices are all seen by none of the (OpenCV) poses.
    Returns (verts, faces) with the vertices as they came."""
    v, f = _mesh('cull_mesh', verts, faces)
    seen = points_seen(v, c2w, H, W, fx, fy, cx, cy)
    return verts, faces[seen[f].any(1)]


def _viewmatrix(z, up, pos):
    """eval_recon.py `viewmatrix` on (n,3) rows: (n,4,4) camera-to-world poses"""
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    v2 = unit(z)
    v0 = unit(np.cross(up, v2))
    v1 = unit(np.cross(v2, v0))
    c2w = np.tile(np.eye(4), (len(z), 1, 1))
    c2w[:, :3, :] = np.stack([v0, v1, v2, pos], 2)
    return c2w


def sample_views(gt_verts, n, seed=0, pc_unseen=None, H=500, W=500, focal=300.):
    """calc_2d_metric's view draw: (n,4,4) float64 poses on the device.  The origin is uniform in the ground
    truth's axis-aligned bounds about their centre, the smallest extent shrunk to 0.3 and the other two to 0.7
    (trimesh's oriented bounds are not built), shifted by +0.4 along z; the target is uniform in +-10,000 rounded
    to 2 decimals, up is (0, 0, -1).  Candidates come from `RandomState(seed)` on the host in blocks; those that
    see any `pc_unseen` point (`views_seeing`, one call per block) are redrawn."""
    gv = _cloud('sample_views', gt_verts)
    lo, hi = gv.min(0).values.cpu().numpy(), gv.max(0).values.cpu().numpy()
    ext = hi - lo
    shrink = np.full(3, 0.7)
    shrink[np.argmin(ext)] = 0.3
    centre = 0.5 * (lo + hi) + np.array([0.0, 0.0, 0.4])
    rng = np.random.RandomState(seed)
    views = np.zeros((0, 4, 4))
    cxy = (W / 2.0 - 0.5, H / 2.0 - 0.5)
    for _ in range(1000):
        if len(views) >= n:
            break
        m = max(2 * (n - len(views)), 16)
        origin = centre + (rng.uniform(size=(m, 3)) - 0.5) * ext * shrink
        target = np.round(rng.uniform(-10000, 10000, size=(m, 3)), 2)
        cand = _viewmatrix(target - origin, np.array([0.0, 0.0, -1.0]), origin)
        if pc_unseen is not None and len(pc_unseen):
            sees = views_seeing(pc_unseen, torch.from_numpy(cand).to(gv.device), H, W, focal, focal, *cxy)
            cand = cand[~sees.cpu().numpy()]
        views = np.concatenate([views, cand])
    if len(views) < n:
        raise RuntimeError('pnr.recon.sample_views: no view avoids the unseen points')
    return torch.from_numpy(views[:n]).to(gv.device)


def calc_2d_metric(rec, gt, align=True, n_imgs=1000, pc_unseen=None, seed=0, views=None):
    """`calc_2d_metric(rec_meshfile, gt_meshfile, align, n_imgs)`, the "Depth L1" column: rec and gt as for
    `calc_3d_metric`; `pc_unseen` (P,3) are the points no sampled view may see (the reference's
    `*_pc_unseen.npy`), `views` (n,4,4) OpenCV poses to use instead of `sample_views(gt, n_imgs, seed, pc_unseen)`.
    Both meshes are rendered at 500 x 500, focal 300, 64 views at a time (the images of a batch are dropped after
    their L1).  Returns {'depth_l1_cm': mean over the views in cm, 'per_view': (n,) float64 in metres, 'views',
    'transformation'}."""
    H = W = 500
    focal, cx, cy = 300.0, 249.5, 249.5
    rv, rf = read_ply(rec) if isinstance(rec, str) else rec
    gv, gf = read_ply(gt) if isinstance(gt, str) else gt
    rv, rf = _mesh('calc_2d_metric', rv, rf)
    gv, gf = _mesh('calc_2d_metric', gv, gf)
    dev = rv.device
    T = torch.eye(4, dtype=torch.float64, device=dev)
    if align:
        T, _, _ = icp(rv, gv, threshold=0.1)
        rv = transform_points(rv, T)
    if pc_unseen is not None:
        pc_unseen = torch.as_tensor(pc_unseen).to(dev)
    views = sample_views(gv, n_imgs, seed, pc_unseen, H, W, focal) if views is None else _poses('calc_2d_metric', views, dev)
    per_view = []
    for i in range(0, views.shape[0], 64):
        c = views[i:i + 64]
        per_view.append(depth_l1(render_depth(gv, gf, c, H, W, focal, focal, cx, cy),
                                 render_depth(rv, rf, c, H, W, focal, focal, cx, cy)))
    per_view = torch.cat(per_view) if per_view else torch.zeros(0, dtype=torch.float64, device=dev)
    return {'depth_l1_cm': float(per_view.mean()) * 100.0 if len(per_view) else 0.0, 'per_view': per_view,
            'views': views, 'transformation': T}
