"""Scoring a reconstruction on the device (src/tools/eval_recon.py: `calc_3d_metric`, `accuracy`, `completion`,
`completion_ratio`, `get_align_transformation`).

The reference aligns with open3d's point-to-point ICP, samples both surfaces with trimesh and measures with two
scipy KD-tree queries.  Here all of it is float64 on the device (csrc/recon.hip, include/pnr.h): an exact
brute-force nearest-neighbour search on the float64 MFMA, trimesh's sampling rule over a counter-based
generator, fixed-order reductions and Kabsch.  Float32 inputs are widened on entry.  Deviations, stated: the
samples follow trimesh's rule but not numpy's random stream; the ICP moves the source by the composed transform
each iteration instead of moving it step by step; `calc_2d_metric`, mesh culling and the trajectory error are
not built.  There is no CPU path.
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
