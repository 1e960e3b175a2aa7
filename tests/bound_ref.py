"""Numpy restatement of the mesh bound's device passes (test infrastructure only): include/pnr.h
`pnr_bound_support` / `pnr_bound_points` / `pnr_bound_contains_*` state the rules, this module is their
specification.

Point set P.  Keyframe k, pixel (v, u) of the `stride` lattice with depth d finite, 0 < d <= depth_trunc:
index k H W + v W + u, position the map growth's candidate with rho = 0 (points_grow_ref.candidates: the
float32 ray of get_rays, p = rays_o + rays_d d, unfused).  Then the extra points at K H W + e.  Every
other index of [0, K H W + n_extra) is invalid: a NaN row.

Support.  h = max over the valid points of (x nx + y ny) + z nz in unfused float32 (a NaN never wins),
arg = the smallest index attaining it; h = -inf, arg = -1 without one.

Containment.  all_f ((x a + y b) + z c <= d) in unfused float64, float32 points widened first.
"""
import numpy as np

from points_grow_ref import candidates

F32 = np.float32


def positions(depth, c2w, fx, fy, cx, cy, stride=1, depth_trunc=1000.0, extra=None):
    """(xyz float32 (K H W + n_extra, 3) with NaN rows for the invalid indices, valid bool)."""
    depth = np.asarray(depth, F32)
    K, H, W = depth.shape
    rows, ok = [], []
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    lattice = ((vv % stride == 0) & (uu % stride == 0)).reshape(-1)
    for k in range(K):
        p, d = candidates(depth[k], np.asarray(c2w[k], F32), fx, fy, cx, cy)
        with np.errstate(invalid='ignore'):
            good = np.isfinite(d) & (d > 0) & (d <= F32(depth_trunc)) & lattice
        rows.append(np.where(good[:, None], p, F32(np.nan)).astype(F32))
        ok.append(good)
    if extra is not None and len(extra):
        e = np.asarray(extra, F32).reshape(-1, 3)
        good = ~np.isnan(e).any(1)
        rows.append(np.where(good[:, None], e, F32(np.nan)).astype(F32))
        ok.append(good)
    if not rows:
        return np.zeros((0, 3), F32), np.zeros(0, bool)
    return np.concatenate(rows), np.concatenate(ok)


def support(xyz, valid, dirs, chunk=64):
    """(h float32 (D,), arg int64 (D,)) of float32 rows `xyz` (the invalid ones excluded)."""
    xyz = np.asarray(xyz, F32)
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    h = np.full(dirs.shape[0], -np.inf, F32)
    arg = np.full(dirs.shape[0], -1, np.int64)
    if xyz.shape[0] == 0:
        return h, arg
    x, y, z = xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3]
    for s in range(0, dirs.shape[0], chunk):
        n = dirs[s:s + chunk]
        with np.errstate(invalid='ignore', over='ignore'):
            v = (x * n[None, :, 0] + y * n[None, :, 1]) + z * n[None, :, 2]
        assert v.dtype == F32
        v = np.where(np.asarray(valid, bool)[:, None] & ~np.isnan(v), v, F32(-np.inf))
        hh = v.max(0)
        first = np.argmax(v == hh[None, :], axis=0)
        h[s:s + chunk] = hh
        arg[s:s + chunk] = np.where(hh > -np.inf, first, -1)
    return h, arg


def contains(points, planes):
    """bool (P,): every plane satisfied, unfused float64."""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    inside = np.ones(p.shape[0], bool)
    for a, b, c, d in planes:
        with np.errstate(invalid='ignore'):
            inside &= (p[:, 0] * a + p[:, 1] * b) + p[:, 2] * c <= d
    return inside


def oracle(xyz, valid=None):
    """(support, points_of) closures over an explicit point set, the arguments of pnr.bound.build_hull."""
    xyz = np.asarray(xyz, F32)
    valid = np.ones(xyz.shape[0], bool) if valid is None else np.asarray(valid, bool)
    return (lambda dirs: support(xyz, valid, dirs)), (lambda idx: xyz[np.asarray(idx, np.int64)])
