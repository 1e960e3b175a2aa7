"""Numpy restatement of growing the neural-point map from a keyframe's depth (test infrastructure
only).  The stage is build-defined (the reference has no neural points; Point-SLAM calls the step
add_neural_points): include/pnr.h `pnr_points_add_frame` states the rules and this module is their
specification.

Candidates.  Pixel rank r of the list `pixels` (flat v W + u) or of the `stride` lattice (row-major),
offset o: candidate c = r len(rho) + o at depth z = depth[v,u] (1 + rho[o]) and position
p = rays_o + rays_d z, all float32 and unfused, with the renderer's ray (get_rays: dirs =
[(u-cx)/fx, -(v-cy)/fy, -1], rays_d = ((d0 R0 + d1 R1) + d2 R2) per row, rays_o = c2w[:3,3]).

Decisions (`decide`), each a function of the float32 candidate positions alone:
  valid     depth[v,u] finite and > 0, and bound[a,0] < p_a < bound[a,1] (float32) on every axis
            (a pixel index outside the image: invalid, p = 0)
  free      valid, and no existing point x_i (rows [0, n)) with (dx dx + dy dy) + dz dz <= radius_add^2
            (float32, unfused: the gather's arithmetic, oracle/ref_points.py)
  kept      free, and (thin > 0) the smallest candidate index of its voxel; the voxel coordinate per
            axis is int(clamp(floor((p_a - origin_a) * (1 / thin)), +-1e9)) in float32 (the hash's
            cell_coord), its identity the three coordinates' low 21 bits
  appended  the kept candidates in candidate order at rows [n, n + n_new), the first capacity - n of
            them; the rest are counted as dropped
Counters: candidates, valid, free, survivors (= kept), dropped.

`decide` takes the candidate positions as an argument, so a test can feed it the device's own float32
positions (teacher forcing) and then compare every decision exactly.  `brute_force64` is the same
rule set in float64 without the voxel-identity mask, and `margins64` the relative distance of every
candidate from each decision threshold, for inputs that stay clear of float32 rounding.
"""
import numpy as np

VALID, FREE, KEPT = 1, 2, 4
F32 = np.float32


def candidate_pixels(H, W, pixels=None, stride=1):
    """(u, v, inside the image) per pixel rank."""
    if pixels is None:
        v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
        u, v = u.reshape(-1), v.reshape(-1)
        return u.astype(np.int64), v.astype(np.int64), np.ones(u.shape, bool)
    pix = np.asarray(pixels, np.int64).reshape(-1)
    ok = (pix >= 0) & (pix < H * W)
    p = np.where(ok, pix, 0)
    return p % W, p // W, ok


def candidates(depth, c2w, fx, fy, cx, cy, pixels=None, stride=1, rho=(0.0,), dtype=np.float32):
    """Candidate positions (C,3) and their pixels' depth (C,) (NaN for a pixel outside the image, whose
    position is 0), in `dtype` arithmetic (float32: the spec; float64: the yardstick)."""
    T = dtype
    H, W = depth.shape
    u, v, ok = candidate_pixels(H, W, pixels, stride)
    R = len(rho)
    c2w = np.asarray(c2w, np.float32).astype(T)
    d = depth.astype(np.float32)[v, u].astype(T)
    dx = (u.astype(T) - T(cx)) / T(fx)
    dy = -((v.astype(T) - T(cy)) / T(fy))
    rd = np.stack([(dx * c2w[r, 0] + dy * c2w[r, 1]) + T(-1.0) * c2w[r, 2] for r in range(3)], -1)
    ro = c2w[:3, 3]
    rho_t = np.asarray(rho, np.float32).astype(T)
    with np.errstate(invalid='ignore', over='ignore'):
        z = d[:, None] * (T(1.0) + rho_t[None, :])                      # (P, R)
        p = ro[None, None, :] + rd[:, None, :] * z[:, :, None]          # (P, R, 3)
    p = np.where(ok[:, None, None], p, T(0.0)).reshape(-1, 3)
    dd = np.repeat(np.where(ok, d, T(np.nan)), R)
    return p.astype(T), dd


def voxel_key(p, origin, thin):
    """The hash's cell identity of float32 positions: 3 x 21-bit two's complement coordinates."""
    inv = F32(1.0) / F32(thin)
    with np.errstate(invalid='ignore', over='ignore'):
        f = np.floor((p.astype(F32) - np.asarray(origin, F32)[None, :]) * inv)
        f = np.fmin(np.fmax(f, F32(-1.0e9)), F32(1.0e9))  # fmin / fmax: a NaN takes the bound, as on the device
    c = f.astype(np.int64) & 0x1FFFFF
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def _first_of_each(keys, mask):
    """mask restricted to the smallest index of each key."""
    idx = np.nonzero(mask)[0]
    out = np.zeros(mask.shape, bool)
    if idx.size:
        _, first = np.unique(keys[idx], return_index=True)
        out[idx[first]] = True
    return out


def decide(cand_xyz, cand_depth, xyz, n, bound, radius_add, thin, origin, chunk=512):
    """Flag bytes (C,) of float32 candidate positions against the existing rows xyz[:n]."""
    p = np.asarray(cand_xyz, F32)
    d = np.asarray(cand_depth, F32)
    b = np.asarray(bound, np.float64).reshape(3, 2).astype(F32)
    with np.errstate(invalid='ignore'):
        valid = np.isfinite(d) & (d > 0)
        for a in range(3):
            valid &= (p[:, a] > b[a, 0]) & (p[:, a] < b[a, 1])
    free = valid.copy()
    x = np.asarray(xyz, F32)[:n]
    r2 = F32(radius_add) * F32(radius_add)
    if n > 0:
        for s in range(0, p.shape[0], chunk):
            q = p[s:s + chunk]
            with np.errstate(invalid='ignore', over='ignore'):
                dl = q[:, None, :] - x[None, :, :]
                d2 = (dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2]
                free[s:s + chunk] &= ~(d2 <= r2).any(1)
    kept = _first_of_each(voxel_key(p, origin, thin), free) if thin > 0 else free.copy()
    return (valid * VALID + free * FREE + kept * KEPT).astype(np.uint8)


def append(flags, cand_xyz, xyz, feats, n, init_feats=None):
    """(xyz, feats, counters) after appending the kept candidates; xyz / feats (capacity, .) copies."""
    xyz, feats = np.array(xyz, F32, copy=True), np.array(feats, F32, copy=True)
    kept = np.nonzero(flags & KEPT)[0]
    room = xyz.shape[0] - n
    take = kept[:room]
    xyz[n:n + take.size] = np.asarray(cand_xyz, F32)[take]
    feats[n:n + take.size] = 0.0 if init_feats is None else np.asarray(init_feats, F32)[take]
    counters = [int(flags.size), int(((flags & VALID) != 0).sum()), int(((flags & FREE) != 0).sum()),
                int(kept.size), int(kept.size - take.size)]
    return xyz, feats, counters


def add_frame(xyz, feats, n, depth, c2w, fx, fy, cx, cy, bound, origin, radius_add, thin=None, pixels=None,
              stride=1, rho=(0.0,), init_feats=None, cand_xyz=None):
    """The whole step.  cand_xyz: positions to decide on instead of the restatement's own (teacher
    forcing).  Returns dict(flags, cand_xyz, xyz, feats, counters, n_new)."""
    thin = radius_add if thin is None else thin
    own, dd = candidates(depth, c2w, fx, fy, cx, cy, pixels, stride, rho)
    p = own if cand_xyz is None else np.asarray(cand_xyz, F32)
    flags = decide(p, dd, xyz, n, bound, radius_add, thin, origin)
    x2, f2, counters = append(flags, p, xyz, feats, n, init_feats)
    return dict(flags=flags, cand_xyz=p, xyz=x2, feats=f2, counters=counters, n_new=counters[3] - counters[4])


# ---- float64 yardstick -----------------------------------------------------------------------------
def margins64(p64, cand_depth, xyz, n, bound, radius_add, thin, origin):
    """Per candidate, the smallest relative distance from a decision threshold (float64): the bound
    faces, the ball radius around every existing point, the voxel faces."""
    p = np.asarray(p64, np.float64)
    b = np.asarray(bound, np.float64).reshape(3, 2)
    m = np.full(p.shape[0], np.inf)
    for a in range(3):
        m = np.minimum(m, np.abs(p[:, a] - b[a, 0]) / max(abs(b[a, 0]), 1.0))
        m = np.minimum(m, np.abs(p[:, a] - b[a, 1]) / max(abs(b[a, 1]), 1.0))
    if n > 0:
        x = np.asarray(xyz, np.float64)[:n]
        d = np.sqrt(((p[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        m = np.minimum(m, (np.abs(d - radius_add) / radius_add).min(1))
    if thin > 0:
        t = (p - np.asarray(origin, np.float64)[None, :]) / thin
        m = np.minimum(m, (np.abs(t - np.round(t)) / np.maximum(np.abs(t), 1.0)).min(1))
    return np.where(np.isfinite(np.asarray(cand_depth, np.float64)), m, np.inf)


def brute_force64(p64, cand_depth, xyz, n, bound, radius_add, thin, origin):
    """The flag bytes by the same rules in float64 (exact voxel coordinates, no identity mask)."""
    p = np.asarray(p64, np.float64)
    d = np.asarray(cand_depth, np.float64)
    b = np.asarray(bound, np.float64).reshape(3, 2)
    valid = np.isfinite(d) & (d > 0) & ((p > b[None, :, 0]) & (p < b[None, :, 1])).all(1)
    free = valid.copy()
    if n > 0:
        x = np.asarray(xyz, np.float64)[:n]
        d2 = ((p[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        free &= ~(d2 <= float(radius_add) ** 2).any(1)
    kept = free.copy()
    if thin > 0:
        vox = np.floor((p - np.asarray(origin, np.float64)[None, :]) / thin).astype(np.int64)
        seen = set()
        for c in np.nonzero(free)[0]:
            k = tuple(vox[c])
            kept[c] = k not in seen
            seen.add(k)
    return (valid * VALID + free * FREE + kept * KEPT).astype(np.uint8)
