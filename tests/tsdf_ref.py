"""Numpy float64 restatement of the TSDF volume's three rules (test infrastructure only; include/pnr.h states
them at `pnr_tsdf`), dense over the directory's box and without any culling.

fuse      allocation (the touch rule on the float32 back-projected pixels of bound_ref.positions, birth frames,
          slots in entry order per call, drops past max_blocks) and the per-voxel running average.  A voxel is
          flagged an EDGE when, in any frame that may update it, the float64 values fall within
            1e-3 px of a pixel-rounding boundary (uf or vf near an integer, the image border included),
            |zc| < 1e-5, or |sdf + sdf_trunc| < 1e-5:
          there a float32 evaluation may decide otherwise, and the comparison leaves the voxel out.
          `margin` is the smallest distance, in blocks, from any (p +- sdf_trunc - origin) / block_length to an
          integer: above the float32 rounding of that expression the allocated set is unambiguous.
extract   the zero-crossing rule applied in float64 to given per-slot arrays.
Dense arrays are indexed [z][y][x] over the voxels, [bz][by][bx] over the blocks."""
import numpy as np

import bound_ref

B = 16


def fuse(calls, origin, voxel_length, sdf_trunc, dims, cam, depth_trunc=1000.0, max_blocks=1 << 30):
    """calls: a list of calls, each a list of frames (depth (H,W), color (H,W,3) or None, c2w (4,4)), float32."""
    H, W, fx, fy, cx, cy = cam
    o = np.asarray(origin, np.float32).astype(np.float64)
    vl, tr = float(np.float32(voxel_length)), float(np.float32(sdf_trunc))
    bl = 16.0 * vl
    dims = np.asarray(dims, np.int64)
    X, Y, Z = (o[a] + (np.arange(B * dims[a]) + 0.5) * vl for a in range(3))
    shape = (B * dims[2], B * dims[1], B * dims[0])
    tsdf, weight, rgb = np.zeros(shape), np.zeros(shape), np.zeros(shape + (3,))
    edge = np.zeros(shape, bool)
    slot_of = np.full(dims[::-1], -1, np.int64)
    slots, dropped, margin, coord_max, m_max = [], 0, np.inf, 0.0, 1.0
    up = lambda a: np.repeat(np.repeat(np.repeat(a, B, 0), B, 1), B, 2)
    for frames in calls:
        birth = np.full(dims[::-1], -1, np.int64)
        for k, (depth, color, c2w) in enumerate(frames):
            p, ok = bound_ref.positions(depth[None], c2w[None], fx, fy, cx, cy, 1, depth_trunc)
            p = p[ok & np.isfinite(p).all(1)].astype(np.float64)
            lo, hi = ((p - tr) - o) / bl, ((p + tr) - o) / bl
            for t in (lo, hi):
                near = (t > -1) & (t < dims + 1)
                if near.any():
                    margin = min(margin, np.abs(t - np.round(t))[near].min())
            lo, hi = np.floor(lo).astype(np.int64), np.floor(hi).astype(np.int64)
            for d in np.ndindex(3, 3, 3):
                b = lo + np.array(d)
                m = ((b <= hi) & (b >= 0) & (b < dims)).all(1)
                bz, by, bx = b[m, 2], b[m, 1], b[m, 0]
                fresh = (slot_of[bz, by, bx] == -1) & (birth[bz, by, bx] == -1)
                birth[bz[fresh], by[fresh], bx[fresh]] = k
        new = np.flatnonzero(birth.reshape(-1) >= 0)
        room = max(0, max_blocks - len(slots))
        flat = slot_of.reshape(-1)
        flat[new[:room]] = len(slots) + np.arange(min(room, new.size))
        flat[new[room:]] = -2
        dropped += max(0, new.size - room)
        slots += [int(e) for e in new[:room]]
        birth = np.where(slot_of >= 0, np.maximum(birth, 0), 1 << 30)
        for k, (depth, color, c2w) in enumerate(frames):
            live = up(birth <= k)
            R, t = c2w[:3, :3].astype(np.float64), c2w[:3, 3].astype(np.float64)
            q = [Z[:, None, None] - t[2], Y[None, :, None] - t[1], X[None, None, :] - t[0]]   # q2, q1, q0
            P = [(R[0, c] * q[2] + R[1, c] * q[1]) + R[2, c] * q[0] for c in range(3)]
            zc = -P[2]
            front = live & (zc > 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                uf, vf = fx * P[0] / zc + cx + 0.5, -fy * P[1] / zc + cy + 0.5
            uf, vf = np.where(front, uf, -9.0), np.where(front, vf, -9.0)
            e = live & (np.abs(zc) < 1e-5)
            near_img = front & (uf > -1e-3) & (uf < W + 1e-3) & (vf > -1e-3) & (vf < H + 1e-3)
            e |= near_img & ((np.abs(uf - np.round(uf)) < 1e-3) | (np.abs(vf - np.round(vf)) < 1e-3))
            inside = front & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
            u, v = np.clip(np.floor(uf), 0, W - 1).astype(np.int64), np.clip(np.floor(vf), 0, H - 1).astype(np.int64)
            d = depth[v, u].astype(np.float64)
            with np.errstate(invalid='ignore'):
                seen = inside & np.isfinite(d) & (d > 0) & (d <= float(np.float32(depth_trunc)))
            d = np.where(seen, d, 0.0)
            m = np.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1.0)
            sdf = (d - zc) * m
            e |= seen & (np.abs(sdf + tr) < 1e-5)
            upd = seen & (sdf > -tr)
            s = np.minimum(1.0, sdf / tr)
            w1 = weight + 1.0
            tsdf = np.where(upd, (tsdf * weight + s) / w1, tsdf)
            if color is not None:
                rgb = np.where(upd[..., None], (rgb * weight[..., None] + color[v, u].astype(np.float64)) / w1[..., None], rgb)
            weight = np.where(upd, w1, weight)
            edge |= e
            coord_max = max(coord_max, np.abs(t).max(), np.abs(d).max(), np.abs(zc[seen]).max(initial=0.0))
            m_max = max(m_max, m[seen].max(initial=1.0))
    coord_max = max(coord_max, np.abs(X).max(), np.abs(Y).max(), np.abs(Z).max())
    return dict(tsdf=tsdf, weight=weight, rgb=rgb, edge=edge, slots=np.array(slots, np.int64), dropped=dropped,
                margin=margin, allocated=up(slot_of >= 0), coord_max=coord_max, m_max=m_max)


def block_view(dense, entry, dims):
    """The (16,16,16[,3]) block of directory entry `entry` of a dense array, indexed [k][j][i]."""
    bx, by, bz = entry % dims[0], (entry // dims[0]) % dims[1], entry // (dims[0] * dims[1])
    return dense[B * bz:B * bz + B, B * by:B * by + B, B * bx:B * bx + B]


def extract(tsdf, weight, rgb, index, origin, voxel_length, dims):
    """Per-slot arrays (n,16,16,16) [k][j][i], rgb (n,3,16,16,16), index (n,) entries -> (xyz, rgb) float64 in
    (slot, voxel index, axis) order."""
    o = np.asarray(origin, np.float32).astype(np.float64)
    vl = float(np.float32(voxel_length))
    shape = tuple(B * d + 1 for d in dims[::-1])     # one more plane per axis: the far faces see weight 0
    T, Wt, C = np.zeros(shape), np.zeros(shape), np.zeros(shape + (3,))
    for s, e in enumerate(index):
        block_view(T, e, dims)[...], block_view(Wt, e, dims)[...] = tsdf[s], weight[s]
        block_view(C, e, dims)[...] = rgb[s].transpose(1, 2, 3, 0)
    here = (slice(0, -1),) * 3
    cross, frac, col = [], [], []
    for a in range(3):                               # the +x, +y, +z neighbour: array axes 2, 1, 0
        there = tuple(slice(1, None) if ax == 2 - a else slice(0, -1) for ax in range(3))
        cross.append((Wt[here] > 0) & (Wt[there] > 0) & (T[here] * T[there] < 0))
        with np.errstate(divide='ignore', invalid='ignore'):
            frac.append(T[here] / (T[here] - T[there]))
            col.append(C[here] + (C[there] - C[here]) * frac[a][..., None])
    cross, frac, col = np.stack(cross, -1), np.stack(frac, -1), np.stack(col, -2)
    xyz, out = [], []
    for e in index:
        bx, by, bz = e % dims[0], (e // dims[0]) % dims[1], e // (dims[0] * dims[1])
        k, j, i, a = np.nonzero(block_view(cross, e, dims))
        p = o[None, :] + (np.stack([bx * B + i, by * B + j, bz * B + k], 1) + 0.5) * vl
        p[np.arange(len(a)), a] += vl * block_view(frac, e, dims)[k, j, i, a]
        xyz.append(p)
        out.append(block_view(col, e, dims)[k, j, i, a])
    return np.concatenate(xyz), np.concatenate(out)
