"""Numpy restatement of the TSDF volume's mesh rules (test infrastructure only; include/pnr.h states them at
`pnr_tsdf_mesh_count`): corner and cell validity, edge ownership, float32 positions and colours in the kernel's
operation order, and the (slot, voxel index, axis) / (slot, cell, case table) orders."""
import numpy as np

from tsdf_ref import B, block_view


def mesh(tsdf, weight, rgb, index, origin, voxel_length, dims, table):
    """Per-slot arrays (n,16,16,16) [k][j][i], rgb (n,3,16,16,16) or None, index (n,) entries ->
    dict(verts (V,3) float32, faces (F,3) int32, rgb (V,3) float32, crossing (V,) bool: tsdf0 tsdf1 < 0,
    block_axes (F,) the number of axes along which the face's cell reaches into the next block)."""
    ntri, tri = table
    o, vl = np.asarray(origin, np.float32), np.float32(voxel_length)
    shape = tuple(B * d + 1 for d in dims[::-1])      # one more plane per axis, never valid: np.roll wraps into it
    T, C, ok = np.zeros(shape, np.float32), np.zeros(shape + (3,), np.float32), np.zeros(shape, bool)
    for s, e in enumerate(index):
        block_view(T, e, dims)[...], block_view(ok, e, dims)[...] = tsdf[s], weight[s] > 0
        if rgb is not None:
            block_view(C, e, dims)[...] = rgb[s].transpose(1, 2, 3, 0)
    below = ok & (T < 0)
    sh = lambda a, dz, dy, dx: np.roll(a, (-dz, -dy, -dx), (0, 1, 2))   # a at (z + dz, y + dy, x + dx)
    corners = [(c >> 2, (c >> 1) & 1, c & 1) for c in range(8)]          # (dz, dy, dx) of corner c
    cell = np.logical_and.reduce([sh(ok, *d) for d in corners])
    case = sum(sh(below, *d).astype(np.int64) << c for c, d in enumerate(corners)) * cell
    has, vid = np.zeros(shape + (3,), bool), np.full(shape + (3,), -1, np.int64)
    for a in range(3):                                 # world axis a is array axis 2 - a
        around = np.zeros(shape, bool)
        for p, q in ((0, 0), (1, 0), (0, 1), (1, 1)):  # the four cells around the edge: -1 along the other two axes
            d = [0, 0, 0]
            d[(4 - a) % 3], d[(3 - a) % 3] = -p, -q
            around |= sh(cell, *d)
        has[..., a] = (below != sh(below, *[int(ax == 2 - a) for ax in range(3)])) & around
    verts, cols, crossing, faces, axes, n = [], [], [], [], [], 0
    for e in index:
        bx, by, bz = e % dims[0], (e // dims[0]) % dims[1], e // (dims[0] * dims[1])
        k, j, i, a = np.nonzero(block_view(has, e, dims))             # C order: voxel index, then axis
        block_view(vid, e, dims)[k, j, i, a] = n + np.arange(len(a))
        n += len(a)
        g = np.stack([bx * B + i, by * B + j, bz * B + k], 1)
        p = o[None, :] + (g.astype(np.float32) + np.float32(0.5)) * vl
        z0, y0, x0 = g[:, 2], g[:, 1], g[:, 0]
        z1, y1, x1 = z0 + (a == 2), y0 + (a == 1), x0 + (a == 0)
        t0, t1 = T[z0, y0, x0], T[z1, y1, x1]
        s = t0 / (t0 - t1)
        p[np.arange(len(a)), a] += vl * s
        verts.append(p)
        cols.append(C[z0, y0, x0] + (C[z1, y1, x1] - C[z0, y0, x0]) * s[:, None])
        crossing.append(t0 * t1 < 0)
    for e in index:
        lo = B * np.array([e // (dims[0] * dims[1]), (e // dims[0]) % dims[1], e % dims[0]])
        for k, j, i in zip(*np.nonzero(block_view(case, e, dims))):
            cs, at = int(block_view(case, e, dims)[k, j, i]), lo + (k, j, i)
            for t in range(ntri[cs]):
                f = []
                for ed in tri[cs][3 * t:3 * t + 3]:
                    a, off = ed >> 2, [0, 0, 0]
                    b, c = [x for x in range(3) if x != a]
                    off[b], off[c] = ed & 1, (ed >> 1) & 1
                    f.append(vid[at[0] + off[2], at[1] + off[1], at[2] + off[0], a])
                faces.append(f)
                axes.append(sum(int(x == B - 1) for x in (i, j, k)))
    cat = lambda x, w: np.concatenate(x) if x else np.zeros((0,) + w)
    return dict(verts=cat(verts, (3,)).astype(np.float32), rgb=cat(cols, (3,)).astype(np.float32),
                faces=np.asarray(faces, np.int32).reshape(-1, 3), crossing=cat(crossing, ()).astype(bool),
                block_axes=np.asarray(axes, np.int64))
