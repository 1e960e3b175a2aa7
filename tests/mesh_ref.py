"""Float64 numpy restatements the mesh-extraction tests compare against (test infrastructure only).

  point_masks_ref   Mesher.point_masks (src/utils/Mesher.py:53-212) in float64, plus every point's
                    smallest relative margin to a decision threshold, so that a test can leave out
                    the points whose answer depends on fp32 rounding (the *edge points*).
  crossing_set      the grid edges a level set crosses and the linear-interpolation crossing on each
                    (the vertex set of any marching-cubes variant), in cell units.
  mesh topology helpers (directed-edge counts, signed volume).

numpy only: the fixture generators import this file under interpreters without torch.
"""
import numpy as np

EDGE_MARGIN = 1e-4   # ~100x the rounding of the fp32 three-term sums behind every compared value
MODES = ('poses', 'maxdepth', 'depthtest')


def _grid_sample(depth, u, v):
    """F.grid_sample(bilinear, align_corners=True, padding_mode='zeros') of depth (H,W) at pixel
    coordinates (u, v) that went through the reference's normalise / unnormalise pair."""
    H, W = depth.shape
    ix = ((u / (W - 1) * 2.0 - 1.0) + 1.0) / 2.0 * (W - 1)
    iy = ((v / (H - 1) * 2.0 - 1.0) + 1.0) / 2.0 * (H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros_like(ix)
    for dy in (0, 1):
        for dx in (0, 1):
            xs, ys = x0 + dx, y0 + dy
            w = (1.0 - np.abs(ix - xs)) * (1.0 - np.abs(iy - ys))
            ok = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1) & np.isfinite(ix) & np.isfinite(iy)
            xi = np.where(ok, xs, 0).astype(np.int64)
            yi = np.where(ok, ys, 0).astype(np.int64)
            out += np.where(ok, depth[yi, xi] * w, 0.0)
    return out


def _rel(a, b, scale):
    """|a - b| relative to the larger compared magnitude (and the magnitude of the terms behind a)."""
    den = np.maximum(np.maximum(np.abs(a), np.abs(b)), scale)
    return np.abs(a - b) / np.maximum(den, 1e-300)


def point_masks_ref(points, w2c, H, W, fx, fy, cx, cy, mode, depth=None, batch=500000):
    """points (N,3) float32, w2c (K,4,4) float32 (the host inverse the reference takes), depth
    (K,H,W) float32 for the two depth modes.  mode: 'poses' (get_mask_use_all_frames), 'maxdepth'
    (depth_test=False) or 'depthtest'.  Returns seen, forecast, unseen (bool) and margin (float64):
    the smallest relative distance of any compared value of the point from its threshold."""
    assert mode in MODES
    pts = np.asarray(points, dtype=np.float32).astype(np.float64)
    w2c = np.asarray(w2c, dtype=np.float32).astype(np.float64)
    N = pts.shape[0]
    seen_all, fore_all, margin_all = np.zeros(N, bool), np.zeros(N, bool), np.full(N, np.inf)
    for s in range(0, N, batch):
        p = pts[s:s + batch]
        seen, fore, margin = np.zeros(len(p), bool), np.zeros(len(p), bool), np.full(len(p), np.inf)
        for k in range(w2c.shape[0]):
            M = w2c[k]
            terms = np.abs(M[:3, None, :3] * p[None, :, :]).sum(-1) + np.abs(M[:3, 3])[:, None]   # (3,n)
            cam = p @ M[:3, :3].T + M[:3, 3]
            x, y, zc = -cam[:, 0], cam[:, 1], cam[:, 2]
            z = zc + np.float64(np.float32(1e-8))
            with np.errstate(divide='ignore', invalid='ignore'):
                u = (fx * x + cx * zc) / z
                v = (fy * y + cy * zc) / z
                az = np.abs(z)
                su = (fx * terms[0] + cx * terms[2]) / az + np.abs(u) * terms[2] / az
                sv = (fy * terms[1] + cy * terms[2]) / az + np.abs(v) * terms[2] / az
            front = z < 0
            cs = (u < W) & (u > 0) & (v < H) & (v > 0) & front
            cf = (u < W + 1000) & (u > -1000) & (v < H + 1000) & (v > -1000) & front
            m = _rel(z, 0.0, terms[2])
            for val, sc, hi in ((u, su, W), (v, sv, H)):
                for b in (0.0, float(hi), -1000.0, float(hi) + 1000.0):
                    m = np.minimum(m, np.nan_to_num(_rel(val, b, sc), nan=np.inf))
            proj = -zc
            if mode == 'maxdepth':
                md = np.float64(np.float32(depth[k].max()) * np.float32(1.1))
                cs &= proj < md
                cf &= proj < md
                m = np.minimum(m, _rel(proj, md, terms[2]))
            elif mode == 'depthtest':
                ds = _grid_sample(depth[k].astype(np.float64), u, v)
                md = ds.max()
                cf &= proj < md
                cs &= (proj < ds + 2.4) & (ds - 2.4 < proj)
                m = np.minimum(m, _rel(proj, md, terms[2]))
                m = np.minimum(m, _rel(proj, ds + 2.4, terms[2]))
                m = np.minimum(m, _rel(proj, ds - 2.4, terms[2]))
            seen |= cs
            fore |= cf
            margin = np.minimum(margin, m)
        fore &= ~seen
        seen_all[s:s + batch], fore_all[s:s + batch], margin_all[s:s + batch] = seen, fore, margin
    return seen_all, fore_all, ~(seen_all | fore_all), margin_all


def crossing_set(vol, level):
    """Crossings of `level` on the grid edges of vol (nx,ny,nz) float32: an edge crosses when exactly
    one of its two samples is < level; the crossing is a + t (b - a) with t = (level - a)/(b - a) in
    float64.  Returns (n,3) float64 positions in cell units, sorted lexicographically."""
    v = np.asarray(vol, dtype=np.float32).astype(np.float64)
    below = v < level
    out = []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        idx = np.argwhere(below[lo] != below[hi])
        a, b = v[lo][tuple(idx.T)], v[hi][tuple(idx.T)]
        pos = idx.astype(np.float64)
        pos[:, ax] += (level - a) / (b - a)
        out.append(pos)
    out = np.concatenate(out, 0)
    return out[np.lexsort(out.T[::-1])]


def sort_rows(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    return a[np.lexsort(a.T[::-1])]


def match_rows(a, b, tol):
    """One-to-one match of the rows of a to the rows of b within `tol` per axis: the permutation
    perm with |a - b[perm]| <= tol, or None (nearest row in the max norm, brute force in chunks)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    if a.shape != b.shape:
        return None
    perm = np.empty(len(a), np.int64)
    for s in range(0, len(a), 256):
        d = np.abs(a[s:s + 256, None, :] - b[None, :, :]).max(-1)
        perm[s:s + 256] = d.argmin(1)
        if (d.min(1) > tol).any():
            return None
    if len(np.unique(perm)) != len(perm):
        return None
    return perm


def directed_edges(faces):
    """{(i, j): count} over the directed edges of the faces (F,3)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    return {(int(i), int(j)): int(c) for (i, j), c in zip(uniq, cnt)}


def edge_report(faces):
    """(manifold, boundary, bad): undirected edges used exactly twice in opposite directions, used
    once, and everything else."""
    d = directed_edges(faces)
    manifold = boundary = bad = 0
    for (i, j), c in d.items():
        r = d.get((j, i), 0)
        if i == j or c > 1 or r > 1:
            bad += 1
        elif r == 1:
            manifold += i < j
        else:
            boundary += 1
    return manifold, boundary, bad


def boundary_edges(faces):
    """The (i, j) directed edges without their opposite."""
    d = directed_edges(faces)
    return [e for e in d if (e[1], e[0]) not in d]


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def vertex_normals_np(vertices, faces):
    """pnr.mesher.vertex_normals in numpy (area-weighted triangle normals, normalised)."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    tn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for a in range(3):
        np.add.at(n, f[:, a], tn)
    norm = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(norm > 0, n / np.where(norm > 0, norm, 1.0), np.array([0.0, 0.0, 1.0]))


def load_case_table(path):
    """(ntri[256], tri[256][3 MC_MAX_TRI]) parsed from the generated csrc/mc_table.h."""
    import re
    text = open(path).read()
    ntri = [int(x) for x in re.search(r'MC_NTRI\[256\] = \{(.*?)\};', text, re.S).group(1).replace('\n', ' ').split(',')
            if x.strip()]
    rows = re.findall(r'^  \{([0-9, ]+)\},$', text, re.M)
    tri = [[int(x) for x in r.split(',')] for r in rows]
    assert len(ntri) == 256 and len(tri) == 256
    return ntri, tri


def marching_cubes_np(vol, level, table, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """csrc/mesh.hip restated: vol (nx,ny,nz) float32 -> vertices (V,3) float64, faces (F,3) int32 in
    the kernel's order (grid points in (ix, iy, iz) row-major order; per point its x, y, z edge)."""
    ntri, tri = table
    v = np.asarray(vol, dtype=np.float32)
    nx, ny, nz = v.shape
    below = v.astype(np.float64) < float(level)
    vid = -np.ones((nx, ny, nz, 3), np.int64)
    verts = []
    for ix in range(nx):
        for iy in range(ny):
            for iz in range(nz):
                for a, (jx, jy, jz) in enumerate(((ix + 1, iy, iz), (ix, iy + 1, iz), (ix, iy, iz + 1))):
                    if jx < nx and jy < ny and jz < nz and below[ix, iy, iz] != below[jx, jy, jz]:
                        s0, s1 = float(v[ix, iy, iz]), float(v[jx, jy, jz])
                        p = [float(ix), float(iy), float(iz)]
                        p[a] += (float(level) - s0) / (s1 - s0)
                        vid[ix, iy, iz, a] = len(verts)
                        verts.append([origin[k] + p[k] * spacing[k] for k in range(3)])
    faces = []
    for ix in range(nx - 1):
        for iy in range(ny - 1):
            for iz in range(nz - 1):
                case = 0
                for c in range(8):
                    case |= int(below[ix + (c & 1), iy + ((c >> 1) & 1), iz + (c >> 2)]) << c
                for t in range(ntri[case]):
                    f = []
                    for e in tri[case][3 * t:3 * t + 3]:
                        a, db, dc = e >> 2, e & 1, (e >> 1) & 1
                        off = [0, 0, 0]
                        b, c2 = [i for i in range(3) if i != a]
                        off[b], off[c2] = db, dc
                        f.append(vid[ix + off[0], iy + off[1], iz + off[2], a])
                    faces.append(f)
    return (np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3))
