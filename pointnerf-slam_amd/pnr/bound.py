"""The convex hull behind the mesh bound (src/utils/Mesher.py:214-279), on the host, to a tolerance.

`build_hull` is a quickhull that never holds the point set P: every pass over P is one call of
`support(dirs float32 (D,3)) -> (h float32 (D,), arg int64 (D,))`, the support function of P (on the
device: pnr_bound_support, csrc/bound.hip; in the CPU tests: tests/bound_ref.py), and the positions of
the few points it keeps come from `points_of(idx int64 (n,)) -> float32 (n,3)`.  The routine itself is
numpy / float64 and imports nothing of the HIP library.

  initial tetrahedron   the supports of +-x, +-y, +-z; the two farthest of them; the farthest from their
                        line among the supports of 8 directions around it; the farthest from that plane
                        among the supports of +-normal.  A height <= 10 eps: ValueError (degenerate set).
  facets                oriented triangles with a float64 unit normal n and offset o, outward, and a
                        directed-edge -> facet map.
  round                 ONE support call for every facet not yet settled (the normals rounded to float32).
                        h32 - o <= eps / 2 settles a facet (h32 is recorded); the others propose their arg
                        point.  Proposals are inserted in order of decreasing float64 distance; one that is
                        no more than eps / 2 outside every live facet is skipped; otherwise the facets it
                        sees (n.p - o > 0, connected to the one it is farthest from) are deleted and new
                        ones fanned from the horizon edges.  New facets are unsettled; a queried facet
                        that survives its round is settled with its measured h32.
  stop                  when every facet is settled, or `max_facets` is reached: the unsettled facets are
                        then queried once more and keep their measured h32.
  planes                off = max(o, h32) + g, g = 2^-21 (|nx| X + |ny| Y + |nz| Z) with X, Y, Z the
                        largest |coordinate| (axis supports): the float32 rounding of the direction and of
                        the unfused three-term dot stays within 4 u sum |n_a p_a|, u = 2^-24; g is twice it.
So with V the hull's vertices (rows of P) and H the intersection of the planes' half spaces,
hull(V) <= hull(P) <= H, every point of P satisfies every plane, and -- unless the facet cap stopped the
refinement -- no point of P lies more than eps / 2 outside a facet of hull(V).
"""
from __future__ import annotations

import numpy as np

_AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


class Hull(object):
    """Result of build_hull.  faces (F,3) int64 into vertices (V,3) float64 (rows vertex_index (V,) of P),
    normals (F,3) / offsets (F,) of the triangles, h32 (F,) the measured supports, planes (F,4) = (n, off)
    unscaled, center (3,) the mean of the vertices, extent (3,), capped, stats."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def scale_planes(planes, center, s):
    """The planes of the hull scaled by `s` about `center` (Mesher.py:273): offsets n.c + s (off - n.c)."""
    planes = np.asarray(planes, np.float64)
    nc = planes[:, :3] @ np.asarray(center, np.float64)
    out = planes.copy()
    out[:, 3] = nc + float(s) * (planes[:, 3] - nc)
    return out


def _unit(v):
    return v / np.linalg.norm(v)


def build_hull(support, points_of, eps, max_facets=16384):
    eps = float(eps)
    if not eps > 0:
        raise ValueError('pnr.bound: eps must be positive')
    stats = {'rounds': 0, 'directions': 0, 'support_calls': 0}
    pos = {}

    def sup(d64):
        d32 = np.ascontiguousarray(np.asarray(d64, np.float64).reshape(-1, 3).astype(np.float32))
        h, arg = support(d32)
        stats['directions'] += d32.shape[0]
        stats['support_calls'] += 1
        arg = np.asarray(arg, np.int64).reshape(-1)
        if (arg < 0).any():
            raise ValueError('pnr.bound: the point set holds no valid point')
        return np.asarray(h, np.float32).reshape(-1).astype(np.float64), arg

    def fetch(idx):
        miss = sorted({int(i) for i in idx} - pos.keys())
        if miss:
            xyz = np.asarray(points_of(np.asarray(miss, np.int64)), np.float32).reshape(-1, 3).astype(np.float64)
            for i, p in zip(miss, xyz):
                pos[i] = p
        return np.stack([pos[int(i)] for i in idx])

    degenerate = ValueError('pnr.bound: degenerate point set (no tetrahedron higher than 10 eps)')
    # ---- the initial tetrahedron
    h_ax, arg_ax = sup(_AXES)
    extent = np.array([max(abs(h_ax[0]), abs(h_ax[1])), max(abs(h_ax[2]), abs(h_ax[3])), max(abs(h_ax[4]), abs(h_ax[5]))])
    p_ax = fetch(arg_ax)
    d2 = ((p_ax[:, None, :] - p_ax[None, :, :]) ** 2).sum(-1)
    ia, ib = np.unravel_index(int(np.argmax(d2)), d2.shape)
    a, b = int(arg_ax[ia]), int(arg_ax[ib])
    if not np.sqrt(d2[ia, ib]) > 10 * eps:
        raise degenerate
    line = _unit(pos[b] - pos[a])
    e1 = _unit(np.cross(line, np.eye(3)[int(np.argmin(np.abs(line)))]))
    e2 = np.cross(line, e1)
    ang = np.arange(8) * (np.pi / 4)
    _, arg8 = sup(np.cos(ang)[:, None] * e1[None, :] + np.sin(ang)[:, None] * e2[None, :])
    off_line = np.linalg.norm(np.cross(fetch(arg8) - pos[a], line), axis=1)
    c = int(arg8[int(np.argmax(off_line))])
    if not off_line.max() > 10 * eps:
        raise degenerate
    nrm = _unit(np.cross(pos[b] - pos[a], pos[c] - pos[a]))
    _, arg2 = sup(np.stack([nrm, -nrm]))
    height = np.abs((fetch(arg2) - pos[a]) @ nrm)
    d = int(arg2[int(np.argmax(height))])
    if not height.max() > 10 * eps:
        raise degenerate
    inner = (pos[a] + pos[b] + pos[c] + pos[d]) / 4.0

    # ---- facets
    cap = 64
    V = np.zeros((cap, 3), np.int64)
    N = np.zeros((cap, 3))
    O = np.zeros(cap)
    H32 = np.full(cap, np.nan)
    alive = np.zeros(cap, bool)
    settled = np.zeros(cap, bool)
    n_fac = 0
    n_alive = 0
    edge = {}

    def plane_of(i, j, k):
        pi, pj, pk = pos[i], pos[j], pos[k]
        e_1, e_2 = pj - pi, pk - pi
        cr = np.cross(e_1, e_2)
        nn = np.linalg.norm(cr)
        if not nn > 1e-10 * max(e_1 @ e_1, e_2 @ e_2):
            return None
        n = cr / nn
        return n, float(n @ pi)

    def add_facet(i, j, k, n, o):
        nonlocal V, N, O, H32, alive, settled, cap, n_fac, n_alive
        if n_fac == cap:
            cap *= 2
            V = np.concatenate([V, np.zeros_like(V)])
            N = np.concatenate([N, np.zeros_like(N)])
            O = np.concatenate([O, np.zeros_like(O)])
            H32 = np.concatenate([H32, np.full_like(H32, np.nan)])
            alive = np.concatenate([alive, np.zeros_like(alive)])
            settled = np.concatenate([settled, np.zeros_like(settled)])
        f = n_fac
        V[f], N[f], O[f], alive[f] = (i, j, k), n, o, True
        edge[(i, j)] = edge[(j, k)] = edge[(k, i)] = f
        n_fac += 1
        n_alive += 1

    for i, j, k in ((a, b, c), (a, b, d), (a, c, d), (b, c, d)):
        n, o = plane_of(i, j, k)
        if n @ inner - o > 0:
            j, k, n, o = k, j, -n, -o
        add_facet(i, j, k, n, o)

    def insert(ip):
        nonlocal n_alive
        p = pos[ip]
        dist = N[:n_fac] @ p - O[:n_fac]
        dist[~alive[:n_fac]] = -np.inf
        top = int(np.argmax(dist))
        if not dist[top] > eps / 2:
            return False
        seen = {top}
        stack = [top]
        horizon = []
        while stack:   # the facets p sees, connected to the one it is farthest from
            f = stack.pop()
            i, j, k = (int(x) for x in V[f])
            for e in ((i, j), (j, k), (k, i)):
                g = edge[(e[1], e[0])]
                if g in seen:
                    continue
                if dist[g] > 0:
                    seen.add(g)
                    stack.append(g)
                else:
                    horizon.append(e)
        new = []
        for i, j in horizon:
            pl = plane_of(i, j, ip)
            if pl is None:   # p on the line of a horizon edge: leave the hull as it is
                return False
            new.append((i, j, ip) + pl)
        for f in seen:
            i, j, k = (int(x) for x in V[f])
            for e in ((i, j), (j, k), (k, i)):
                del edge[e]
            alive[f] = False
        n_alive -= len(seen)
        for fac in new:
            add_facet(*fac)
        return True

    capped = False
    while True:
        uns = np.nonzero(alive[:n_fac] & ~settled[:n_fac])[0]
        if uns.size == 0:
            break
        if n_alive >= max_facets:   # the cap: the open facets keep their measured support
            capped = True
            h, _ = sup(N[uns])
            H32[uns] = h
            settled[uns] = True
            break
        stats['rounds'] += 1
        h, arg = sup(N[uns])
        H32[uns] = h
        done = h - O[uns] <= eps / 2
        settled[uns[done]] = True
        prop_f, prop_p = uns[~done], arg[~done]
        if prop_p.size:
            fetch(prop_p)
            best = {}
            for f, ip in zip(prop_f, prop_p):
                dd = float(N[f] @ pos[int(ip)] - O[f])
                best[int(ip)] = max(best.get(int(ip), -np.inf), dd)
            for ip in sorted(best, key=lambda q: (-best[q], q)):
                if n_alive >= max_facets:
                    break
                insert(ip)
        left = uns[alive[uns]]
        settled[left] = True   # (its proposal was within eps / 2 of the hull in float64, or the cap cut the round)

    live = np.nonzero(alive[:n_fac])[0]
    tri = V[live]
    vidx = np.unique(tri)
    vertices = np.stack([pos[int(i)] for i in vidx])
    faces = np.searchsorted(vidx, tri)
    normals, offsets, h32 = N[live].copy(), O[live].copy(), H32[live].copy()
    guard = 2.0 ** -21 * (np.abs(normals) @ extent)
    planes = np.concatenate([normals, (np.maximum(offsets, h32) + guard)[:, None]], 1)
    stats['facets'] = int(live.size)
    stats['vertices'] = int(vidx.size)
    return Hull(faces=faces, vertices=vertices, vertex_index=vidx, normals=normals, offsets=offsets, h32=h32,
                planes=planes, center=vertices.mean(0), extent=extent, capped=capped, stats=stats)
