"""pnr.bound.build_hull on the numpy oracle (tests/bound_ref.py): no GPU, no libpnr.so.

The bounds are the routine's own contract (pnr/bound.py): a closed triangulated surface whose vertices are
rows of P, every point of P inside every plane, and no point more than eps / 2 outside a facet unless the
facet cap stopped the refinement.  The facet counts are held within 4x the figures of the prototype runs
(116 facets for the noiseless room, 232 at 1 % depth noise)."""
import numpy as np
import pytest

import bound_ref
from pnr import bound

EPS_ROOM = 7.8e-4         # the prototype runs' eps (a tenth of the default 4 scale / 512 at scale 1)


def closed_surface(faces):
    """Every directed edge once, with its twin; returns the undirected edge count."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    directed = {(int(i), int(j)) for i, j in e}
    assert len(directed) == len(e), 'a directed edge appears twice'
    assert all((j, i) in directed for i, j in directed), 'an edge without its twin'
    return len(e) // 2


def check_outer(hull, P, eps=None):
    F, V = hull.faces.shape[0], hull.vertices.shape[0]
    E = closed_surface(hull.faces)
    assert V - E + F == 2
    assert np.array_equal(hull.vertices, P[hull.vertex_index].astype(np.float64))
    assert len(np.unique(hull.faces)) == V
    assert bound_ref.contains(P, hull.planes).all()
    excess = (P.astype(np.float64) @ hull.normals.T - hull.offsets[None, :]).max()
    print('facets', F, 'vertices', V, 'stats', hull.stats, 'largest excess', excess)
    if eps is not None:
        assert excess <= eps / 2
    return excess


def room_points(noise, seed=3):
    """A rotated 0.6 x 0.4 x 0.3 room seen from 8 cameras inside it: 8,000 wall hits per camera (64k
    points), the depth along each ray multiplied by 1 + noise N(0,1), plus the camera centres."""
    rng = np.random.RandomState(seed)
    half = np.array([0.3, 0.2, 0.15])
    ax, ay, az = 0.3, -0.5, 0.7
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R, t = Rz @ Ry @ Rx, np.array([0.1, -0.2, 0.05])
    pts = []
    cams = rng.uniform(-0.6, 0.6, (8, 3)) * half
    for o in cams:
        d = rng.randn(8000, 3)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        with np.errstate(divide='ignore'):
            hit = np.where(d > 0, (half - o) / d, (-half - o) / d).min(1)
        pts.append(o + d * (hit * (1.0 + noise * rng.randn(8000)))[:, None])
    pts.append(cams)
    return (np.concatenate(pts) @ R.T + t).astype(np.float32)


def cube_points():
    rng = np.random.RandomState(0)
    corners = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
    return np.concatenate([rng.uniform(-0.45, 0.45, (2500, 3)), corners, rng.uniform(-0.45, 0.45, (2500, 3))]).astype(
        np.float32)


def test_imports_without_the_library():
    import sys
    assert 'pnr.bound' in sys.modules and bound.build_hull.__module__ == 'pnr.bound'
    assert not any(hasattr(bound, n) for n in ('torch', '_lib', 'ctypes'))


def test_binding_mirrors_the_header_struct():
    """pnr_bound_frames (include/pnr.h): 2 pointers, 4 int32, 5 floats, pad, pointer, int64."""
    import ctypes
    from pnr import _lib
    assert ctypes.sizeof(_lib.BoundFrames) == 72
    assert _lib.BoundFrames.K.offset == 16 and _lib.BoundFrames.fx.offset == 32
    assert _lib.BoundFrames.depth_trunc.offset == 48 and _lib.BoundFrames.extra_xyz.offset == 56
    assert _lib.BoundFrames.n_extra.offset == 64
    for name in ('pnr_bound_support_workspace_bytes', 'pnr_bound_support', 'pnr_bound_points',
                 'pnr_bound_contains_f32', 'pnr_bound_contains_f64', 'pnr_bound_support_max_dirs'):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 14


def test_cube():
    P, eps = cube_points(), 1e-4
    hull = bound.build_hull(*bound_ref.oracle(P), eps)
    assert hull.faces.shape == (12, 3) and hull.vertices.shape == (8, 3) and not hull.capped
    assert np.array_equal(np.abs(hull.vertices), np.full((8, 3), 0.5))
    check_outer(hull, P, eps)
    np.testing.assert_allclose(hull.center, 0.0, atol=1e-15)
    centres = np.concatenate([np.eye(3), -np.eye(3)])
    assert bound_ref.contains(centres * 0.5, hull.planes).all()
    assert not bound_ref.contains(centres * (0.5 + 2 * eps), hull.planes).any()
    assert bound_ref.contains(centres * (0.5 + 2 * eps) * 0.99, hull.planes).all()


@pytest.mark.parametrize('noise,prototype_facets', [(0.0, 116), (0.01, 232)])
def test_room(noise, prototype_facets):
    P = room_points(noise)
    assert P.shape == (64008, 3)
    hull = bound.build_hull(*bound_ref.oracle(P), EPS_ROOM)
    assert not hull.capped
    check_outer(hull, P, EPS_ROOM)
    assert 4 <= hull.faces.shape[0] <= 4 * prototype_facets
    assert hull.stats['facets'] == hull.faces.shape[0] and hull.stats['rounds'] >= 1
    assert hull.stats['directions'] >= 6 + 8 + 2 + hull.faces.shape[0]


def test_invalid_rows_are_not_points():
    """NaN rows flagged invalid are never hull vertices and never counted."""
    P = room_points(0.0)
    Q = np.concatenate([np.full((5, 3), np.nan, np.float32), P])
    valid = np.concatenate([np.zeros(5, bool), np.ones(P.shape[0], bool)])
    a = bound.build_hull(*bound_ref.oracle(P), EPS_ROOM)
    b = bound.build_hull(*bound_ref.oracle(Q, valid), EPS_ROOM)
    assert np.array_equal(a.faces, b.faces) and np.array_equal(a.planes, b.planes)
    assert np.array_equal(a.vertex_index + 5, b.vertex_index)


def test_sphere_facet_cap():
    rng = np.random.RandomState(1)
    P = rng.randn(2000, 3)
    P = (0.3 * P / np.linalg.norm(P, axis=1, keepdims=True)).astype(np.float32)
    hull = bound.build_hull(*bound_ref.oracle(P), 1e-5, max_facets=64)
    assert hull.capped and 64 <= hull.faces.shape[0] < 64 + 64
    excess = check_outer(hull, P)
    assert excess > 1e-5 / 2                      # the refinement did stop early ...
    assert bound_ref.contains(P, hull.planes).all()   # ... and the planes still hold every point
    full = bound.build_hull(*bound_ref.oracle(P), 1e-5)
    assert not full.capped and full.faces.shape[0] > hull.faces.shape[0]
    check_outer(full, P, 1e-5)


def test_degenerate_sets_raise():
    rng = np.random.RandomState(2)
    flat = np.concatenate([rng.uniform(-1, 1, (500, 2)), np.full((500, 1), 0.25)], 1).astype(np.float32)
    with pytest.raises(ValueError):
        bound.build_hull(*bound_ref.oracle(flat), 1e-4)
    line = (np.linspace(-1, 1, 100)[:, None] * np.array([[1.0, 2.0, 3.0]])).astype(np.float32)
    with pytest.raises(ValueError):
        bound.build_hull(*bound_ref.oracle(line), 1e-4)
    with pytest.raises(ValueError):
        bound.build_hull(*bound_ref.oracle(np.zeros((0, 3), np.float32)), 1e-4)
    with pytest.raises(ValueError):
        bound.build_hull(*bound_ref.oracle(flat[:10], np.zeros(10, bool)), 1e-4)


def test_scaling_about_the_centre():
    P = cube_points() + np.float32(0.25)
    hull = bound.build_hull(*bound_ref.oracle(P), 1e-4)
    scaled = bound.scale_planes(hull.planes, hull.center, 1.02)
    assert np.array_equal(scaled[:, :3], hull.planes[:, :3])
    dist = hull.planes[:, 3] - hull.planes[:, :3] @ hull.center
    dist_scaled = scaled[:, 3] - scaled[:, :3] @ hull.center
    np.testing.assert_allclose(dist, 0.5, atol=1e-6)
    np.testing.assert_allclose(dist_scaled, 1.02 * dist, rtol=1e-12)
    assert np.array_equal(bound.scale_planes(hull.planes, hull.center, 1.0)[:, 3], hull.planes[:, 3]) or np.allclose(
        bound.scale_planes(hull.planes, hull.center, 1.0), hull.planes, rtol=0, atol=1e-15)
