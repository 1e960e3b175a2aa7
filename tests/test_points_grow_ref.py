"""Growing the neural-point map, CPU side: the numpy restatement (tests/points_grow_ref.py) against a
brute-force float64 version of the same rules, the thinning rule's invariants, and the host logic of
`pnr.NeuralPoints(capacity=...)` / `add_frame` that needs no GPU."""
import copy
import pickle

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (repo paths)
import points_grow_ref as G

H, W, FX, FY, CX, CY = 48, 64, 50.0, 51.0, 31.5, 23.5
BOUND = np.array([[-1.0, 1.2], [-0.9, 1.0], [-1.6, 0.4]])
RADIUS = 0.05
RHO = (-0.02, 0.0, 0.02)


def camera():
    a, b = 0.2, -0.15
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    c2w = np.eye(4)
    c2w[:3, :3] = ry @ rx
    c2w[:3, 3] = [0.1, 0.05, 0.3]
    return c2w.astype(np.float32)


def frame(seed=0):
    """A depth image whose surface leaves the bound on one side, with holes, over a cloud that covers
    part of the surface."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depth = (1.0 + 0.25 * np.sin(u / 9.0) + 0.2 * np.cos(v / 7.0) + 0.012 * u).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = 0.0
    c2w = camera()
    p64, _ = G.candidates(depth, c2w, FX, FY, CX, CY, dtype=np.float64)
    ok = np.isfinite(p64).all(1) & (depth.reshape(-1) > 0)
    near = p64[ok][rng.choice(ok.sum(), 300, replace=False)][:, :]
    near = near[near[:, 0] < 0.3]  # the cloud covers the surface's low-x part only
    xyz = (near + 0.02 * rng.standard_normal(near.shape)).astype(np.float32)
    return depth, c2w, xyz


def test_restatement_matches_float64_brute_force():
    depth, c2w, xyz = frame()
    n = xyz.shape[0]
    origin = (BOUND[:, 0] - 0.11).astype(np.float32)
    p64, d64 = G.candidates(depth, c2w, FX, FY, CX, CY, rho=RHO, dtype=np.float64)
    m = G.margins64(p64, d64, xyz, n, BOUND, RADIUS, RADIUS, origin)
    # float32 positions carry ~1e-7 relative error: pixels with every candidate 1e-4 clear of an edge
    clear = (m.reshape(-1, len(RHO)) > 1e-4).all(1)
    pixels = np.nonzero(clear)[0]
    assert pixels.size > 0.9 * H * W
    sel = (pixels[:, None] * len(RHO) + np.arange(len(RHO))[None, :]).reshape(-1)
    ref = G.brute_force64(p64[sel], d64[sel], xyz, n, BOUND, RADIUS, RADIUS, origin)
    cap = n + 5000
    xyz_c = np.concatenate([xyz, np.zeros((cap - n, 3), np.float32)])
    out = G.add_frame(xyz_c, np.zeros((cap, 32), np.float32), n, depth, c2w, FX, FY, CX, CY, BOUND, origin, RADIUS,
                      pixels=pixels, rho=RHO)
    assert np.abs(out['cand_xyz'][np.isfinite(d64[sel])] - p64[sel][np.isfinite(d64[sel])]).max() < 1e-6
    assert np.array_equal(out['flags'], ref)
    c = out['counters']
    assert c[0] == sel.size and c[0] > c[1] > c[2] > c[3] > 0 and c[4] == 0
    assert c[0] - c[1] > 0.02 * c[0] and c[1] - c[2] > 0.05 * c[0] and c[2] - c[3] > 0.05 * c[0]
    # appended in candidate order, nothing else touched
    kept = np.nonzero(out['flags'] & G.KEPT)[0]
    assert np.array_equal(out['xyz'][n:n + kept.size], out['cand_xyz'][kept])
    assert np.array_equal(out['xyz'][:n], xyz) and not out['xyz'][n + kept.size:].any()


def test_thinning_invariants_and_capacity():
    depth, c2w, xyz = frame(seed=1)
    n = xyz.shape[0]
    origin = (BOUND[:, 0] - 0.11).astype(np.float32)
    cap = n + 40
    xyz_c = np.concatenate([xyz, np.full((cap - n, 3), 7.0, np.float32)])
    feats_c = np.full((cap, 32), 3.0, np.float32)
    init = np.random.default_rng(2).standard_normal((H * W * 3, 32)).astype(np.float32)
    out = G.add_frame(xyz_c, feats_c, n, depth, c2w, FX, FY, CX, CY, BOUND, origin, RADIUS, thin=0.08, rho=RHO,
                      init_feats=init)
    fl, p = out['flags'], out['cand_xyz']
    free, kept = np.nonzero(fl & G.FREE)[0], np.nonzero(fl & G.KEPT)[0]
    key = G.voxel_key(p, origin, 0.08)
    assert np.unique(key[kept]).size == kept.size                      # one survivor per voxel
    assert set(key[kept]) == set(key[free])                            # every occupied voxel has one
    first = {}
    for c in free:
        first.setdefault(key[c], c)
    assert sorted(first.values()) == kept.tolist()                     # and it is the minimum index
    assert ((fl & G.KEPT) == 0)[(fl & G.FREE) == 0].all() and ((fl & G.FREE) == 0)[(fl & G.VALID) == 0].all()
    # capacity: the first 40 kept candidates in candidate order, the rest dropped
    assert kept.size > 40 and out['counters'][3:] == [kept.size, kept.size - 40] and out['n_new'] == 40
    assert np.array_equal(out['xyz'][n:], p[kept[:40]]) and np.array_equal(out['feats'][n:], init[kept[:40]])
    assert np.array_equal(out['feats'][:n], feats_c[:n])
    # no thinning: every free candidate is kept
    out0 = G.add_frame(xyz_c, feats_c, n, depth, c2w, FX, FY, CX, CY, BOUND, origin, RADIUS, thin=0.0, rho=RHO)
    assert np.array_equal((out0['flags'] & G.KEPT) != 0, (out0['flags'] & G.FREE) != 0)


def test_pixel_list_and_stride_orders():
    depth, c2w, _ = frame()
    p_all, _ = G.candidates(depth, c2w, FX, FY, CX, CY)
    pix = np.array([W * 5 + 3, W * 5 + 3, H * W - 1, 0, -1, H * W])
    p, d = G.candidates(depth, c2w, FX, FY, CX, CY, pixels=pix, rho=(0.0, 0.5))
    assert np.array_equal(p[0::2][:4], p_all[pix[:4]]) and np.isnan(d[8:]).all() and not p[8:].any()
    ps, _ = G.candidates(depth, c2w, FX, FY, CX, CY, stride=3)
    v, u = np.meshgrid(np.arange(0, H, 3), np.arange(0, W, 3), indexing='ij')
    assert np.array_equal(ps, p_all[(v * W + u).reshape(-1)])


def test_capacity_host_logic():
    from pnr import NeuralPoints
    xyz = torch.rand((10, 3))
    with pytest.raises(ValueError):
        NeuralPoints(xyz, capacity=9)
    with pytest.raises(ValueError):
        NeuralPoints(torch.zeros((0, 3)), capacity=16)             # empty: no origin to derive
    with pytest.raises(RuntimeError):
        NeuralPoints(xyz).add_frame(torch.zeros((4, 4)), torch.eye(4), 4, 4, 1., 1., 0., 0., BOUND)
    plain = NeuralPoints(xyz)
    assert plain.capacity is None and plain.n_points == 10 and plain._struct().n_points == 10
    pts = NeuralPoints(xyz, torch.ones((10, 32)), capacity=4096, radius=0.05)
    assert pts.n_points == 10 and pts.xyz.shape == (4096, 3) and pts.feats.shape == (4096, 32)
    assert torch.equal(pts.xyz[:10], xyz) and not pts.xyz[10:].any() and not pts.feats[10:].any()
    assert pts._struct().n_points == 10
    assert pts.table_bits == 11 and plain.table_bits == 10             # from the capacity
    assert pts.origin == pytest.approx((xyz.min(0).values - pts.cell).tolist())
    empty = NeuralPoints(torch.zeros((0, 3)), capacity=64, bound=BOUND, radius=0.05)
    assert empty.n_points == 0 and empty.origin == pytest.approx((BOUND[:, 0] - empty.cell).tolist())
    with pytest.raises(ValueError):                                    # the probe must cover the ball
        pts.add_frame(torch.zeros((4, 4)), torch.eye(4), 4, 4, 1., 1., 0., 0., BOUND, radius_add=0.051)
    # the live count travels with the object
    pts._n = 12
    for clone in (copy.deepcopy(pts), pickle.loads(pickle.dumps(pts))):
        assert clone.n_points == 12 and clone.capacity == 4096 and clone._struct().n_points == 12
        assert clone._index is None
    # a checkpoint holds the live rows and the capacity
    from pnr.logger import c_from_state, c_state
    st = c_state({'points_color': pts})['points_color']
    assert st['xyz'].shape == (12, 3) and st['feats'].shape == (12, 32) and st['capacity'] == 4096
    back = c_from_state({'points_color': st})['points_color']
    assert back.n_points == 12 and back.capacity == 4096 and back.origin == pts.origin and back.table_bits == 11
    assert 'capacity' not in c_state({'points_color': plain})['points_color']
    old = pts.__getstate__()
    for k in ('_n', 'capacity', 'last_add'):
        old.pop(k)
    back = NeuralPoints.__new__(NeuralPoints)
    back.__setstate__(old)                                             # a state saved before clouds grew
    assert back.n_points == 4096 and back.capacity is None


def test_binding_names_both_entry_points():
    import ctypes
    from pnr import _lib
    assert 'pnr_points_add_workspace_bytes' in _lib.SYMBOLS and 'pnr_points_add_frame' in _lib.SYMBOLS
    assert _lib.PointsAdd.rho.offset == 64 and _lib.PointsAdd.bound.offset == 104
    assert _lib.PointsAdd.init_feats.offset == 128 and ctypes.sizeof(_lib.PointsAdd) == 152
    L = _lib.load()
    assert L.pnr_points_add_workspace_bytes(-1) == 0
    small, big = L.pnr_points_add_workspace_bytes(1), L.pnr_points_add_workspace_bytes(9216)
    assert 0 < small < big and big >= 9216 * (16 + 1 + 12) + 32768 * 12  # rows + the 2x power-of-two table
    assert L.pnr_points_add_frame(None, 0, None, None, None, None, 0, None, None) == -1
