"""The mesh bound on the device (csrc/bound.hip, pnr.mesher.FrameBound) against its numpy specification
(tests/bound_ref.py), exactly: the support function and the positions bit for bit, the containment test
byte for byte, the hull from frames equal to pnr.bound.build_hull driven by the specification, and
Mesher.get_mesh with mesh_bound_mask='frames'.

Shapes: 3 keyframes of 24 x 40 (2,880 point slots = two full 1,024-slot tiles and a ragged third, one
workgroup each); direction counts on both sides of the wave (63 / 64 / 65), of the one- / two- / four-
directions-per-thread kernels (300, 600) and of the library's cap (1,025: the host splits); one larger
pair of frames (532 tiles, more than the persistent grid has workgroups, so a workgroup walks several
tiles).  Point counts of the containment on both sides of a 256-thread workgroup and beyond one, facet
counts on both sides of the 256-plane LDS stage."""
import types

import numpy as np
import pytest
import torch

import bound_ref
from conftest import golden_params
from test_gpu_mesh_extract import E2E_SCALE, scene_box
from test_gpu_parity import make_decoder, make_renderer

pytestmark = pytest.mark.gpu

K, H, W = 3, 24, 40
CAM = dict(fx=30.0, fy=28.0, cx=19.5, cy=11.5)
N0 = K * H * W


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def pose(ax, ay, az, t):
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = Rz @ Ry @ Rx, t
    return m.astype(np.float32)


def small_frames(tie=False):
    """depth (K,H,W) with zeros, a negative, inf, nan and one value above depth_trunc; c2w (K,4,4)."""
    rng = np.random.RandomState(11)
    depth = rng.uniform(0.5, 2.5, (K, H, W)).astype(np.float32)
    depth[0, 0, :7] = 0.0
    depth[1, 5, 3] = -1.0
    depth[1, 23, 39] = np.inf
    depth[2, 12, 0] = np.nan
    depth[2, 3, 9] = 1500.0
    depth[0, 6, 6] = 0.0
    c2w = np.stack([pose(0.1, 0.2, -0.3, [0.2, -0.1, 0.3]), pose(-0.4, 1.1, 0.2, [-0.3, 0.2, 0.1]),
                    pose(0.7, -2.0, 0.5, [0.1, 0.4, -0.2])])
    if tie:
        depth[2], c2w[2] = depth[0], c2w[0]
    return depth, c2w


EXTRA = np.array([[3.5, 0.1, -0.2], [-0.4, -3.25, 0.3], [0.0, 0.5, 4.0]], np.float32)


def frame_points(pnr, dev, depth, c2w, stride=1, extra=None, depth_trunc=1000.0):
    return pnr.mesher.FramePoints(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), CAM['fx'], CAM['fy'],
                                  CAM['cx'], CAM['cy'], stride=stride, depth_trunc=depth_trunc, extra=extra)


def directions(n, seed=5):
    rng = np.random.RandomState(seed)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d = rng.randn(max(n, 6), 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[1:7] = axes if n >= 7 else d[1:7]
    return d[:n].astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_spec_cache = {}


def spec(stride, n_extra, tie=False):
    key = (stride, n_extra, tie)
    if key not in _spec_cache:
        depth, c2w = small_frames(tie)
        _spec_cache[key] = bound_ref.positions(depth, c2w, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], stride, 1000.0,
                                               EXTRA[:n_extra])
    return _spec_cache[key]


# ---- the support function and the positions --------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('n_extra', [0, 3])
def test_support_and_points_exact(dev, stride, n_extra):
    import pnr
    depth, c2w = small_frames()
    xyz, valid = spec(stride, n_extra)
    fp = frame_points(pnr, dev, depth, c2w, stride, EXTRA[:n_extra])
    assert fp.n_index == N0 + n_extra == xyz.shape[0]
    # positions of every index, and of indices outside the set
    idx = np.concatenate([np.arange(fp.n_index), [-1, fp.n_index, fp.n_index + 5, -(1 << 40), 1 << 40]]).astype(np.int64)
    got = fp.points(torch.from_numpy(idx)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (idx.size, 3)
    assert np.isnan(got[fp.n_index:]).all()
    got = got[:fp.n_index]
    assert np.array_equal(np.isnan(got).any(1), ~valid) and np.array_equal(np.isnan(got).all(1), ~valid)
    assert np.array_equal(bits(got[valid]), bits(xyz[valid]))
    n_invalid = int((~valid[:N0]).sum())
    lattice = ((np.arange(H)[:, None] % stride == 0) & (np.arange(W)[None, :] % stride == 0)).sum() * K
    print('stride', stride, 'valid', int(valid.sum()), 'invalid pixels', n_invalid)
    assert valid[:N0].sum() <= lattice and (stride > 1 or n_invalid == 12)
    for D in (1, 2, 63, 64, 65, 300, 600, 1025):
        dirs = directions(D)
        h, arg = fp.support(torch.from_numpy(dirs))
        assert h.dtype == torch.float32 and arg.dtype == torch.int64 and h.shape == (D,) and arg.shape == (D,)
        rh, rarg = bound_ref.support(xyz, valid, dirs)
        assert np.array_equal(bits(h.cpu().numpy()), bits(rh)), D
        assert np.array_equal(arg.cpu().numpy(), rarg), D
        h2, arg2 = fp.support(torch.from_numpy(dirs))
        assert torch.equal(h, h2) and torch.equal(arg, arg2)
    assert fp.max_dirs == 1024


def test_support_tie_takes_the_smaller_index(dev):
    import pnr
    depth, c2w = small_frames(tie=True)
    xyz, valid = spec(1, 0, tie=True)
    assert np.array_equal(bits(xyz[:H * W]), bits(xyz[2 * H * W:]))
    fp = frame_points(pnr, dev, depth, c2w)
    dirs = directions(64, seed=6)
    h, arg = fp.support(torch.from_numpy(dirs))
    rh, rarg = bound_ref.support(xyz, valid, dirs)
    arg = arg.cpu().numpy()
    assert np.array_equal(bits(h.cpu().numpy()), bits(rh)) and np.array_equal(arg, rarg)
    assert (arg < 2 * H * W).all() and (arg < H * W).any()


def test_support_without_a_valid_point(dev):
    import pnr
    depth, c2w = small_frames()
    for bad in (np.zeros_like(depth), np.full_like(depth, np.nan), np.full_like(depth, 1500.0)):
        fp = frame_points(pnr, dev, bad, c2w)
        h, arg = fp.support(torch.from_numpy(directions(65)))
        assert bool(torch.isinf(h).all()) and bool((h < 0).all()) and bool((arg == -1).all())
        assert bool(torch.isnan(fp.points(torch.arange(N0))).all())
    # no keyframe at all, and extra points alone
    empty = pnr.mesher.FramePoints(torch.zeros((0, H, W), device=dev), torch.zeros((0, 4, 4), device=dev), **CAM)
    h, arg = empty.support(torch.from_numpy(directions(3)))
    assert bool((h == -np.inf).all()) and bool((arg == -1).all())
    only = pnr.mesher.FramePoints(torch.zeros((0, H, W), device=dev), torch.zeros((0, 4, 4), device=dev), **CAM,
                                  extra=EXTRA)
    dirs = directions(7)
    h, arg = only.support(torch.from_numpy(dirs))
    rh, rarg = bound_ref.support(EXTRA, np.ones(3, bool), dirs)
    assert np.array_equal(bits(h.cpu().numpy()), bits(rh)) and np.array_equal(arg.cpu().numpy(), rarg)


def test_support_many_tiles_per_workgroup(dev):
    """532 tiles of 1,024 slots: more tiles than the persistent grid has workgroups."""
    import pnr
    rng = np.random.RandomState(12)
    Kb, Hb, Wb = 2, 340, 800
    depth = rng.uniform(0.5, 2.5, (Kb, Hb, Wb)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.1] = 0.0
    c2w = small_frames()[1][:Kb]
    cam = dict(fx=600.0, fy=600.0, cx=399.5, cy=169.5)
    xyz, valid = bound_ref.positions(depth, c2w, cam['fx'], cam['fy'], cam['cx'], cam['cy'], 1, 1000.0, EXTRA)
    fp = pnr.mesher.FramePoints(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), **cam, extra=EXTRA)
    for D in (7, 300):
        dirs = directions(D, seed=8)
        h, arg = fp.support(torch.from_numpy(dirs))
        rh, rarg = bound_ref.support(xyz, valid, dirs, chunk=8)
        assert np.array_equal(bits(h.cpu().numpy()), bits(rh)) and np.array_equal(arg.cpu().numpy(), rarg)
    pick = torch.from_numpy(rng.randint(0, xyz.shape[0], 5000).astype(np.int64))
    got = fp.points(pick).cpu().numpy()
    want = xyz[pick.numpy()]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got[~np.isnan(got)]), bits(want[~np.isnan(want)]))


def test_support_argument_errors(dev):
    import ctypes
    import pnr
    from pnr import _lib
    L = _lib.load()
    depth, c2w = small_frames()
    fp = frame_points(pnr, dev, depth, c2w)
    f = fp.frames
    one = ctypes.c_void_p(256)
    assert L.pnr_bound_support_workspace_bytes(ctypes.byref(f), 8) > 0
    assert L.pnr_bound_support_workspace_bytes(ctypes.byref(f), -1) == 0
    assert L.pnr_bound_support_workspace_bytes(ctypes.byref(f), 1025) == 0
    assert L.pnr_bound_support_workspace_bytes(None, 8) == 0
    assert L.pnr_bound_support(None, one, 1, one, one, one, 1 << 20, None) == -1
    assert L.pnr_bound_support(ctypes.byref(f), None, 1, one, one, one, 1 << 20, None) == -1
    assert L.pnr_bound_support(ctypes.byref(f), one, -1, one, one, one, 1 << 20, None) == -1
    assert L.pnr_bound_support(ctypes.byref(f), one, 4, one, one, one, 16, None) == -2
    assert L.pnr_bound_support(ctypes.byref(f), one, 0, None, None, None, 0, None) == 0
    bad = _lib.BoundFrames.from_buffer_copy(f)
    bad.stride = 0
    assert L.pnr_bound_support_workspace_bytes(ctypes.byref(bad), 8) == 0
    assert L.pnr_bound_points(ctypes.byref(bad), one, 1, one, None) == -1
    bad = _lib.BoundFrames.from_buffer_copy(f)
    bad.K = -1
    assert L.pnr_bound_support(ctypes.byref(bad), one, 1, one, one, one, 1 << 20, None) == -1
    bad = _lib.BoundFrames.from_buffer_copy(f)
    bad.depth = None
    assert L.pnr_bound_support(ctypes.byref(bad), one, 1, one, one, one, 1 << 20, None) == -1
    assert L.pnr_bound_points(ctypes.byref(f), None, 1, one, None) == -1
    assert L.pnr_bound_points(ctypes.byref(f), None, 0, None, None) == 0
    assert L.pnr_bound_contains_f32(None, 5, one, 1, one, None) == -1
    assert L.pnr_bound_contains_f64(one, 5, None, 1, one, None) == -1
    assert L.pnr_bound_contains_f64(one, -1, one, 1, one, None) == -1
    assert L.pnr_bound_contains_f32(None, 0, None, 0, None, None) == 0


# ---- containment -----------------------------------------------------------------------------------
def planes_for(F):
    """The slab |x|, |y| <= 0.5 first, then random planes that leave the slab's faces' centres inside."""
    rng = np.random.RandomState(F + 1)
    box = np.array([[1, 0, 0, 0.5], [-1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, -1, 0, 0.5]], np.float64)
    n = rng.randn(max(F, 4), 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    rnd = np.concatenate([n, rng.uniform(0.75, 1.5, (n.shape[0], 1))], 1)
    return np.concatenate([box, rnd])[:F]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('F', [0, 4, 12, 300])
def test_contains_exact(dev, dtype, F):
    import pnr
    planes = planes_for(F)
    planes_t = torch.from_numpy(planes).to(dev)
    for P in (1, 255, 257, 70001):
        rng = np.random.RandomState(P)
        p = (rng.randn(P, 3) * 0.4).astype(dtype)
        on = np.array([[0.5, 0.1, -0.1], [-0.5, 0.0, 0.2], [0.25, 0.5, 0.0], [0.0, -0.5, -0.25], [0.5, 0.5, 0.0]], dtype)
        p[:min(P, 5)] = on[:min(P, 5)]          # exactly on a plane (or an edge): `<=` keeps them
        if P > 10:
            p[7] = np.nan
        want = bound_ref.contains(p, planes)
        got = pnr.mesher.bound_contains(torch.from_numpy(p).to(dev), planes_t, chunk=65536)
        assert got.dtype == torch.bool and got.is_cuda and got.shape == (P,)
        assert np.array_equal(got.cpu().numpy(), want), (P, F)
        assert want[:min(P, 5)].all()
        if F > 0 and P > 10:
            assert not want[7] and 0 < want.sum() < P
        if F == 0:
            assert want.all()
        assert torch.equal(got, pnr.mesher.bound_contains(p, planes_t))    # numpy input, one chunk


# ---- the hull from frames --------------------------------------------------------------------------
def test_hull_from_frames_is_the_host_hull_of_the_spec(dev):
    import pnr
    depth, c2w = small_frames()
    keyframes = [{'depth': torch.from_numpy(depth[k]).to(dev), 'est_c2w': torch.from_numpy(c2w[k])} for k in range(K)]
    fb = pnr.mesher.get_bound_from_frames(keyframes, H, W, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], scale=1.0,
                                          bound_scale=1.02, device=dev)
    xyz, valid = bound_ref.positions(depth, c2w, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], 1, 1000.0, c2w[:, :3, 3])
    eps = 4.0 / 512
    hull = pnr.bound.build_hull(*bound_ref.oracle(xyz, valid), eps)
    print('facets', fb.stats, 'host', hull.stats)
    assert fb.eps == eps and np.array_equal(fb.faces, hull.faces) and np.array_equal(fb.vertex_index, hull.vertex_index)
    assert np.array_equal(fb.planes_unscaled, hull.planes) and np.array_equal(fb.vertices, hull.vertices)
    want = pnr.bound.scale_planes(hull.planes, hull.center, 1.02)
    assert fb.planes.dtype == torch.float64 and fb.planes.is_cuda and np.array_equal(fb.planes.cpu().numpy(), want)
    assert fb.stats['facets'] == hull.faces.shape[0] >= 4 and fb.stats['directions'] == hull.stats['directions']
    # every valid point, fetched back through pnr_bound_points, is inside -- scaled or not
    fp = frame_points(pnr, dev, depth, c2w, extra=c2w[:, :3, 3])
    pts = fp.points(torch.from_numpy(np.nonzero(valid)[0]))
    assert not bool(torch.isnan(pts).any())
    assert bool(fb.contains(pts).all()) and bool(fb(pts.double()).all())
    assert bool(pnr.mesher.bound_contains(pts, torch.from_numpy(hull.planes).to(dev)).all())
    assert not bool(fb.contains(torch.tensor([[50.0, 0.0, 0.0]])).any())
    # a stride thins the set: still the host hull of the thinned specification
    fb3 = pnr.mesher.get_bound_from_frames(keyframes, H, W, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], device=dev,
                                           stride=3, eps=0.02, max_facets=40)
    x3, v3 = bound_ref.positions(depth, c2w, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], 3, 1000.0, c2w[:, :3, 3])
    h3 = pnr.bound.build_hull(*bound_ref.oracle(x3, v3), 0.02, 40)
    assert np.array_equal(fb3.faces, h3.faces) and np.array_equal(fb3.planes_unscaled, h3.planes)
    assert bool(fb3.contains(torch.from_numpy(x3[v3])).all())
    with pytest.raises(ValueError):
        pnr.mesher.get_bound_from_frames([], H, W, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], device=dev)
    with pytest.raises(ValueError):
        pnr.mesher.get_bound_from_frames([{'depth': torch.zeros(H, W), 'est_c2w': torch.from_numpy(c2w[0])}], H, W,
                                         CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'], device=dev)


# ---- Mesher.get_mesh -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mesh_scene(dev, scene):
    """The small decoder / renderer scene of tests/test_gpu_mesh_extract.py, with the keyframes' depth cut
    to 0.6 of the rendered depth: their hull ends in free space and cuts the level set."""
    import pnr
    Hm, Wm = 24, 32
    cam = dict(H=Hm, W=Wm, fx=16.0, fy=16.0, cx=15.5, cy=11.5)
    r = make_renderer(pnr, scene, ray_batch_size=1000, points_batch_size=5000, **cam)
    dec = make_decoder(pnr, golden_params('trained'), dev)
    slam = types.SimpleNamespace(renderer=r, bound=scene['bound_t'], verbose=False, **cam)
    cfg = dict(pnr.ROOM0_CFG, scale=E2E_SCALE,
               meshing={'resolution': 24, 'remove_small_geometry_threshold': 0.002 / E2E_SCALE ** 2})
    cfg['mapping'] = dict(cfg['mapping'], marching_cubes_bound=(scene['bound'] / E2E_SCALE).tolist())
    m = pnr.Mesher(cfg, None, slam, points_batch_size=5000, ray_batch_size=1000)
    poses = torch.from_numpy(scene['poses'][:2].copy())
    keyframes = [{'est_c2w': poses[k],
                  'depth': 0.6 * r.render_img({}, dec, poses[k].to(dev), dev, 'color')[0].float()} for k in range(2)]
    return dict(mesher=m, dec=dec, keyframes=keyframes, poses=poses)


def test_get_mesh_with_the_frame_bound(dev, mesh_scene, tmp_path):
    import pnr
    m, dec, kfs, poses = (mesh_scene[k] for k in ('mesher', 'dec', 'keyframes', 'poses'))
    path = str(tmp_path / 'm.ply')
    kw = dict(device=dev, color=False, clean_mesh=False)
    fb = m.get_bound_from_frames(kfs, m.scale, device=dev)
    assert isinstance(fb, pnr.mesher.FrameBound) and fb.bound_scale == m.clean_mesh_bound_scale == 1.02
    assert fb.eps == 4.0 * m.scale / 512.0
    grid = m.get_grid_uniform(m.resolution)
    points = grid['grid_points'].to(dev)
    inside = fb.contains(points)
    assert 0 < int(inside.sum()) < points.shape[0]
    by_name = m.get_mesh(path, {}, dec, kfs, poses, 1, mesh_bound_mask='frames', **kw)
    by_tensor = m.get_mesh(path, {}, dec, kfs, poses, 1, mesh_bound_mask=inside, **kw)
    by_object = m.get_mesh(path, {}, dec, kfs, poses, 1, mesh_bound_mask=fb, **kw)
    plain = m.get_mesh(path, {}, dec, kfs, poses, 1, **kw)
    assert by_name is not None and plain is not None
    for other in (by_tensor, by_object):
        assert torch.equal(by_name[0], other[0]) and torch.equal(by_name[1], other[1])
    print('faces with the bound', by_name[1].shape[0], 'without', plain[1].shape[0])
    assert by_name[0].shape != plain[0].shape or not torch.equal(by_name[0], plain[0])
    # every vertex lies on a grid edge with an end inside the scaled hull: within one cell of it
    spacing = np.array([a[2] - a[1] for a in grid['xyz']])
    world = (by_name[0] * m.scale).double()
    excess = (world @ fb.planes[:, :3].T - fb.planes[:, 3][None, :]).max()
    print('largest excess over the scaled hull', float(excess), 'cell diagonal', np.linalg.norm(spacing))
    assert float(excess) <= np.linalg.norm(spacing)
    lo, hi = scene_box(m)
    assert bool((world >= torch.from_numpy(lo).to(dev) - 1e-9).all()) and bool((world <= torch.from_numpy(hi).to(dev) + 1e-9).all())
    # the default call applies no hull mask: the grid query and marching cubes alone
    z = m.eval_points(points, dec, {}, 'fine', dev)[:, -1].contiguous()
    v0, f0 = pnr.mesher.marching_cubes(z, grid['xyz'], m.level_set)
    assert torch.equal(plain[0], v0 / m.scale) and torch.equal(plain[1], f0)
    # with the cleaning and the colours: still the mesh of the tensor mask, bit for bit
    full_name = m.get_mesh(path, {}, dec, kfs, poses, 1, device=dev, mesh_bound_mask='frames')
    full_tensor = m.get_mesh(path, {}, dec, kfs, poses, 1, device=dev, mesh_bound_mask=inside)
    assert full_name is not None and all(torch.equal(a, b) for a, b in zip(full_name, full_tensor))
    with pytest.raises(ValueError):
        m.get_mesh(path, {}, dec, kfs, poses, 1, mesh_bound_mask='hull', **kw)


def test_get_mesh_forecast_face_cull(dev, mesh_scene, tmp_path):
    """show_forecast=True (:475-485): the faces whose three vertices all lie outside the bound are culled
    before the component filter."""
    import pnr
    m, dec, kfs, poses = (mesh_scene[k] for k in ('mesher', 'dec', 'keyframes', 'poses'))
    path = str(tmp_path / 'f.ply')
    kw = dict(device=dev, show_forecast=True, color=False)
    got = m.get_mesh(path, {}, dec, kfs, poses, 1, mesh_bound_mask='frames', **kw)
    raw = m.get_mesh(path, {}, dec, kfs, poses, 1, clean_mesh=False, **kw)
    assert got is not None and raw is not None
    fb = m.get_bound_from_frames(kfs, m.scale, device=dev)
    v0, f0 = raw[0] * m.scale, raw[1]            # (E2E_SCALE is a power of two: exact)
    keep = fb.contains(v0)
    culled = int((~keep)[f0.long()].all(dim=1).sum())
    print('faces', f0.shape[0], 'culled by the bound', culled)
    assert 0 < culled < f0.shape[0]
    cv, cf = pnr.mesher.clean_mesh(v0, f0, keep, threshold=m.remove_small_geometry_threshold * m.scale ** 2)
    assert torch.equal(got[0], cv / m.scale) and torch.equal(got[1], cf)
    assert cf.shape[0] <= f0.shape[0] - culled
