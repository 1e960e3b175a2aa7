"""Mesh extraction on the device (csrc/mesh.hip, pnr.mesher): point masks against the reference
fixture, marching cubes against the skimage fixture and the numpy restatement, the cleaning, and
Mesher.get_mesh end to end.

Tolerances: masks are compared on every non-edge point (tests/mesh_ref.py: relative margin to a decision
threshold >= 1e-4, ~100x the fp32 rounding involved), at most 1% edge points.  Marching-cubes vertices
match skimage within 1e-5 of a cell per axis (20x skimage's own measured 4.8e-7 deviation from the exact
float64 interpolation, tests/golden/make_golden_mc.py) and the float64 numpy crossing within 1e-12."""
import types

import numpy as np
import pytest
import torch

import mesh_ref
from conftest import golden_params, load_golden
from test_gpu_parity import make_decoder, make_renderer
from test_mesh_extract import SMOOTH, TABLE_H, fixture_mesh, parse_ply

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def masks():
    return load_golden('masks.npz')


@pytest.fixture(scope='module')
def mc():
    return load_golden('mc.npz')


@pytest.fixture(scope='module')
def table():
    return mesh_ref.load_case_table(TABLE_H)


def device_mc(dev, vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    import pnr
    v, f = pnr.mesher.marching_cubes_volume(torch.from_numpy(np.ascontiguousarray(vol)).to(dev), level, spacing, origin)
    assert v.dtype == torch.float64 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v.cpu().numpy(), f.cpu().numpy()


def assert_is_restatement(v, f, vol, level, table, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """The device mesh is the numpy restatement's: same order, same faces, same float64 vertices."""
    rv, rf = mesh_ref.marching_cubes_np(vol, level, table, spacing, origin)
    assert v.shape == rv.shape and np.array_equal(f, rf)
    np.testing.assert_allclose(v, rv, rtol=0, atol=1e-12 * max(1.0, float(np.abs(rv).max()) if rv.size else 1.0))


def on_border(cells, shape, i, j):
    """Both vertices lie in one border face of the volume (cell units)."""
    for a in range(3):
        for b in (0.0, shape[a] - 1.0):
            if abs(cells[i, a] - b) < 1e-9 and abs(cells[j, a] - b) < 1e-9:
                return True
    return False


# ---- point masks -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', mesh_ref.MODES)
def test_point_masks_vs_reference(dev, masks, mode):
    import pnr
    H, W, fx, fy, cx, cy = masks['intr']
    H, W, batch = int(H), int(W), int(masks['batch'])
    keyframes = [{'est_c2w': torch.from_numpy(masks['c2w'][k]), 'depth': torch.from_numpy(masks['depth'][k]).to(dev)}
                 for k in range(masks['c2w'].shape[0])]
    est = torch.from_numpy(masks['c2w'])

    def run():
        return pnr.mesher.point_masks(torch.from_numpy(masks['points']), keyframes, est, est.shape[0] - 1, H, W, fx, fy,
                                      cx, cy, dev, depth_test=mode == 'depthtest',
                                      get_mask_use_all_frames=mode == 'poses', points_batch_size=batch)

    seen, fore, unseen = run()
    assert seen.dtype == torch.bool and seen.is_cuda and seen.shape == (masks['points'].shape[0],)
    w2c = np.stack([np.linalg.inv(m) for m in masks['c2w']])
    margin = mesh_ref.point_masks_ref(masks['points'], w2c, H, W, fx, fy, cx, cy, mode, masks['depth'], batch)[3]
    edge = margin < mesh_ref.EDGE_MARGIN
    assert edge.mean() <= 0.01
    for name, got in (('seen', seen), ('forecast', fore), ('unseen', unseen)):
        got = got.cpu().numpy()
        want = masks[f'{mode}/{name}']
        print(mode, name, 'differing points', int((got != want).sum()), 'of them off the edges',
              int((got != want)[~edge].sum()))
        assert np.array_equal(got[~edge], want[~edge]), name
    assert torch.equal(unseen, ~(seen | fore)) and not bool((seen & fore).any())
    for a, b in zip((seen, fore, unseen), run()):
        assert torch.equal(a, b)


def test_point_masks_without_keyframes(dev, masks):
    import pnr
    seen, fore, unseen = pnr.mesher.point_masks(torch.from_numpy(masks['points'][:100]), [], None, 0, 48, 64, 40., 40.,
                                                31.5, 23.5, dev)
    assert not bool(seen.any()) and not bool(fore.any()) and bool(unseen.all())


# ---- marching cubes --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SMOOTH)
def test_marching_cubes_smooth(dev, mc, table, name):
    import pnr
    vol, level, sp = mc[f'{name}/vol'], float(mc[f'{name}/level']), mc['spacing']
    v, f = device_mc(dev, vol, level, sp)
    fv, ff = fixture_mesh(mc, name)
    perm = mesh_ref.match_rows(v / sp, fv / sp, 1e-5)
    assert perm is not None, 'vertices do not match the Lewiner fixture one-to-one'
    assert len(f) == len(ff)
    ours = pnr.mesher.vertex_normals(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)).cpu().numpy()
    theirs = pnr.mesher.vertex_normals(torch.from_numpy(fv).to(dev), torch.from_numpy(ff).to(dev)).cpu().numpy()
    dots = (ours * theirs[perm]).sum(1)
    print(name, 'min normal dot', dots.min())
    assert dots.min() > 0
    manifold, boundary, bad = mesh_ref.edge_report(f)
    assert bad == 0
    if name == 'plane':
        cells = v / sp
        assert boundary > 0 and all(on_border(cells, vol.shape, i, j) for i, j in mesh_ref.boundary_edges(f))
    else:
        assert boundary == 0
    if name == 'sphere':
        v_ours, v_fix = mesh_ref.signed_volume(v, f), mesh_ref.signed_volume(fv, ff)
        analytic = np.sign(v_fix) * 4.0 / 3.0 * np.pi * float(mc['sphere_radius']) ** 3
        print('sphere volumes: ours', v_ours, 'fixture', v_fix, 'analytic', analytic)
        assert v_ours * v_fix > 0 and abs(v_ours - v_fix) <= abs(v_fix - analytic)
    assert_is_restatement(v, f, vol, level, table, sp)
    v2, f2 = device_mc(dev, vol, level, sp)
    assert np.array_equal(v, v2) and np.array_equal(f, f2)


def test_marching_cubes_noise(dev, mc, table):
    vol, level, sp = mc['noise/vol'], float(mc['noise/level']), mc['spacing']
    v, f = device_mc(dev, vol, level, sp)
    fv, ff = fixture_mesh(mc, 'noise')
    cells = v / sp
    assert mesh_ref.match_rows(cells, fv / sp, 1e-5) is not None
    assert mesh_ref.match_rows(cells, mesh_ref.crossing_set(vol, level), 1e-12 * max(vol.shape)) is not None
    manifold, boundary, bad = mesh_ref.edge_report(f)
    assert bad == 0
    assert boundary == mesh_ref.edge_report(ff)[1]
    assert all(on_border(cells, vol.shape, i, j) for i, j in mesh_ref.boundary_edges(f))
    assert_is_restatement(v, f, vol, level, table, sp)
    v2, f2 = device_mc(dev, vol, level, sp)
    assert np.array_equal(v, v2) and np.array_equal(f, f2)


def test_marching_cubes_all_256_patterns(dev, table):
    """Each corner sign pattern as a 2x2x2 block padded to 4x4x4 with the outside value: a closed,
    consistently oriented surface around the below-level corners."""
    one = np.where(np.arange(64).reshape(4, 4, 4) == 21, -1.0, 1.0).astype(np.float32)
    sign = mesh_ref.signed_volume(*device_mc(dev, one, 0.0))
    for case in range(256):
        vol = np.full((4, 4, 4), 1.0, np.float32)
        for c in range(8):
            if (case >> c) & 1:
                vol[1 + (c & 1), 1 + ((c >> 1) & 1), 1 + (c >> 2)] = -1.0
        v, f = device_mc(dev, vol, 0.0)
        manifold, boundary, bad = mesh_ref.edge_report(f)
        assert boundary == 0 and bad == 0, case
        assert (len(f) > 0) == (case != 0)
        if case:
            assert mesh_ref.signed_volume(v, f) * sign > 0, case
            assert len(np.unique(f)) == len(v), case


@pytest.mark.parametrize('shape', [(67, 5, 3), (3, 5, 67), (2, 2, 2), (5, 1, 4), (1, 1, 1)])
def test_marching_cubes_shapes(dev, table, shape):
    """67 samples on one axis: more than one 256-thread workgroup of grid points, with cells and shared
    vertices across the workgroup boundary; the smallest volume with a cell; volumes without a cell."""
    vol = np.random.RandomState(sum(shape)).randn(*shape).astype(np.float32)
    sp, org = (0.5, 0.25, 2.0), (-1.0, 3.0, 0.125)
    v, f = device_mc(dev, vol, 0.05, sp, org)
    assert_is_restatement(v, f, vol, 0.05, table, sp, org)
    if min(shape) >= 2:
        assert len(f) > 0 and mesh_ref.edge_report(f)[2] == 0
    else:
        assert len(f) == 0


def test_marching_cubes_empty(dev):
    for fill in (1.0, -1.0):
        v, f = device_mc(dev, np.full((6, 7, 5), fill, np.float32), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_marching_cubes_strides(dev, table):
    """The reference's flat (ny, nx, nz) grid order read through strides, and a sliced view: bitwise the
    mesh of a contiguous copy."""
    import pnr
    rng = np.random.RandomState(9)
    nx, ny, nz = 7, 6, 5
    x, y, z = np.linspace(-1.0, 2.0, nx), np.linspace(0.0, 1.0, ny), np.linspace(3.0, 5.0, nz)
    flat = torch.from_numpy(rng.randn(ny * nx * nz).astype(np.float32)).to(dev)
    v, f = pnr.mesher.marching_cubes(flat, [x, y, z], 0.1)
    vol = flat.reshape(ny, nx, nz).permute(1, 0, 2)
    assert not vol.is_contiguous()
    sp, org = (x[2] - x[1], y[2] - y[1], z[2] - z[1]), (x[0], y[0], z[0])
    vc, fc = pnr.mesher.marching_cubes_volume(vol.contiguous(), 0.1, sp, org)
    assert torch.equal(v, vc) and torch.equal(f, fc) and f.shape[0] > 0
    assert_is_restatement(v.cpu().numpy(), f.cpu().numpy(), vol.cpu().numpy(), 0.1, table, sp, org)
    big = torch.from_numpy(rng.randn(13, 9, 14).astype(np.float32)).to(dev)
    view = big[::2, 1:, 1::3]
    vs, fs = pnr.mesher.marching_cubes_volume(view, 0.0)
    vc, fc = pnr.mesher.marching_cubes_volume(view.contiguous(), 0.0)
    assert torch.equal(vs, vc) and torch.equal(fs, fc) and fs.shape[0] > 0


# ---- cleaning --------------------------------------------------------------------------------------
def test_clean_mesh_two_spheres(dev):
    import pnr
    g = np.stack(np.meshgrid(*[np.arange(24.0)] * 3, indexing='ij'), -1)
    c_big, c_small = np.array([7.3, 7.2, 7.1]), np.array([17.2, 17.3, 17.1])
    vol = np.minimum(np.linalg.norm(g - c_big, axis=-1) - 5.0, np.linalg.norm(g - c_small, axis=-1) - 2.5)
    v, f = pnr.mesher.marching_cubes_volume(torch.from_numpy(vol.astype(np.float32)).to(dev), 0.0)
    near_big = (v - torch.from_numpy(c_big).to(dev)).norm(dim=1) < 6.0
    area = pnr.mesher.face_areas(v, f)
    of_big = near_big[f[:, 0].long()]
    a_big, a_small = float(area[of_big].sum()), float(area[~of_big].sum())
    assert 0 < a_small < 0.5 * a_big
    seen = torch.ones(v.shape[0], dtype=torch.bool, device=dev)
    want_v, want_f = v[near_big], f[of_big]
    for kw in (dict(threshold=0.5 * (a_small + a_big)), dict(largest=True)):
        cv, cf = pnr.mesher.clean_mesh(v, f, seen, **kw)
        assert cv.is_cuda and cf.is_cuda and cf.dtype == torch.int32 and cv.dtype == torch.float64
        assert torch.equal(cv, want_v) and cf.shape == want_f.shape
        assert int(cf.min()) == 0 and int(cf.max()) == cv.shape[0] - 1
        assert torch.equal(cv[cf.long()], v[want_f.long()])            # the same triangles, in the same order
        assert mesh_ref.edge_report(cf.cpu().numpy())[1:] == (0, 0)
    cv, cf = pnr.mesher.clean_mesh(v, f, seen, threshold=0.5 * a_small)
    assert torch.equal(cv, v) and torch.equal(cf, f)
    cv, cf = pnr.mesher.clean_mesh(v, f, ~seen, threshold=0.5 * a_small)
    assert cv.shape == (0, 3) and cf.shape == (0, 3)
    # a face stays when one of its vertices is seen: seeing only the small sphere's vertices keeps it alone
    cv, cf = pnr.mesher.clean_mesh(v, f, ~near_big)
    assert torch.equal(cv, v[~near_big]) and cf.shape[0] == int((~of_big).sum())
    assert int(cf.min()) == 0 and int(cf.max()) == cv.shape[0] - 1


# ---- end to end ------------------------------------------------------------------------------------
E2E_SCALE = 0.5   # a power of two: (v / scale) * scale is exact, so the colours can be recomputed bitwise


@pytest.fixture(scope='module')
def e2e(dev, scene, tmp_path_factory):
    import pnr
    H, W = 24, 32
    cam = dict(H=H, W=W, fx=16.0, fy=16.0, cx=15.5, cy=11.5)
    r = make_renderer(pnr, scene, ray_batch_size=1000, points_batch_size=5000, **cam)
    dec = make_decoder(pnr, golden_params('trained'), dev)
    slam = types.SimpleNamespace(renderer=r, bound=scene['bound_t'], verbose=False, **cam)
    cfg = dict(pnr.ROOM0_CFG, scale=E2E_SCALE,
               meshing={'resolution': 24, 'remove_small_geometry_threshold': 0.002 / E2E_SCALE ** 2})
    cfg['mapping'] = dict(cfg['mapping'], marching_cubes_bound=(scene['bound'] / E2E_SCALE).tolist())
    m = pnr.Mesher(cfg, None, slam, points_batch_size=5000, ray_batch_size=1000)
    poses = torch.from_numpy(scene['poses'][:2].copy())
    keyframes = [{'est_c2w': poses[k], 'depth': r.render_img({}, dec, poses[k].to(dev), dev, 'color')[0].float()}
                 for k in range(2)]
    out = {}
    d = tmp_path_factory.mktemp('mesh')
    for show_forecast in (False, True):
        runs = []
        for rep in range(2):
            path = str(d / f'mesh_{int(show_forecast)}_{rep}.ply')
            res = m.get_mesh(path, {}, dec, keyframes, poses, 1, device=dev, show_forecast=show_forecast)
            runs.append((path, res))
        out[show_forecast] = runs
    return dict(mesher=m, renderer=r, dec=dec, keyframes=keyframes, poses=poses, runs=out)


@pytest.mark.parametrize('show_forecast', [False, True])
def test_get_mesh_end_to_end(dev, e2e, show_forecast):
    import pnr
    m, r, dec = e2e['mesher'], e2e['renderer'], e2e['dec']
    (path, res), (path2, res2) = e2e['runs'][show_forecast]
    assert res is not None
    v, f, col = res
    print('show_forecast', show_forecast, 'vertices', v.shape[0], 'faces', f.shape[0])
    assert v.shape[0] > 0 and f.shape[0] > 0 and col.shape == v.shape and col.dtype == torch.uint8
    # the file parses and holds the returned mesh
    pv, pf, pc = parse_ply(path)
    assert np.array_equal(pv, v.cpu().numpy().astype(np.float32))
    assert np.array_equal(pf, f.cpu().numpy()) and np.array_equal(pc, col.cpu().numpy())
    # the faces index the (compacted) vertices
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0] and len(torch.unique(f)) == v.shape[0]
    # the coordinates are divided by scale (bit for bit in test_get_mesh_is_its_stages): scaled back they
    # lie in the marching-cubes grid's box
    world = v * E2E_SCALE
    lo = torch.from_numpy(scene_box(m)[0]).to(dev)
    hi = torch.from_numpy(scene_box(m)[1]).to(dev)
    assert bool((world >= lo - 1e-9).all()) and bool((world <= hi + 1e-9).all())
    # the colours are mesh_colors of the returned mesh (cyan on the forecast vertices)
    want = torch.from_numpy(pnr.mesher.mesh_colors(r, dec, {}, world, f, dev, m.color_mesh_extraction_method)).to(dev)
    if show_forecast:
        fore = m.point_masks(world, e2e['keyframes'], e2e['poses'], 1, dev)[1]
        want[fore] = torch.tensor([0, 255, 255], dtype=torch.uint8, device=dev)
    assert torch.equal(col, want)
    # two runs are bitwise equal, file included
    assert all(torch.equal(a, b) for a, b in zip(res, res2))
    assert open(path, 'rb').read() == open(path2, 'rb').read()


def scene_box(m):
    b = m.marching_cubes_bound.numpy()
    return b[:, 0] - 0.05, b[:, 1] + 0.05


def test_get_mesh_is_its_stages(dev, e2e):
    """show_forecast=False restated stage by stage: grid query, marching cubes, the seen-vertex cull and
    the component filter give the returned mesh bit for bit."""
    import pnr
    m, dec = e2e['mesher'], e2e['dec']
    v, f, _ = e2e['runs'][False][0][1]
    grid = m.get_grid_uniform(m.resolution)
    z = m.eval_points(grid['grid_points'].to(dev), dec, {}, 'fine', dev)[:, -1].contiguous()
    v0, f0 = pnr.mesher.marching_cubes(z, grid['xyz'], m.level_set)
    seen = m.point_masks(v0, e2e['keyframes'], e2e['poses'], 1, dev)[0]
    cv, cf = pnr.mesher.clean_mesh(v0, f0, seen, threshold=m.remove_small_geometry_threshold * m.scale ** 2)
    assert 0 < cf.shape[0] < f0.shape[0]
    assert torch.equal(cv / m.scale, v) and torch.equal(cf, f)


def test_get_mesh_bound_mask_and_no_surface(dev, e2e, tmp_path):
    m, dec = e2e['mesher'], e2e['dec']
    v, f, _ = e2e['runs'][False][0][1]
    path = str(tmp_path / 'masked.ply')
    centre = m.marching_cubes_bound.mean(dim=1).to(dev)

    def inside(p):
        return (p.to(dev).double() - centre).norm(dim=1) < 0.3

    res = m.get_mesh(path, {}, dec, e2e['keyframes'], e2e['poses'], 1, device=dev, color=False, clean_mesh=False,
                     mesh_bound_mask=inside)
    assert res is not None and res[2] is None
    assert bool(((res[0] * m.scale - centre).norm(dim=1) < 0.3 + 0.1).all())
    # a mask that leaves nothing inside: occupancy 100 everywhere, no surface at level 10
    assert m.get_mesh(path, {}, dec, e2e['keyframes'], e2e['poses'], 1, device=dev,
                      mesh_bound_mask=lambda p: torch.zeros(p.shape[0], dtype=torch.bool, device=dev)) is None
