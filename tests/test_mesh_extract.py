"""Mesh extraction without a GPU: the float64 restatement of Mesher.point_masks against the reference
fixture (tests/golden/masks.npz), the skimage fixture (tests/golden/mc.npz) against the numpy crossing
set, the generated case table (csrc/mc_table.h) through a numpy restatement of the kernel, the PLY
writer, the cleaning (torch ops, run here on CPU tensors) and the new C-ABI argument checks.

Edge points: a point whose smallest relative margin to a decision threshold (u / v bounds, z < 0,
max_depth, +-2.4) is below 1e-4 of the larger compared magnitude -- ~100x the rounding of the fp32
three-term sums involved -- may differ between fp32 and float64; at most 1% of the fixture's points
may be such points."""
import ctypes
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

import mesh_ref
from conftest import REPO, load_golden

TABLE_H = os.path.join(REPO, 'pointnerf-slam_amd', 'csrc', 'mc_table.h')
SMOOTH = ('sphere', 'blobs', 'plane')


@pytest.fixture(scope='module')
def masks():
    return load_golden('masks.npz')


@pytest.fixture(scope='module')
def mc():
    return load_golden('mc.npz')


@pytest.fixture(scope='module')
def table():
    return mesh_ref.load_case_table(TABLE_H)


def fixture_mesh(mc, name):
    """The skimage mesh a volume is pinned to: Lewiner (the reference's call) on the smooth volumes,
    Lorensen on the noise volume (Lewiner adds cell-centre vertices there)."""
    if name == 'noise':
        return mc['noise/verts_lorensen'].astype(np.float64), mc['noise/faces_lorensen']
    return mc[f'{name}/verts'].astype(np.float64), mc[f'{name}/faces']


def w2c_of(masks):
    return np.stack([np.linalg.inv(m) for m in masks['c2w']])


@pytest.mark.parametrize('mode', mesh_ref.MODES)
def test_restatement_equals_reference_off_the_edges(masks, mode):
    H, W, fx, fy, cx, cy = masks['intr']
    seen, fore, unseen, margin = mesh_ref.point_masks_ref(masks['points'], w2c_of(masks), int(H), int(W), fx, fy, cx, cy,
                                                          mode, masks['depth'], int(masks['batch']))
    edge = margin < mesh_ref.EDGE_MARGIN
    print(mode, 'edge points', int(edge.sum()), 'of', edge.size)
    assert edge.mean() <= 0.01
    for name, got in (('seen', seen), ('forecast', fore), ('unseen', unseen)):
        assert np.array_equal(got[~edge], masks[f'{mode}/{name}'][~edge]), name
    assert masks[f'{mode}/seen'].any() and masks[f'{mode}/forecast'].any() and masks[f'{mode}/unseen'].any()


def test_chunk_maximum_matters(masks):
    """The fixture's points_batch_size makes the depth-test mode's per-chunk max_depth visible: one
    chunk over all points gives another forecast mask."""
    H, W, fx, fy, cx, cy = masks['intr']
    args = (masks['points'], w2c_of(masks), int(H), int(W), fx, fy, cx, cy, 'depthtest', masks['depth'])
    a = mesh_ref.point_masks_ref(*args, int(masks['batch']))
    b = mesh_ref.point_masks_ref(*args, 1 << 20)
    assert not np.array_equal(a[1], b[1])


@pytest.mark.parametrize('name', SMOOTH + ('noise',))
def test_crossing_set_equals_fixture_vertices(mc, name):
    verts, _ = fixture_mesh(mc, name)
    cross = mesh_ref.crossing_set(mc[f'{name}/vol'], float(mc[f'{name}/level']))
    cells = verts / mc['spacing']
    perm = mesh_ref.match_rows(cells, cross, 1e-6)
    assert perm is not None
    assert not (mc[f'{name}/vol'] == np.float32(mc[f'{name}/level'])).any()


def test_case_table_is_the_generators(table):
    spec = importlib.util.spec_from_file_location('gen_mc_table', os.path.join(REPO, 'tools', 'gen_mc_table.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ntri, tri = table
    for case, tris in enumerate(gen.table()):
        assert ntri[case] == len(tris)
        assert tri[case][:3 * len(tris)] == [e for t in tris for e in t]
    assert ntri[0] == ntri[255] == 0 and max(ntri) <= 5


def test_all_256_cases_closed_and_oriented(table):
    """Each corner pattern as a 2x2x2 block inside a 4x4x4 volume of the outside value: a closed,
    consistently oriented surface (every edge twice, in opposite directions) -- which needs the
    ambiguous faces of neighbouring cells to agree."""
    one = np.where(np.arange(64).reshape(4, 4, 4) == 21, -1.0, 1.0).astype(np.float32)   # corner 0 alone
    sign = mesh_ref.signed_volume(*mesh_ref.marching_cubes_np(one, 0.0, table))
    for case in range(256):
        vol = np.full((4, 4, 4), 1.0, np.float32)
        for c in range(8):
            if (case >> c) & 1:
                vol[1 + (c & 1), 1 + ((c >> 1) & 1), 1 + (c >> 2)] = -1.0
        v, f = mesh_ref.marching_cubes_np(vol, 0.0, table)
        manifold, boundary, bad = mesh_ref.edge_report(f)
        assert boundary == 0 and bad == 0, case
        assert (len(f) > 0) == (case != 0)
        if case:
            assert mesh_ref.signed_volume(v, f) * sign > 0, case


@pytest.mark.parametrize('name', SMOOTH + ('noise',))
def test_table_against_skimage(mc, table, name):
    """The numpy restatement of the kernel with the generated table against skimage: same vertices,
    same face count and winding on the smooth volumes, same boundary on the noise volume."""
    sp = mc['spacing']
    v, f = mesh_ref.marching_cubes_np(mc[f'{name}/vol'], float(mc[f'{name}/level']), table, sp)
    fv, ff = fixture_mesh(mc, name)
    perm = mesh_ref.match_rows(v / sp, fv / sp, 1e-5)
    assert perm is not None
    manifold, boundary, bad = mesh_ref.edge_report(f)
    assert bad == 0 and boundary == mesh_ref.edge_report(ff)[1]
    if name != 'noise':
        assert len(f) == len(ff)
        dots = (mesh_ref.vertex_normals_np(v, f) * mesh_ref.vertex_normals_np(fv, ff)[perm]).sum(1)
        assert dots.min() > 0


def parse_ply(path):
    """A parser for exactly the PLY dialect write_ply promises."""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int(next(line for line in lines if line.startswith('element vertex')).split()[-1])
    nf = int(next(line for line in lines if line.startswith('element face')).split()[-1])
    props = [line.split()[1:] for line in lines if line.startswith('property')]
    has_col = ['uchar', 'red'] in props
    assert props[:3] == [['float', 'x'], ['float', 'y'], ['float', 'z']]
    assert props[-1] == ['list', 'uchar', 'int', 'vertex_indices']
    assert len(props) == (7 if has_col else 4)
    vsize = 12 + (3 if has_col else 0)
    body = raw[end:]
    assert len(body) == nv * vsize + nf * 13
    verts = np.zeros((nv, 3), np.float32)
    cols = np.zeros((nv, 3), np.uint8) if has_col else None
    for i in range(nv):
        verts[i] = struct.unpack_from('<3f', body, i * vsize)
        if has_col:
            cols[i] = struct.unpack_from('<3B', body, i * vsize + 12)
    faces = np.zeros((nf, 3), np.int32)
    for i in range(nf):
        n, a, b, c = struct.unpack_from('<B3i', body, nv * vsize + i * 13)
        assert n == 3
        faces[i] = (a, b, c)
    return verts, faces, cols


@pytest.mark.parametrize('with_color', [True, False])
def test_ply_round_trip(tmp_path, with_color):
    import pnr
    rng = np.random.RandomState(0)
    v = rng.randn(37, 3)
    f = rng.randint(0, 37, (51, 3)).astype(np.int32)
    col = rng.randint(0, 256, (37, 3)).astype(np.uint8) if with_color else None
    path = str(tmp_path / 'm.ply')
    pnr.mesher.write_ply(path, torch.from_numpy(v), torch.from_numpy(f), col)
    pv, pf, pc = parse_ply(path)
    assert np.array_equal(pv, v.astype(np.float32)) and np.array_equal(pf, f)
    assert (pc is None) if not with_color else np.array_equal(pc, col)
    pnr.mesher.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    pv, pf, _ = parse_ply(path)
    assert pv.shape == (0, 3) and pf.shape == (0, 3)


def test_clean_mesh_on_cpu_tensors(table):
    """clean_mesh is torch ops: the component / area / compaction logic runs here on CPU tensors."""
    import pnr
    g = np.stack(np.meshgrid(*[np.arange(16.0)] * 3, indexing='ij'), -1)
    vol = np.minimum(np.linalg.norm(g - [4.3, 4.2, 4.1], axis=-1) - 3.0,
                     np.linalg.norm(g - [11.2, 11.3, 11.1], axis=-1) - 1.5).astype(np.float32)
    v, f = mesh_ref.marching_cubes_np(vol, 0.0, table)
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    label = pnr.mesher.vertex_components(len(v), ft)
    assert len(torch.unique(label)) == 2
    areas = [float(pnr.mesher.face_areas(vt, ft)[label[ft[:, 0].long()] == lab].sum()) for lab in torch.unique(label)]
    big = max(areas)
    assert min(areas) < 0.5 * big
    all_seen = torch.ones(len(v), dtype=torch.bool)
    for kw in (dict(threshold=0.5 * (min(areas) + big)), dict(largest=True)):
        cv, cf = pnr.mesher.clean_mesh(vt, ft, all_seen, **kw)
        assert 0 < len(cv) < len(v) and int(cf.max()) == len(cv) - 1 and int(cf.min()) == 0
        assert abs(float(pnr.mesher.face_areas(cv, cf).sum()) - big) < 1e-9 * big
        assert np.linalg.norm(cv.numpy() - [4.3, 4.2, 4.1], axis=1).max() < 4.0
        assert mesh_ref.edge_report(cf.numpy())[1:] == (0, 0)
    cv, cf = pnr.mesher.clean_mesh(vt, ft, ~all_seen, threshold=0.0)
    assert cv.shape == (0, 3) and cf.shape == (0, 3)
    cv, cf = pnr.mesher.clean_mesh(vt, ft, None)
    assert torch.equal(cv, vt) and torch.equal(cf, ft)
    # two triangles that share one vertex: one component here (shared vertices), two for trimesh
    tri = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32)
    assert len(torch.unique(pnr.mesher.vertex_components(5, tri))) == 1


def test_mesher_defaults_and_exports():
    import types
    import pnr
    assert pnr.Mesher is pnr.mesher.Mesher and 'Mesher' in pnr.__all__
    assert 'meshing' not in pnr.ROOM0_CFG
    slam = types.SimpleNamespace(renderer=None, bound=None, H=24, W=32, fx=20., fy=20., cx=15.5, cy=11.5)
    m = pnr.Mesher(pnr.ROOM0_CFG, None, slam)
    assert (m.resolution, m.level_set, m.depth_test, m.get_largest_components) == (256, 10, False, False)
    assert m.remove_small_geometry_threshold == 0.2 and m.color_mesh_extraction_method == 'render_ray_along_normal'
    assert m.points_batch_size == 500000 and m.ray_batch_size == 100000
    cfg = dict(pnr.ROOM0_CFG, meshing={'resolution': 24, 'depth_test': True})
    m = pnr.Mesher(cfg, None, slam)
    assert m.resolution == 24 and m.depth_test and m.level_set == 10
    np.testing.assert_allclose(m.marching_cubes_bound.numpy(), np.array(pnr.ROOM0_CFG['mapping']['bound']) * 0.1)


def test_mesh_abi_queries_and_arg_errors():
    from pnr import _lib
    L = _lib.load()
    assert L.pnr_abi_version() == 14
    assert L.pnr_point_masks_workspace_bytes(1000, 3, _lib.MASK_POSES) == 0
    assert L.pnr_point_masks_workspace_bytes(1000, 3, _lib.MASK_MAX_DEPTH) == 0
    assert L.pnr_point_masks_workspace_bytes(1000, 3, _lib.MASK_DEPTH_TEST) >= 3 * (1 + 4) * 4
    assert L.pnr_point_masks(None, 10, None, 1, 4, 4, 1., 1., 1., 1., 0, None, None, None, None, None, 0, None) == -1
    assert L.pnr_point_masks(None, 0, None, 1, 4, 4, 1., 1., 1., 1., 0, None, None, None, None, None, 0, None) == 0
    one = ctypes.c_void_p(16)
    assert L.pnr_point_masks(one, 10, one, 1, 4, 4, 1., 1., 1., 1., 3, None, None, one, one, None, 0, None) == -1
    assert L.pnr_point_masks(one, 10, one, 1, 4, 4, 1., 1., 1., 1., _lib.MASK_MAX_DEPTH, None, None, one, one, None, 0,
                             None) == -1
    assert L.pnr_point_masks(one, 1000, one, 3, 4, 4, 1., 1., 1., 1., _lib.MASK_DEPTH_TEST, one, None, one, one, one, 8,
                             None) == -2
    cap = L.pnr_marching_cubes_max_points()
    assert 256 ** 3 <= cap < 2 ** 31
    assert L.pnr_marching_cubes_workspace_bytes(256, 256, 256) >= 4 * 256 ** 3
    assert L.pnr_marching_cubes_workspace_bytes(0, 4, 4) == 0
    assert L.pnr_marching_cubes_workspace_bytes(cap, 2, 1) == 0
    z3 = (ctypes.c_double * 3)(0, 0, 0)
    assert L.pnr_marching_cubes_count(None, 4, 4, 4, 16, 4, 1, 0.0, None, 0, None, None, None) == -1
    assert L.pnr_marching_cubes_count(one, 4, 4, 4, 16, 4, 1, 0.0, one, 8, one, one, None) == -2
    assert L.pnr_marching_cubes_emit(one, 4, 4, 4, 16, 4, 1, 0.0, z3, z3, one, 8, one, one, None) == -2
    assert L.pnr_marching_cubes_emit(one, 4, 4, 4, 16, 4, 1, 0.0, z3, z3, one, 1 << 20, None, one, None) == -1
