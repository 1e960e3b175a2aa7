"""pnr.TSDFVolume.extract_triangle_mesh (csrc/tsdf.hip k_tsdf_mesh) against the numpy restatement of its rules
(tests/tsdf_mesh_ref.py) on the device's own fused blocks, bit for bit: positions and colours are float32 sums,
products and correctly rounded divisions in a stated order, which numpy reproduces.  Shapes as in test_gpu_tsdf.py.
The box puts block corners at (0, 0, 0.08) and (+-0.125, 0, 0.08): the plane passes through the first, the sphere
within 2 mm of the others, so faces come from cells that reach into the next block along one, two and three axes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_ref
import tsdf_mesh_ref
from conftest import REPO
from test_gpu_tsdf import CAM, DIMS, H, TRUNC, VL, W, look_at, plane_depth, sphere_depth, stack

TABLE = mesh_ref.load_case_table(os.path.join(REPO, 'pointnerf-slam_amd', 'csrc', 'mc_table.h'))
LO = np.array([-0.21, -0.21, -0.13])
BOUND = np.stack([LO, LO + np.array([0.4, 0.4, 0.28])], 1)
# name -> (surface, max_blocks, colour); the sphere's three frames fill 48 blocks
CASES = {'plane': ('plane', 64, True), 'sphere': ('sphere', 64, True), 'dropped': ('sphere', 40, True),
         'nocolor': ('sphere', 64, False)}


def case_frames(surface):
    if surface == 'plane':     # one frame: voxels of live blocks outside its frustum keep weight 0
        c2w = [look_at([0.03, -0.05, 0.4], [0.0, 0.0, 0.08], 0.1)]
        depth = [plane_depth(c2w[0], [0.0, 0.0, 0.08], [0.25, -0.2, 1.0])]
    else:
        c2w = [look_at([0.05, -0.5, 0.1], [0, 0, 0], 0.2), look_at([0.5, 0.1, 0.3], [0, 0, 0], -0.4),
               look_at([-0.3, 0.3, 0.35], [0, 0, 0], 0.7)]
        depth = [sphere_depth(m, [0.0, 0.0, 0.0], 0.15) for m in c2w]
    col = np.random.RandomState(len(surface)).uniform(0, 1, (len(c2w), H, W, 3)).astype(np.float32)
    return [(depth[k], col[k], c2w[k]) for k in range(len(c2w))]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_mesh_is_the_rule_on_the_device_volume(name):
    import pnr
    surface, max_blocks, color = CASES[name]
    frames = case_frames(surface)
    vol = pnr.TSDFVolume(BOUND, VL, TRUNC, H, W, max_blocks=max_blocks, device='cuda:0', color=color, **CAM)
    assert tuple(vol.dims) == DIMS and all(x.shape == (0, 3) for x in vol.extract_triangle_mesh())   # freshly reset
    depth, col, c2w = stack(frames)
    vol.integrate(depth, col if color else None, c2w)
    assert (vol.dropped_blocks > 0) == (name == 'dropped')
    b = vol.blocks()
    want = tsdf_mesh_ref.mesh(b['tsdf'].cpu().numpy(), b['weight'].cpu().numpy(),
                              b['rgb'].cpu().numpy() if color else None, b['index'].cpu().numpy().astype(np.int64),
                              vol.origin, VL, DIMS, TABLE)
    # the inputs: enough faces, from cells that reach over a block face, a block edge and a block corner
    print(name, 'blocks', vol.n_blocks, 'V', len(want['verts']), 'F', len(want['faces']), 'faces by block axes',
          np.bincount(want['block_axes'], minlength=4), 'strict crossings', int(want['crossing'].sum()))
    assert len(want['faces']) >= 300 and (np.bincount(want['block_axes'], minlength=4) > 0).all()
    verts, faces, rgb = vol.extract_triangle_mesh()
    assert verts.dtype == rgb.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda
    for got, key in ((faces, 'faces'), (verts, 'verts'), (rgb, 'rgb')):
        assert torch.equal(got.cpu(), torch.from_numpy(want[key])), key
    assert bool((rgb != 0).any()) == color
    f, v = faces.cpu().numpy(), verts.cpu().numpy()
    assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)   # in range; every vertex referenced
    assert mesh_ref.edge_report(f)[2] == 0
    points = {row.tobytes() for row in vol.extract_points()[0].cpu().numpy()}
    assert all(row.tobytes() in points for row in v[want['crossing']])
    if name == 'plane':        # the faces look at the camera that saw them: towards positive tsdf
        v64 = v.astype(np.float64)
        normal = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
        assert ((normal * (frames[0][2][:3, 3].astype(np.float64) - v64[f[:, 0]])).sum(1) > 0).all()
    again = vol.extract_triangle_mesh()
    assert all(torch.equal(x, y) for x, y in zip((verts, faces, rgb), again))


def test_mesh_argument_errors_touch_no_device():
    from pnr import _lib
    L = _lib.load()
    v = _lib.Tsdf()
    ref, ptr = ctypes.byref(v), ctypes.c_void_p(4096)      # never dereferenced: every call returns before a launch
    assert L.pnr_tsdf_mesh_workspace_bytes(None) == 0 and L.pnr_tsdf_mesh_workspace_bytes(ref) == 0
    assert L.pnr_tsdf_mesh_count(None, ptr, 1 << 30, ptr, ptr, None) == -1
    v.voxel_length, v.sdf_trunc, v.depth_trunc, v.max_blocks, v.H, v.W = VL, TRUNC, 1000.0, 64, H, W
    v.dims[:], v.fx, v.fy, v.cx, v.cy = DIMS, CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy']
    need = L.pnr_tsdf_mesh_workspace_bytes(ref)
    assert need >= 64 * (256 * 8 + 16)
    assert L.pnr_tsdf_mesh_count(ref, ptr, need, ptr, ptr, None) == -1         # the volume has no buffers
    v.directory = v.tsdf = v.weight = v.block_index = 4096
    assert L.pnr_tsdf_mesh_count(ref, ptr, need - 1, ptr, ptr, None) == -2
    assert L.pnr_tsdf_mesh_count(ref, ptr, need, None, ptr, None) == -1
    assert L.pnr_tsdf_mesh_emit(ref, ptr, need - 1, ptr, None, ptr, None) == -2
    assert L.pnr_tsdf_mesh_emit(ref, ptr, need, ptr, ptr, ptr, None) == -1     # colour asked of a volume without
    v.max_blocks = 1 << 17                                                     # 2^17 4096 5 faces pass 2^31
    assert L.pnr_tsdf_mesh_workspace_bytes(ref) == 0 and L.pnr_tsdf_mesh_count(ref, ptr, need, ptr, ptr, None) == -1
