"""Golden seen / forecast / unseen masks, made by running the REFERENCE Mesher.point_masks
(src/utils/Mesher.py:53-212) on the CPU (run in the build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_masks.py [/root/reference]

The reference module imports open3d, skimage, trimesh and its dataset readers at the top; point_masks
uses none of them, so empty stub modules stand in, and the object is made with object.__new__ (its
__init__ builds a dataset reader).

  masks.npz
    points (4096,3) f32      uniform in the cube [-3,3]^3
    c2w (3,4,4) f32          yawed keyframe poses (also the estimate_c2w_list of the poses-only mode, idx = 2)
    depth (3,48,64) f32      keyframe depth in 1.5-2.5 with ~10% zeros
    intr (6,) f64            H, W, fx, fy, cx, cy
    batch i64                points_batch_size = 1500: the depth-test mode's max_depth is per chunk
    <mode>/seen, <mode>/forecast, <mode>/unseen (4096,) bool   for mode in poses (get_mask_use_all_frames),
                             maxdepth (depth_test=False), depthtest (depth_test=True)

Asserted here: the float64 restatement tests/mesh_ref.py equals the reference on every non-edge point,
and at most 1% of the points are edge points, in every mode.
"""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import mesh_ref  # noqa: E402

N, K, H, W = 4096, 3, 48, 64
FX, FY, CX, CY = 40.0, 40.0, 31.5, 23.5
BATCH = 1500


def poses():
    out = []
    for k, (yaw, t) in enumerate(((0.3, (0.2, -0.1, 0.4)), (2.1, (-0.5, 0.3, -0.2)), (-1.2, (0.1, 0.2, -0.6)))):
        c, s = np.cos(yaw), np.sin(yaw)
        m = np.eye(4)
        m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array(
            [[1, 0, 0], [0, np.cos(0.1 * k), -np.sin(0.1 * k)], [0, np.sin(0.1 * k), np.cos(0.1 * k)]])
        m[:3, 3] = t
        out.append(m)
    return np.stack(out).astype(np.float32)


def main():
    torch.set_num_threads(1)
    for name in ('open3d', 'skimage', 'trimesh', 'src.utils.datasets'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['src.utils.datasets'].get_dataset = None
    sys.path.insert(0, REF)
    from src.utils.Mesher import Mesher                      # noqa: E402

    rng = np.random.RandomState(3)
    points = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    c2w = poses()
    depth = rng.uniform(1.5, 2.5, (K, H, W)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.1] = 0.0
    keyframes = [{'est_c2w': torch.from_numpy(c2w[k]), 'depth': torch.from_numpy(depth[k])} for k in range(K)]
    w2c = np.stack([np.linalg.inv(c2w[k]) for k in range(K)])

    data = {'points': points, 'c2w': c2w, 'depth': depth, 'intr': np.array([H, W, FX, FY, CX, CY], np.float64),
            'batch': np.int64(BATCH)}
    for mode in mesh_ref.MODES:
        m = object.__new__(Mesher)
        m.H, m.W, m.fx, m.fy, m.cx, m.cy = H, W, FX, FY, CX, CY
        m.points_batch_size = BATCH
        m.depth_test = mode == 'depthtest'
        seen, fore, unseen = m.point_masks(torch.from_numpy(points), keyframes, torch.from_numpy(c2w), K - 1, 'cpu',
                                           get_mask_use_all_frames=mode == 'poses')
        rs, rf, ru, margin = mesh_ref.point_masks_ref(points, w2c, H, W, FX, FY, CX, CY, mode, depth, BATCH)
        edge = margin < mesh_ref.EDGE_MARGIN
        assert edge.mean() <= 0.01, (mode, edge.mean())
        for a, b in ((seen, rs), (fore, rf), (unseen, ru)):
            assert np.array_equal(a[~edge], b[~edge]), mode
        print(mode, 'seen', int(seen.sum()), 'forecast', int(fore.sum()), 'unseen', int(unseen.sum()),
              'edge points', int(edge.sum()), 'disagreeing edge points',
              int(((seen != rs) | (fore != rf)).sum()))
        data[f'{mode}/seen'], data[f'{mode}/forecast'], data[f'{mode}/unseen'] = seen, fore, unseen
    np.savez_compressed(os.path.join(OUT, 'masks.npz'), **data)


if __name__ == '__main__':
    main()
