"""Golden marching-cubes meshes from skimage, the library Mesher.get_mesh calls
(src/utils/Mesher.py:441-448: skimage.measure.marching_cubes with its defaults = Lewiner).

Run under an interpreter that has scikit-image (0.18.3 when the fixture was made; numpy only besides):

    PYTHONDONTWRITEBYTECODE=1 python3.9 tests/golden/make_golden_mc.py

  mc.npz, for <name> in sphere (level 0), blobs (two tanh blobs, level 10), plane (a tilted plane
  that reaches the volume border, level 0), noise (Gaussian noise, level 0.1):
    <name>/vol     (14,11,9) f32   the volume as skimage receives it (x, y, z axes)
    <name>/level   f64
    <name>/verts   (V,3) f32       skimage Lewiner vertices (spacing applied, no origin)
    <name>/faces   (F,3) i32       skimage Lewiner faces
    noise/verts_lorensen, noise/faces_lorensen    method='lorensen' on the noise volume
    spacing (3,) f64, sphere_centre (3,) f64, sphere_radius f64   (world units)

Asserted here: on the three smooth volumes the two methods give the same vertex and face sets; every
stored vertex lies within 1e-6 of a cell of the float64 linear-interpolation crossing
(tests/mesh_ref.py crossing_set) -- but for Lewiner on the noise volume, whose ambiguous cases add
cell-centre vertices (which is why the noise volume is pinned to Lorensen); no sample equals its level.
"""
import os
import sys

import numpy as np
from skimage import measure

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import mesh_ref  # noqa: E402

SHAPE = (14, 11, 9)
SPACING = np.array([0.1, 0.2, 0.3])
CENTRE = np.array([0.6537, 1.0219, 1.2113])
RADIUS = 0.5


def volumes():
    g = np.stack(np.meshgrid(*[np.arange(n) * s for n, s in zip(SHAPE, SPACING)], indexing='ij'), -1)
    rng = np.random.RandomState(5)
    d1 = np.linalg.norm(g - np.array([0.4131, 0.6217, 0.8093]), axis=-1)
    d2 = np.linalg.norm(g - np.array([0.9057, 1.4311, 1.6129]), axis=-1)
    n = np.array([0.31, 0.52, 0.8])
    return {
        'sphere': ((np.linalg.norm(g - CENTRE, axis=-1) - RADIUS).astype(np.float32), 0.0),
        'blobs': ((10 * (1 + np.tanh(5 * (0.33 - d1))) + 10 * (1 + np.tanh(5 * (0.36 - d2)))).astype(np.float32), 10.0),
        'plane': (((g * n).sum(-1) - 1.4107).astype(np.float32), 0.0),
        'noise': (rng.randn(*SHAPE).astype(np.float32), 0.1),
    }


def face_set(verts, faces):
    """Faces as rotation-canonical triples of vertex coordinates (independent of vertex numbering)."""
    out = set()
    for f in faces:
        t = [tuple(verts[i].tolist()) for i in f]
        k = t.index(min(t))
        out.add(tuple(t[k:] + t[:k]))
    return out


def main():
    data = {'spacing': SPACING, 'sphere_centre': CENTRE, 'sphere_radius': np.float64(RADIUS)}
    worst = 0.0
    for name, (vol, level) in volumes().items():
        assert not (vol == np.float32(level)).any(), name
        out = {}
        for method in ('lewiner', 'lorensen'):
            verts, faces, _, _ = measure.marching_cubes(vol, level=level, spacing=tuple(SPACING), method=method)
            out[method] = (verts.astype(np.float32), faces.astype(np.int32))
            if name == 'noise' and method == 'lewiner':
                continue   # Lewiner adds a cell-centre vertex in some ambiguous cases: not a crossing set
            cells = mesh_ref.sort_rows(verts.astype(np.float64) / SPACING)
            cross = mesh_ref.crossing_set(vol, level)
            assert cells.shape == cross.shape, (name, method, cells.shape, cross.shape)
            perm = mesh_ref.match_rows(cells, cross, 1e-6)
            assert perm is not None, (name, method)
            worst = max(worst, float(np.abs(cells - cross[perm]).max()))
        (vl, fl), (vo, fo) = out['lewiner'], out['lorensen']
        if name != 'noise':
            assert np.array_equal(mesh_ref.sort_rows(vl), mesh_ref.sort_rows(vo)), name
            assert face_set(vl, fl) == face_set(vo, fo), name
        else:
            data['noise/verts_lorensen'], data['noise/faces_lorensen'] = vo, fo
        data[f'{name}/vol'], data[f'{name}/level'] = vol, np.float64(level)
        data[f'{name}/verts'], data[f'{name}/faces'] = vl, fl
        print(name, 'verts', vl.shape[0], 'faces', fl.shape[0], 'lorensen faces', fo.shape[0],
              'boundary edges (lorensen)', len(mesh_ref.boundary_edges(fo)))
    print('worst |skimage vertex - float64 crossing| (cells):', worst)
    np.savez_compressed(os.path.join(OUT, 'mc.npz'), **data)


if __name__ == '__main__':
    main()
