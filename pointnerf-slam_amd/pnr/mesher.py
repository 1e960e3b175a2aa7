"""The Mesher's decoder consumers on the HIP path.

Under configs/pointNeRF_slam.yaml (`meshing.color_mesh_extraction_method: render_ray_along_normal`,
:37) Mesher.get_mesh (src/utils/Mesher.py:349-570) calls the decoder twice:
  * the dense grid query: get_grid_uniform (:321-347) + Mesher.eval_points (:281-319) over
    resolution^3 points in points_batch_size chunks, occupancy = raw[:, -1] (:427-430);
  * the vertex colouring (:526-553): one ray per mesh vertex, started `length`=0.1 behind the
    vertex along its normal (rays_o = v - 0.1 n, rays_d = n), rendered by
    Renderer.render_batch_ray with gt_depth = 0.1 in ray_batch_size chunks; the colour is clipped
    to [0,1] and stored as uint8 (:555-556).  `direct_point_query` (:513-524, the nice-slam
    setting) is eval_points(vertices)[..., :3].
The geometry between the two also runs on the device (csrc/mesh.hip), because the reference's
host libraries for it (skimage, trimesh, open3d) are not importable on this stack:
  * `point_masks`: the seen / forecast / unseen split of Mesher.point_masks (:53-212), one kernel
    call per points_batch_size chunk (the depth-test mode's max_depth is a per-chunk maximum);
  * `marching_cubes`: an indexed float64 / int32 mesh with shared vertices in a deterministic order,
    skimage's default winding, a generated crack-free case table (tools/gen_mc_table.py);
  * `clean_mesh`: the all-unseen face cull, connected components, the small-component filter or
    the largest component, and the compaction (:469-510), in torch ops on the device;
  * `get_bound_from_frames` (:214-279): the convex hull of what the keyframes saw as a `FrameBound`
    -- the support function of the back-projected depth pixels, the positions of chosen points and the
    containment test on the device (csrc/bound.hip), the quickhull between them on the host
    (pnr/bound.py) -- applied by get_mesh with `mesh_bound_mask='frames'`;
  * `write_ply`, and `Mesher.get_mesh` that strings everything together.
Stated deviations.  Components rule: components are taken over shared VERTICES, trimesh.split takes
them over shared edges: the two differ only where components touch at a single vertex.  Depth pixels,
not a TSDF surface: the reference's hull is taken over the vertices of an open3d TSDF surface (voxel
4 scale / 512) fused from the depth maps, ours over the valid depth pixels themselves and the camera
centres; the two hulls differ by the order of that voxel, and parity with open3d is unpinned, as for
`vertex_normals`.  A hull to a tolerance: refinement stops when no point lies more than eps / 2
(default eps = 4 scale / 512) outside a facet, and each facet's plane is then moved out to the measured
support of the points plus a rounding guard, so hull(V) <= hull(P) <= H for the result H with vertices
V: every input point is inside by construction.  get_mesh's default `mesh_bound_mask=None` applies no
hull mask (eval_points already returns 100 outside the scene bound).
The vertex normals the reference takes from open3d (`compute_vertex_normals`, open3d is not in
this image) are restated by `vertex_normals` on the device: area-weighted sums of the unnormalised triangle normals, normalised, with (0,0,1) for a
vertex whose sum vanishes (open3d TriangleMesh::ComputeVertexNormals + MeshBase::NormalizeNormals).
That restatement is "parity unpinned" (no open3d output is available to pin it); the colouring
itself is pinned through render_batch_ray against the oracle (tests/test_gpu_parity.py).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import bound as _bound


def get_grid_uniform(bound, resolution, padding=0.05):
    """src/utils/Mesher.py:321-347: float32 (R^3, 3) grid points over `bound` (3,2) padded by
    `padding` (np.linspace per axis, np.meshgrid 'xy' order, ravel) and the per-axis coordinates."""
    b = np.asarray(bound.cpu() if isinstance(bound, torch.Tensor) else bound, dtype=np.float64).reshape(3, 2)
    x, y, z = (np.linspace(b[a][0] - padding, b[a][1] + padding, resolution) for a in range(3))
    xx, yy, zz = np.meshgrid(x, y, z)
    grid_points = torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float)
    return {'grid_points': grid_points, 'xyz': [x, y, z]}


def eval_grid(renderer, decoders, c, points, device, stage='color'):
    """The Mesher's grid query (src/utils/Mesher.py:427-430): raw (P,4) float32 of `points` in
    renderer.points_batch_size chunks through the HIP eval_points (the occupancy is raw[:, -1])."""
    _lib.require_cuda(points)
    with torch.no_grad():
        out = [renderer.eval_points(p, decoders, c, stage, device)
               for p in torch.split(points, renderer.points_batch_size)]
    return torch.cat(out, 0) if out else torch.empty((0, 4), device=points.device)


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """open3d compute_vertex_normals restated on the device (float64): per triangle the
    unnormalised cross((v1 - v0), (v2 - v0)), summed into its three vertices, then normalised;
    a zero sum gives (0, 0, 1).  vertices (V,3), faces (F,3) int -> (V,3) float64."""
    v = vertices.double()
    f = faces.long()
    tn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    n = torch.zeros_like(v)
    for a in range(3):
        n.index_add_(0, f[:, a], tn)
    norm = n.norm(dim=1, keepdim=True)
    z = torch.zeros_like(n)
    z[:, 2] = 1.0
    return torch.where(norm > 0, n / torch.where(norm > 0, norm, torch.ones_like(norm)), z)


def color_along_normal(renderer, decoders, c, vertices, normals, device, length=0.1, stage='color'):
    """src/utils/Mesher.py:526-553: vertex colour (V,3) float32 from one ray per vertex,
    rays_o = v - length * n, rays_d = n, gt_depth = length, rendered in ray_batch_size chunks."""
    v = vertices.to(device).double()
    n = normals.to(device).double()
    _lib.require_cuda(v)
    rays_d = n
    rays_o = v + (-1.0) * length * n
    gt_depth = torch.full((v.shape[0],), length, device=v.device)
    out = []
    with torch.no_grad():
        bs = renderer.ray_batch_size
        for i in range(0, rays_d.shape[0], bs):
            _, _, col = renderer.render_batch_ray(c, decoders, rays_d[i:i + bs], rays_o[i:i + bs], device,
                                                  stage=stage, gt_depth=gt_depth[i:i + bs])
            out.append(col)
    return torch.cat(out, 0) if out else torch.empty((0, 3), device=v.device)


def direct_point_query(renderer, decoders, c, vertices, device, stage='color'):
    """src/utils/Mesher.py:513-524 (`direct_point_query`): eval_points(vertices)[..., :3]."""
    return eval_grid(renderer, decoders, c, vertices.to(device).float(), device, stage)[..., :3]


def vertex_colors_u8(colors: torch.Tensor) -> np.ndarray:
    """src/utils/Mesher.py:555-556: clip to [0,1], x255, uint8 (truncation, as numpy astype)."""
    return (np.clip(colors.detach().cpu().numpy(), 0, 1) * 255).astype(np.uint8)


def mesh_colors(renderer, decoders, c, vertices, faces, device, method='render_ray_along_normal'):
    """The colour branch of Mesher.get_mesh (:512-556) for a mesh from the caller's marching cubes:
    uint8 (V,3) vertex colours by the configured `color_mesh_extraction_method`."""
    v = torch.as_tensor(vertices)
    if method == 'render_ray_along_normal':
        n = vertex_normals(v.to(device), torch.as_tensor(faces).to(device))
        col = color_along_normal(renderer, decoders, c, v, n, device)
    elif method == 'direct_point_query':
        col = direct_point_query(renderer, decoders, c, v, device)
    else:
        raise ValueError(f'pnr.mesher: unknown color_mesh_extraction_method {method!r}')
    return vertex_colors_u8(col)


# ---- the geometry between the grid query and the colouring (csrc/mesh.hip) ------------------------

# configs/pointNeRF_slam.yaml:29-38, used for the cfg['meshing'] keys a config leaves out
MESHING_DEFAULTS = {
    'level_set': 10, 'resolution': 256, 'eval_rec': False, 'clean_mesh': True, 'depth_test': False,
    'mesh_coarse_level': False, 'clean_mesh_bound_scale': 1.02, 'get_largest_components': False,
    'color_mesh_extraction_method': 'render_ray_along_normal', 'remove_small_geometry_threshold': 0.2,
}


def _w2c(c2w_list, device):
    """(K,4,4) float32 on the device: np.linalg.inv of each float32 c2w on the host, as
    src/utils/Mesher.py:90-92 / :128-130 compute it."""
    mats = [np.linalg.inv(c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w))
            for c2w in c2w_list]
    if not mats:
        return torch.empty((0, 4, 4), dtype=torch.float32, device=device)
    return torch.from_numpy(np.stack(mats)).to(device).float().contiguous()


def point_masks(points, keyframe_dict, estimate_c2w_list, idx, H, W, fx, fy, cx, cy, device, depth_test=False,
                get_mask_use_all_frames=False, points_batch_size=500000):
    """src/utils/Mesher.py:53-212 on the device: (seen, forecast, unseen) bool tensors over `points`
    (N,3).  get_mask_use_all_frames uses the poses estimate_c2w_list[0..idx] and no depth; otherwise
    the keyframes' 'est_c2w' and 'depth', with max_depth = 1.1 max(depth_k) (depth_test=False) or the
    bilinear depth sample and its maximum over the points of each points_batch_size chunk
    (depth_test=True).  One kernel call per chunk, as the reference loops."""
    lib = _lib.load()
    device = torch.device(device)
    if not isinstance(points, torch.Tensor):
        points = torch.from_numpy(np.asarray(points))
    pts = points.detach().to(device).float().contiguous()
    _lib.require_cuda(pts)
    depth = max_depth = None
    if get_mask_use_all_frames:
        mode = _lib.MASK_POSES
        w2c = _w2c([estimate_c2w_list[i] for i in range(0, idx + 1)], device)
    else:
        w2c = _w2c([kf['est_c2w'] for kf in keyframe_dict], device)
        if depth_test:
            mode = _lib.MASK_DEPTH_TEST
            if len(keyframe_dict):
                depth = torch.stack([kf['depth'].to(device).reshape(H, W) for kf in keyframe_dict]).float().contiguous()
        else:
            mode = _lib.MASK_MAX_DEPTH
            if len(keyframe_dict):
                max_depth = torch.stack([(torch.max(kf['depth']) * 1.1).to(device) for kf in keyframe_dict])
                max_depth = max_depth.float().contiguous()
    K, N = w2c.shape[0], pts.shape[0]
    seen = torch.zeros(N, dtype=torch.uint8, device=device)
    fore = torch.zeros(N, dtype=torch.uint8, device=device)
    if K > 0:
        for s in range(0, N, points_batch_size):
            n = min(points_batch_size, N - s)
            nbytes = lib.pnr_point_masks_workspace_bytes(n, K, mode)
            ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=device)
            _lib.check(lib.pnr_point_masks(_lib.ptr(pts[s:s + n]), n, _lib.ptr(w2c), K, H, W, fx, fy, cx, cy, mode,
                                           _lib.ptr(depth), _lib.ptr(max_depth), _lib.ptr(seen[s:s + n]),
                                           _lib.ptr(fore[s:s + n]), _lib.ptr(ws), nbytes, _lib.stream_of(device)),
                       'point_masks')
    seen, fore = seen.bool(), fore.bool()
    return seen, fore, ~(seen | fore)


# ---- the mesh bound from the keyframes (csrc/bound.hip, pnr/bound.py) -----------------------------

DEPTH_TRUNC = 1000.0   # src/utils/Mesher.py:261 (open3d's depth_trunc)


class FramePoints(object):
    """The point set P of the mesh bound on the device (include/pnr.h `pnr_bound_frames`): the valid
    depth pixels (finite, 0 < d <= depth_trunc) of the `stride` lattice of every keyframe, back-projected
    as the map growth does (index k H W + v W + u), then `extra` (n,3) points (index K H W + e).
    depth (K,H,W) and c2w (K,4,4) are float32 device tensors."""

    def __init__(self, depth, c2w, fx, fy, cx, cy, stride=1, depth_trunc=DEPTH_TRUNC, extra=None):
        self.lib = _lib.load()
        self.depth = depth.detach().float().contiguous()
        self.c2w = c2w.detach().to(self.depth.device).float().contiguous()
        _lib.require_cuda(self.depth, self.c2w)
        if self.depth.dim() != 3 or self.c2w.shape != (self.depth.shape[0], 4, 4):
            raise ValueError('pnr.mesher: depth (K,H,W) and c2w (K,4,4) expected')
        self.device = self.depth.device
        self.extra = None
        if extra is not None and len(extra):
            self.extra = torch.as_tensor(extra).detach().to(self.device).float().reshape(-1, 3).contiguous()
        K, H, W = self.depth.shape
        f = _lib.BoundFrames()
        f.depth, f.c2w = self.depth.data_ptr() if K else None, self.c2w.data_ptr() if K else None
        f.K, f.H, f.W, f.stride = K, H, W, int(stride)
        f.fx, f.fy, f.cx, f.cy, f.depth_trunc = float(fx), float(fy), float(cx), float(cy), float(depth_trunc)
        f.extra_xyz = self.extra.data_ptr() if self.extra is not None else None
        f.n_extra = self.extra.shape[0] if self.extra is not None else 0
        self.frames = f
        self.n_index = K * H * W + f.n_extra
        self.max_dirs = int(self.lib.pnr_bound_support_max_dirs())
        self.support_launches = 0

    def support(self, dirs):
        """pnr_bound_support: (h float32 (D,), arg int64 (D,)) device tensors for `dirs` (D,3); h = -inf
        and arg = -1 when no point is valid.  More directions than the library's cap are split."""
        d = torch.as_tensor(dirs).detach().to(self.device).float().reshape(-1, 3).contiguous()
        D = d.shape[0]
        h = torch.empty(D, dtype=torch.float32, device=self.device)
        arg = torch.empty(D, dtype=torch.int64, device=self.device)
        st = _lib.stream_of(self.device)
        for s in range(0, D, self.max_dirs):
            n = min(self.max_dirs, D - s)
            nbytes = self.lib.pnr_bound_support_workspace_bytes(ctypes.byref(self.frames), n)
            if nbytes == 0:
                raise RuntimeError('pnr: bound_support failed (bad argument)')
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.pnr_bound_support(ctypes.byref(self.frames), _lib.ptr(d[s:s + n]), n,
                                                  _lib.ptr(h[s:s + n]), _lib.ptr(arg[s:s + n]), _lib.ptr(ws), nbytes,
                                                  st), 'bound_support')
            self.support_launches += 1
        return h, arg

    def points(self, idx):
        """pnr_bound_points: float32 (n,3) positions of the indices `idx`; NaN rows for indices that
        name no valid point."""
        i = torch.as_tensor(idx).detach().to(self.device).long().reshape(-1).contiguous()
        xyz = torch.empty((i.shape[0], 3), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pnr_bound_points(ctypes.byref(self.frames), _lib.ptr(i), i.shape[0], _lib.ptr(xyz),
                                             _lib.stream_of(self.device)), 'bound_points')
        return xyz

    # the two callables of pnr.bound.build_hull: one small host read each
    def support_np(self, dirs):
        h, arg = self.support(torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32)))
        return h.cpu().numpy(), arg.cpu().numpy()

    def points_np(self, idx):
        return self.points(torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))).cpu().numpy()


def bound_contains(points, planes, chunk=1 << 22):
    """pnr_bound_contains_*: bool (P,) device tensor, True where (x a + y b) + z c <= d holds in unfused
    float64 for every row (a, b, c, d) of the device tensor `planes` (F,4) float64.  `points` (P,3):
    a float32 or float64 tensor (moved to the planes' device) or numpy array; any other dtype is taken
    as float64.  Runs in chunks of `chunk` points."""
    lib = _lib.load()
    _lib.require_cuda(planes)
    pl = planes.detach().double().reshape(-1, 4).contiguous()
    p = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.asarray(points))
    p = p.detach().to(pl.device)
    if p.dtype != torch.float32:
        p = p.double()
    p = p.reshape(-1, 3).contiguous()
    fn = lib.pnr_bound_contains_f32 if p.dtype == torch.float32 else lib.pnr_bound_contains_f64
    out = torch.empty(p.shape[0], dtype=torch.uint8, device=pl.device)
    st = _lib.stream_of(pl.device)
    for s in range(0, p.shape[0], chunk):
        n = min(chunk, p.shape[0] - s)
        _lib.check(fn(_lib.ptr(p[s:s + n]), n, _lib.ptr(pl) if pl.shape[0] else None, pl.shape[0],
                      _lib.ptr(out[s:s + n]), st), 'bound_contains')
    return out.bool()


class FrameBound(object):
    """The mesh bound of src/utils/Mesher.py:214-279: the convex hull (to the tolerance `eps`, see
    pnr/bound.py) of the keyframes' back-projected depth pixels and camera centres, scaled by
    `bound_scale` about its centre (:273).

    planes           (F,4) float64 on the device: a point is inside when n.p <= off for every row
    planes_unscaled  the same before the scaling (host, float64)
    vertices, faces  the hull's triangles (host; vertices (V,3) float64 unscaled, rows of the point set)
    vertex_index     (V,) their indices in the point set
    center           (3,) the mean of the vertices (open3d's get_center() of the hull mesh)
    stats            rounds, directions, support_calls, facets, vertices of the build
    `contains(points)` is the reference's `mesh_bound.contains`; the object is callable, so it is a valid
    `mesh_bound_mask` of Mesher.get_mesh."""

    def __init__(self, hull, bound_scale, eps, device):
        self.device = torch.device(device)
        self.eps = float(eps)
        self.bound_scale = float(bound_scale)
        self.planes_unscaled = hull.planes
        self.planes_host = _bound.scale_planes(hull.planes, hull.center, bound_scale)
        self.planes = torch.from_numpy(self.planes_host).to(self.device)
        self.vertices, self.faces, self.vertex_index = hull.vertices, hull.faces, hull.vertex_index
        self.center = hull.center
        self.capped = hull.capped
        self.stats = dict(hull.stats)

    def contains(self, points, chunk=1 << 22):
        return bound_contains(points, self.planes, chunk)

    __call__ = contains


def get_bound_from_frames(keyframe_dict, H, W, fx, fy, cx, cy, scale=1.0, bound_scale=1.02, device='cuda:0',
                          stride=1, eps=None, max_facets=16384):
    """src/utils/Mesher.py:214-279 on the device: the FrameBound of the keyframes' 'depth' (H,W) and
    'est_c2w' (4,4).  `eps` defaults to the reference's TSDF voxel 4 scale / 512; `stride` >= 1 thins the
    pixels to a lattice.  One small host read per refinement round, as marching cubes reads its counts."""
    if len(keyframe_dict) == 0:
        raise ValueError('pnr.mesher: get_bound_from_frames needs at least one keyframe')
    device = torch.device(device)
    depth = torch.stack([kf['depth'].to(device).reshape(H, W) for kf in keyframe_dict]).float()
    c2w = torch.stack([torch.as_tensor(kf['est_c2w']).detach().to(device).float().reshape(4, 4)
                       for kf in keyframe_dict])
    pts = FramePoints(depth, c2w, fx, fy, cx, cy, stride=stride, extra=c2w[:, :3, 3])
    lattice = depth[:, ::stride, ::stride]
    if not bool((torch.isfinite(lattice) & (lattice > 0) & (lattice <= DEPTH_TRUNC)).any()):
        raise ValueError('pnr.mesher: get_bound_from_frames found no valid depth pixel')
    eps =4.0 * float(scale) / 512.0 if eps is None else float(eps)
    hull = _bound.build_hull(pts.support_np, pts.points_np, eps, max_facets)
    fb = FrameBound(hull, bound_scale, eps, device)
    fb.stats['support_launches'] = pts.support_launches
    return fb


def marching_cubes_volume(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Marching cubes over a float32 device tensor vol[ix, iy, iz] of any strides (no copy is made):
    vertices (V,3) float64 = origin + (i + t) spacing with t = (level - a) / (b - a) in float64, faces
    (F,3) int32, vertices shared, skimage's default winding, a fixed order (two runs are bitwise equal).
    A volume without a crossing gives an empty mesh."""
    lib = _lib.load()
    _lib.require_cuda(vol)
    if vol.dim() != 3 or vol.dtype != torch.float32:
        raise ValueError('pnr.mesher: marching cubes takes a 3-d float32 volume')
    nx, ny, nz = vol.shape
    sx, sy, sz = vol.stride()
    nbytes = lib.pnr_marching_cubes_workspace_bytes(nx, ny, nz)
    if nbytes == 0:
        raise ValueError(f'pnr.mesher: unsupported marching-cubes volume {tuple(vol.shape)} '
                         f'(1 <= samples <= {lib.pnr_marching_cubes_max_points()})')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    counts = torch.zeros(2, dtype=torch.int64, device=vol.device)
    st = _lib.stream_of(vol.device)
    _lib.check(lib.pnr_marching_cubes_count(_lib.ptr(vol), nx, ny, nz, sx, sy, sz, float(level), _lib.ptr(ws), nbytes,
                                            counts.data_ptr(), counts.data_ptr() + 8, st), 'marching_cubes_count')
    n_v, n_f = (int(x) for x in counts.tolist())
    vertices = torch.empty((n_v, 3), dtype=torch.float64, device=vol.device)
    # (a volume one sample thick has crossings but no cell: the C call still wants a faces pointer)
    fbuf = torch.empty((max(n_f, 1), 3), dtype=torch.int32, device=vol.device)
    faces = fbuf[:n_f]
    if n_v > 0:
        o = (ctypes.c_double * 3)(*[float(x) for x in origin])
        sp = (ctypes.c_double * 3)(*[float(x) for x in spacing])
        _lib.check(lib.pnr_marching_cubes_emit(_lib.ptr(vol), nx, ny, nz, sx, sy, sz, float(level), o, sp, _lib.ptr(ws),
                                               nbytes, _lib.ptr(vertices), _lib.ptr(fbuf), st), 'marching_cubes_emit')
    return vertices, faces


def marching_cubes(z, grid_xyz, level):
    """The marching-cubes step of Mesher.get_mesh (:437-467): `z` is the flat float32 occupancy of
    get_grid_uniform's points, index (iy nx + ix) nz + iz, read through strides (the reference's
    reshape + transpose copy is not made); spacing = xyz[a][2] - xyz[a][1] and origin = xyz[a][0] as
    the reference takes them.  Returns (vertices float64 world coordinates, faces int32)."""
    x, y, zz = (np.asarray(a, dtype=np.float64) for a in grid_xyz)
    nx, ny, nz = len(x), len(y), len(zz)
    if z.numel() != nx * ny * nz:
        raise ValueError('pnr.mesher: the occupancy does not match the grid')
    vol = z.reshape(ny, nx, nz).permute(1, 0, 2)
    spacing = [(a[2] - a[1]) if len(a) > 2 else ((a[1] - a[0]) if len(a) > 1 else 1.0) for a in (x, y, zz)]
    return marching_cubes_volume(vol, level, spacing, (x[0], y[0], zz[0]))


def face_areas(vertices, faces):
    """Triangle areas (F,) float64."""
    f = faces.long()
    v = vertices.double()
    return 0.5 * torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1).norm(dim=1)


def vertex_components(n_vertices, faces):
    """Connected-component label (the smallest vertex index of the component) of every vertex, over
    shared vertices: min-label propagation across the faces with pointer jumping, on the device."""
    f = faces.long()
    label = torch.arange(n_vertices, device=faces.device)
    if f.shape[0] == 0:
        return label
    flat = f.reshape(-1)
    while True:
        fmin = label[f].min(dim=1).values
        new = label.scatter_reduce(0, flat, fmin.repeat_interleave(3), 'amin')
        new = new[new]
        if torch.equal(new, label):
            return label
        label = new


def compact_mesh(vertices, faces):
    """Drops the vertices no face names, keeping the order of both."""
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[faces.long().reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    return vertices[used], new_index[faces.long()].to(torch.int32)


def clean_mesh(vertices, faces, seen_mask=None, threshold=None, largest=False):
    """src/utils/Mesher.py:469-510 on the device: drop the faces whose three vertices are all unseen
    (`seen_mask` (V,) bool; None = keep all), split into connected components, keep the component of
    the largest area (`largest`) or those whose area exceeds `threshold` (already multiplied by
    scale^2; None = keep all), and compact.  Components are taken over shared vertices (trimesh.split:
    shared edges; the two differ only where components touch at a single vertex).  The order of the
    kept vertices and faces is preserved; the per-component areas are summed in a fixed order."""
    f = faces
    if seen_mask is not None:
        unseen = ~seen_mask.to(vertices.device).bool()
        f = f[~unseen[f.long()].all(dim=1)]
    if f.shape[0] > 0 and (largest or threshold is not None):
        label = vertex_components(vertices.shape[0], f)
        _, comp, counts = torch.unique(label[f[:, 0].long()], return_inverse=True, return_counts=True)
        order = torch.argsort(comp, stable=True)
        run = torch.cumsum(face_areas(vertices, f)[order], 0)
        ends = torch.cumsum(counts, 0) - 1
        area = run[ends]
        area = area - torch.cat([area.new_zeros(1), area[:-1]])
        keep = (comp == torch.argmax(area)) if largest else (area > threshold)[comp]
        f = f[keep]
    return compact_mesh(vertices, f)


_clean_mesh = clean_mesh   # Mesher.get_mesh has the reference's `clean_mesh` flag of the same name


def write_ply(path, vertices, faces, vertex_colors=None):
    """Binary little-endian PLY: float x y z (+ uchar red green blue), faces as
    `list uchar int vertex_indices`."""
    v = (vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices))
    f = (faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces))
    v = v.reshape(-1, 3).astype('<f4')
    f = f.reshape(-1, 3).astype('<i4')
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {v.shape[0]}',
              'property float x', 'property float y', 'property float z']
    if vertex_colors is not None:
        col = vertex_colors.detach().cpu().numpy() if isinstance(vertex_colors, torch.Tensor) else np.asarray(vertex_colors)
        col = col.reshape(-1, 3).astype(np.uint8)
        if col.shape[0] != v.shape[0]:
            raise ValueError('pnr.mesher: one colour per vertex')
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        header += ['property uchar red', 'property uchar green', 'property uchar blue']
    header += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    vert = np.empty(v.shape[0], dtype=fields)
    vert['x'], vert['y'], vert['z'] = v[:, 0], v[:, 1], v[:, 2]
    if vertex_colors is not None:
        vert['red'], vert['green'], vert['blue'] = col[:, 0], col[:, 1], col[:, 2]
    face = np.empty(f.shape[0], dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    face['n'] = 3
    face['idx'] = f
    with open(path, 'wb') as out:
        out.write(('\n'.join(header) + '\n').encode('ascii'))
        out.write(vert.tobytes())
        out.write(face.tobytes())


class Mesher(object):
    """src/utils/Mesher.py on the HIP path: the reference's constructor arguments and get_mesh.

    cfg['meshing'] keys that are absent take the values of configs/pointNeRF_slam.yaml:29-38
    (MESHING_DEFAULTS); cfg['mapping']['marching_cubes_bound'] falls back to cfg['mapping']['bound'].
    No dataset reader is built.  get_bound_from_frames returns a FrameBound (the hull of the depth
    pixels to a tolerance, not of open3d's TSDF surface); get_mesh applies it with
    `mesh_bound_mask='frames'`."""

    def __init__(self, cfg, args, slam, points_batch_size=500000, ray_batch_size=100000):
        self.points_batch_size = points_batch_size
        self.ray_batch_size = ray_batch_size
        self.renderer = slam.renderer
        self.coarse = cfg.get('coarse', False)
        self.scale = cfg['scale']
        self.occupancy = cfg.get('occupancy', False)
        m = {**MESHING_DEFAULTS, **cfg.get('meshing', {})}
        self.resolution = m['resolution']
        self.level_set = m['level_set']
        self.clean_mesh_bound_scale = m['clean_mesh_bound_scale']
        self.remove_small_geometry_threshold = m['remove_small_geometry_threshold']
        self.color_mesh_extraction_method = m['color_mesh_extraction_method']
        self.get_largest_components = m['get_largest_components']
        self.depth_test = m['depth_test']
        self.bound = slam.bound
        self.nice = False
        self.verbose = getattr(slam, 'verbose', False)
        mapping = cfg['mapping']
        self.marching_cubes_bound = torch.from_numpy(
            np.array(mapping.get('marching_cubes_bound', mapping['bound'])) * self.scale)
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy

    def point_masks(self, input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames=False):
        """Mesher.point_masks (:53-212); bool tensors on the device."""
        return point_masks(input_points, keyframe_dict, estimate_c2w_list, idx, self.H, self.W, self.fx, self.fy,
                           self.cx, self.cy, device, depth_test=self.depth_test,
                           get_mask_use_all_frames=get_mask_use_all_frames, points_batch_size=self.points_batch_size)

    def eval_points(self, p, decoders, c=None, stage='color', device='cuda:0'):
        """Mesher.eval_points (:281-319): raw (P,4) in points_batch_size chunks."""
        out = [self.renderer.eval_points(pi, decoders, c, stage, device) for pi in torch.split(p, self.points_batch_size)]
        return torch.cat(out, 0) if out else torch.empty((0, 4), device=p.device)

    def get_grid_uniform(self, resolution):
        return get_grid_uniform(self.marching_cubes_bound, resolution)

    def get_bound_from_frames(self, keyframe_dict, scale=1, device='cuda:0', **kw):
        """Mesher.get_bound_from_frames (:214-279): the FrameBound of the keyframes, scaled by
        clean_mesh_bound_scale about its centre.  `kw`: stride, eps, max_facets."""
        return get_bound_from_frames(keyframe_dict, self.H, self.W, self.fx, self.fy, self.cx, self.cy, scale=scale,
                                     bound_scale=self.clean_mesh_bound_scale, device=device, **kw)

    def get_mesh(self, mesh_out_file, c, decoders, keyframe_dict, estimate_c2w_list, idx, device='cuda:0',
                 show_forecast=False, color=True, clean_mesh=True, get_mask_use_all_frames=False,
                 mesh_bound_mask=None):
        """Mesher.get_mesh (:349-574): extracts the mesh, writes it to `mesh_out_file` (binary PLY) and
        returns (vertices (V,3) float64 divided by scale, faces (F,3) int32, colors (V,3) uint8 or None)
        on the device; None when the level set has no surface (the reference's except branch).

        `mesh_bound_mask` is the reference's convex hull (get_bound_from_frames, :421 / :475):
        'frames' builds the FrameBound of `keyframe_dict` at self.scale, as the reference does in every
        extraction; a FrameBound or any callable points (N,3) -> bool (N,) is used as given; a bool
        tensor over the grid points masks the grid alone.  With show_forecast=False it sets the occupancy
        outside it to 100 (:433); with show_forecast=True a callable also culls the faces whose vertices
        all lie outside it (:475-485).  None (the default) applies no hull mask."""
        with torch.no_grad():
            device = torch.device(device)
            if isinstance(mesh_bound_mask, str):
                if mesh_bound_mask != 'frames':
                    raise ValueError(f"pnr.mesher: mesh_bound_mask {mesh_bound_mask!r} (the only name is 'frames')")
                mesh_bound_mask = self.get_bound_from_frames(keyframe_dict, self.scale, device=device)
            grid = self.get_grid_uniform(self.resolution)
            points = grid['grid_points'].to(device)
            masks = dict(keyframe_dict=keyframe_dict, estimate_c2w_list=estimate_c2w_list, idx=idx, device=device,
                         get_mask_use_all_frames=get_mask_use_all_frames)
            if show_forecast:
                seen, forecast, unseen = self.point_masks(points, **masks)
                z = torch.zeros(points.shape[0], dtype=torch.float32, device=device)
                z[forecast] = self.eval_points(points[forecast], decoders, c, 'coarse', device)[:, -1] + 0.2
                z[seen] = self.eval_points(points[seen], decoders, c, 'fine', device)[:, -1]
                z[unseen] = -100
            else:
                z = self.eval_points(points, decoders, c, 'fine', device)[:, -1].contiguous()
                if mesh_bound_mask is not None:
                    inside = mesh_bound_mask(points) if callable(mesh_bound_mask) else mesh_bound_mask
                    z[~inside.to(device).bool()] = 100
            vertices, faces = marching_cubes(z, grid['xyz'], self.level_set)
            if vertices.shape[0] == 0:
                print('marching_cubes error. Possibly no surface extracted from the level set.')
                return None
            if clean_mesh:
                if show_forecast:
                    keep = mesh_bound_mask(vertices).to(device).bool() if callable(mesh_bound_mask) else None
                else:
                    keep = self.point_masks(vertices, **masks)[0]
                vertices, faces = _clean_mesh(
                    vertices, faces, keep, largest=self.get_largest_components,
                    threshold=self.remove_small_geometry_threshold * self.scale * self.scale)
            colors = None
            if color:
                colors = torch.from_numpy(mesh_colors(self.renderer, decoders, c, vertices, faces, device,
                                                      self.color_mesh_extraction_method)).to(device)
                if show_forecast:   # cyan for the forecast region
                    forecast = self.point_masks(vertices, **masks)[1]
                    colors[forecast] = torch.tensor([0, 255, 255], dtype=torch.uint8, device=device)
            vertices = vertices / self.scale
            write_ply(mesh_out_file, vertices, faces, colors)
            if self.verbose:
                print('Saved mesh at', mesh_out_file)
            return vertices, faces, colors
