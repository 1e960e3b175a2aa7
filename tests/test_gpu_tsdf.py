"""The block-sparse TSDF volume (csrc/tsdf.hip, pnr.TSDFVolume) against its float64 restatement
(tests/tsdf_ref.py), and the mesh bound over its surface (pnr.mesher.get_bound_from_frames(surface='tsdf')).

Shapes: 48 x 64 images, fx = fy = 40, scale 1 (voxel 4 / 512, 16-voxel blocks of 0.125), sdf_trunc = 5.12 voxels,
a directory of 4 x 4 x 3 blocks.  The boxes' low corners were chosen so that no p +- sdf_trunc of the reference
comes within 1e-4 of a block boundary (asserted): the allocated sets must then be equal.

The error bound of tsdf and rgb on the voxels the reference does not flag as edges: every rounded float32
operation errs by at most 2^-24 of its result, and results on the way to zc are at most 2 max|coordinate| (q = X - t),
hence 2^-23 max|coordinate| each.  On the way from the inputs to s = min(1, sdf / sdf_trunc): X_a 2 and q_a 1 per
axis (9), the three products and two sums of P_2 (5), d - zc (1), the product with m (1), m's own nine
((u - cx) / fx, (v - cy) / fy: 4; two squares, two sums, the root: 5), the division (1): 26, scaled by m_max /
sdf_trunc.  The running average adds three roundings of values <= 1 per frame, at most 9 with K <= 3, which the same
unit covers because max|coordinate| m_max / sdf_trunc >= 1 (asserted).  C = 35."""
import numpy as np
import pytest
import torch

import tsdf_ref

pytestmark = pytest.mark.gpu

H, W = 48, 64
CAM = dict(fx=40.0, fy=40.0, cx=31.5, cy=23.5)
CAM_T = (H, W) + tuple(CAM.values())
VL = 4.0 / 512.0
TRUNC = 5.12 * VL
DIMS = (4, 4, 3)
C_OPS = 35


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def look_at(eye, target, roll=0.0):
    """c2w float32 of a camera at `eye` looking down its -z at `target`, y up, rolled about the view axis."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, [0.0, 0.3, 1.0] if abs(f[2]) < 0.9 else [0.2, 1.0, 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    r, u = np.cos(roll) * r + np.sin(roll) * u, np.cos(roll) * u - np.sin(roll) * r
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, eye
    return m.astype(np.float32)


def pixel_rays(c2w):
    """World origin (3,) and per-pixel directions (H,W,3) with camera z = -1, float64: depth is the parameter."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = np.stack([(u - CAM['cx']) / CAM['fx'], -(v - CAM['cy']) / CAM['fy'], -np.ones_like(u, float)], -1)
    return c2w[:3, 3].astype(np.float64), d @ c2w[:3, :3].astype(np.float64).T


def plane_depth(c2w, point, normal):
    o, d = pixel_rays(c2w)
    t = ((np.asarray(point) - o) @ np.asarray(normal)) / (d @ np.asarray(normal))
    return np.where(t > 0, t, 0.0).astype(np.float32)


def sphere_depth(c2w, centre, radius):
    o, d = pixel_rays(c2w)
    oc = o - np.asarray(centre)
    a, b, c = (d * d).sum(-1), (d @ oc), oc @ oc - radius ** 2
    disc = b * b - a * c
    t = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
    return np.where((disc > 0) & (t > 0), t, 0.0).astype(np.float32)


def case_frames(name):
    """(bound (3,2), [(depth, colour, c2w)]) of a case; the bounds' low corners carry the searched offsets."""
    if name == 'plane':
        c2w = [look_at([0.01, -0.02, 0.27], [0.01, -0.02, 0.0], 0.1)]
        depth = [plane_depth(c2w[0], [0, 0, 0.013], [0, 0, 1.0])]
        lo = np.array([-0.2 + 0.00471, -0.2 + 0.00569, -0.14 + 0.0055])
    elif name == 'sphere':
        c2w = [look_at([0.05, -0.5, 0.1], [0, 0, 0], 0.2), look_at([0.45, 0.3, -0.05], [0.3, 0.0, 0.0], -0.4),
               look_at([0.17, 0.16, 0.1], [0, 0, 0], 0.7)]      # outside; sees a part; inside the box
        depth = [sphere_depth(m, [0.0, 0.0, 0.0], 0.15) for m in c2w]
        depth[0][10, 20:24], depth[1][30, 5], depth[2][7, 40], depth[2][20, 31] = 0.0, np.nan, np.inf, 1500.0
        lo = np.array([-0.2 + 0.00278, -0.2 + 0.00132, -0.14 + 0.00024])
    else:
        c2w = [look_at([0.1, 0.0, 0.6], [0, 0, 0], 0.3)]
        depth = [plane_depth(c2w[0], [0, 0, 0.0], [0.5, 0.0, np.sqrt(0.75)])]   # leaves the box on every side
        lo = np.array([-0.2 + 0.00476, -0.2 + 0.00276, -0.14 + 0.00593])
    col = np.random.RandomState(len(name)).uniform(0, 1, (len(c2w), H, W, 3)).astype(np.float32)
    bound = np.stack([lo, lo + np.array([0.4, 0.4, 0.28])], 1)
    return bound, [(depth[k], col[k], c2w[k]) for k in range(len(c2w))]


def make_volume(pnr, dev, bound, max_blocks=64):
    vol = pnr.TSDFVolume(bound, VL, TRUNC, H, W, max_blocks=max_blocks, device=dev, **CAM)
    assert tuple(vol.dims) == DIMS
    return vol


def stack(frames):
    return tuple(torch.from_numpy(np.stack([f[i] for f in frames])) for i in range(3))


_cache = {}


def fused(pnr, dev, name):
    """(volume fused in one call, the reference, the frames), computed once per case."""
    if name not in _cache:
        bound, frames = case_frames(name)
        vol = make_volume(pnr, dev, bound)
        vol.integrate(*stack(frames))
        ref = tsdf_ref.fuse([frames], vol.origin, VL, TRUNC, DIMS, CAM_T)
        _cache[name] = (vol, ref, frames, bound)
    return _cache[name]


def sorted_blocks(vol):
    b = vol.blocks()
    order = torch.argsort(b['index'])
    return b['index'][order], b['tsdf'][order], b['weight'][order], b['rgb'][order]


@pytest.mark.parametrize('name', ['plane', 'sphere', 'leaving'])
def test_fuse_matches_the_float64_rules(dev, name):
    import pnr
    vol, ref, frames, _ = fused(pnr, dev, name)
    assert ref['margin'] > 1e-4, ref['margin']
    b = vol.blocks()
    index = b['index'].cpu().numpy()
    assert np.array_equal(index, ref['slots']) and (np.diff(index) > 0).all()      # the same set, in entry order
    assert vol.n_blocks == len(ref['slots']) > 0 and vol.dropped_blocks == 0
    share = ref['edge'][ref['allocated']].mean()
    unit = ref['coord_max'] * ref['m_max'] / float(np.float32(TRUNC))
    bound = C_OPS * 2.0 ** -23 * unit
    assert share <= 0.05 and unit >= 1.0
    worst = {'tsdf': 0.0, 'rgb': 0.0}
    updated = 0
    for s, e in enumerate(index):
        keep = ~tsdf_ref.block_view(ref['edge'], e, DIMS)
        want_w = tsdf_ref.block_view(ref['weight'], e, DIMS)
        assert np.array_equal(b['weight'][s].cpu().numpy()[keep], want_w[keep].astype(np.float32))
        updated += int((want_w[keep] > 0).sum())
        worst['tsdf'] = max(worst['tsdf'], np.abs(b['tsdf'][s].cpu().numpy().astype(np.float64)
                                                  - tsdf_ref.block_view(ref['tsdf'], e, DIMS))[keep].max(initial=0.0))
        got_rgb = b['rgb'][s].cpu().numpy().astype(np.float64).transpose(1, 2, 3, 0)
        worst['rgb'] = max(worst['rgb'], np.abs(got_rgb - tsdf_ref.block_view(ref['rgb'], e, DIMS))[keep].max(initial=0.0))
    print(name, 'blocks', len(index), 'updated voxels', updated, 'edge share', share, 'bound', bound, 'worst', worst,
          'margin', ref['margin'], 'max weight', ref['weight'].max())
    assert updated > 1000 and ref['weight'].max() == len(frames)
    assert worst['tsdf'] <= bound and worst['rgb'] <= bound


def test_batching_and_reruns_are_bitwise(dev):
    import pnr
    vol, _, frames, bound = fused(pnr, dev, 'sphere')
    again, split = make_volume(pnr, dev, bound), make_volume(pnr, dev, bound)
    again.integrate(*stack(frames))
    assert all(torch.equal(x, y) for x, y in zip(sorted_blocks(vol), sorted_blocks(again)))
    assert torch.equal(vol.blocks()['index'], again.blocks()['index'])
    split.integrate(*(torch.from_numpy(a) for a in frames[0]))            # one frame, unbatched
    n0 = split.n_blocks
    split.integrate(*stack(frames[1:]))
    assert 0 < n0 < split.n_blocks == vol.n_blocks
    assert all(torch.equal(x, y) for x, y in zip(sorted_blocks(vol), sorted_blocks(split)))
    assert not torch.equal(vol.blocks()['index'], split.blocks()['index'])   # only the slot order differs


@pytest.mark.parametrize('name', ['sphere', 'leaving'])
def test_extract_points_is_the_rule_on_the_device_volume(dev, name):
    import pnr
    vol = fused(pnr, dev, name)[0]
    b = vol.blocks()
    xyz, rgb = vol.extract_points()
    want_xyz, want_rgb = tsdf_ref.extract(b['tsdf'].cpu().numpy(), b['weight'].cpu().numpy(), b['rgb'].cpu().numpy(),
                                          b['index'].cpu().numpy().astype(np.int64), vol.origin, VL, DIMS)
    assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.shape == want_xyz.shape and xyz.shape[0] > 500
    # X0: 2 roundings, s: 2, the product and the sum: 2, of magnitudes <= max|xyz| + voxel; colours are <= 1
    atol = 6 * 2.0 ** -24 * (np.abs(want_xyz).max() + VL)
    err_xyz, err_rgb = np.abs(xyz.cpu().numpy() - want_xyz).max(), np.abs(rgb.cpu().numpy() - want_rgb).max()
    print(name, 'points', xyz.shape[0], 'xyz error', err_xyz, 'of', atol, 'rgb error', err_rgb)
    assert err_xyz <= atol and err_rgb <= 6 * 2.0 ** -24
    xyz2, rgb2 = vol.extract_points()
    assert torch.equal(xyz, xyz2) and torch.equal(rgb, rgb2)
    crosses_blocks = (np.floor((want_xyz - vol.origin) / VL - 0.5).astype(int) % 16 == 15).any(0)
    assert crosses_blocks.all()     # crossings between voxels of neighbouring blocks, on every axis


def test_blocks_past_max_blocks_are_dropped_in_entry_order(dev):
    import pnr
    vol, ref, frames, bound = fused(pnr, dev, 'sphere')
    room = vol.n_blocks - 5
    small = make_volume(pnr, dev, bound, max_blocks=room)
    small.integrate(*stack(frames))                                        # returns 0: no exception
    assert small.n_blocks == room and small.dropped_blocks == 5
    want = tsdf_ref.fuse([frames], vol.origin, VL, TRUNC, DIMS, CAM_T, max_blocks=room)
    assert want['dropped'] == 5 and np.array_equal(small.blocks()['index'].cpu().numpy(), want['slots'])
    full, part = vol.blocks(), small.blocks()
    assert all(torch.equal(full[k][:room], part[k]) for k in ('index', 'tsdf', 'weight', 'rgb'))
    small.integrate(*stack(frames[:1]))                                    # a dropped block is counted once
    assert small.n_blocks == room and small.dropped_blocks == 5


def test_bound_from_frames_over_the_tsdf_surface(dev):
    """A plane 0.8 in front of a camera that looks along the grid's diagonal, and one pixel at depth 1.6.  Around the
    outlier only that pixel can update a voxel (to its neighbours the place lies behind the plane), and the pixel's
    pencil there is at most sqrt(2) zc / fx across, which is less than the distance vl sqrt(1 - max dir_a^2)
    between the ray and the second of two voxel centres that are neighbours along an axis (asserted): no two
    neighbours both have a weight, so the outlier leaves no crossing, while the hull over the pixels holds it."""
    import pnr
    Hb, Wb, cam = 192, 256, dict(fx=800.0, fy=800.0, cx=127.5, cy=95.5)
    c2w = look_at([0.01, 0.02, 0.03], [1.0, 1.1, 0.9], 0.3)
    depth = np.full((Hb, Wb), 0.8, np.float32)
    depth[80, 160] = 1.6
    ray = c2w[:3, :3].astype(np.float64) @ np.array([(160 - cam['cx']) / cam['fx'], -(80 - cam['cy']) / cam['fy'], -1.0])
    outlier = c2w[:3, 3] + ray * 1.6
    axis = np.abs(ray / np.linalg.norm(ray)).max()
    assert np.sqrt(2) * (1.6 + 2 * TRUNC) / cam['fx'] < VL * np.sqrt(1 - axis ** 2)
    kfs = [{'depth': torch.from_numpy(depth).to(dev), 'est_c2w': torch.from_numpy(c2w)}]
    kw = dict(scale=1.0, device=dev, **cam)
    by_pixels = pnr.mesher.get_bound_from_frames(kfs, Hb, Wb, **kw)
    fb = pnr.mesher.get_bound_from_frames(kfs, Hb, Wb, surface='tsdf', max_blocks=512, **kw)
    surf = fb.volume.extract_points()[0]
    print('tsdf bound', fb.stats)
    assert fb.stats['tsdf_dropped_blocks'] == 0 and fb.stats['surface_points'] == surf.shape[0] > 200
    assert bool(fb.contains(surf).all()) and bool(fb.contains(torch.from_numpy(c2w[None, :3, 3])).all())
    point = torch.from_numpy(outlier[None]).to(dev)
    assert bool(by_pixels.contains(point).all()) and not bool(fb.contains(point).any())
    zc = -((surf.cpu().numpy().astype(np.float64) - c2w[:3, 3]) @ c2w[:3, :3].astype(np.float64))[:, 2]
    assert zc.max() < 0.8 + 2 * TRUNC and abs(zc - 0.8).min() < VL
