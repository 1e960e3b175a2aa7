"""The mesh depth rasteriser (csrc/raster.hip, pnr.recon) against the rule of include/pnr.h "mesh depth
rasteriser", evaluated in inline float64 numpy for every (pixel, face) pair.

A pixel is undecided, and excused, when the reference finds a face with an |E_k| <= 2^-40 (|a j| + |b i| + |c|)
whose other two edge values do not reject it, or a winning z within 2^-40 relative of z_near or z_far; at most 1 %
may be excused (on these inputs numpy excuses none).  On decided pixels both images are covered or both empty, and
a covered depth is within 1 float32 ulp of float32(reference): the float64 error is far below 2^-25.  That premise,
checked once on the CPU: the same formula in np.longdouble covers the same pixels and differs from the float64
reference by at most 5.0e-12 relative (below 2^-37) on the inputs below.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -40


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def recon():
    import pnr
    return pnr.recon


def camera(M, x):
    """p = R^T (x - t) for c2w = [R t], summed as the header states"""
    d = x - M[:3, 3]
    return (d[:, 0:1] * M[0, :3] + d[:, 1:2] * M[1, :3]) + d[:, 2:3] * M[2, :3]


def reference(v, f, M, H, W, K, zn=0.01, zf=20.0, dt=np.float64):
    """(depth (H,W) with inf where empty, undecided (H,W)) of one view by the header's rule"""
    fx, fy, cx, cy = (dt(k) for k in K)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    p = camera(M.astype(dt), v.astype(dt))
    q = np.stack([fx * p[:, 0] + cx * p[:, 2], fy * p[:, 1] + cy * p[:, 2], p[:, 2]], 1)[f]
    jj, ii = np.meshgrid(np.arange(W).astype(dt), np.arange(H).astype(dt))
    E, near = [], []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        sw = (f[:, i] > f[:, j])[:, None]
        n = np.where(sw, -1, 1) * np.cross(np.where(sw, q[:, j], q[:, i]), np.where(sw, q[:, i], q[:, j]))
        if k == 0:
            det = (q[:, 0, 0] * n[:, 0] + q[:, 0, 1] * n[:, 1]) + q[:, 0, 2] * n[:, 2]
        a, b, c = (n[:, m, None, None] for m in range(3))
        e = (a * jj + b * ii) + c
        near.append(np.abs(e) <= dt(TOL) * (np.abs(a * jj) + np.abs(b * ii) + np.abs(c)))
        E.append(e * np.sign(det)[:, None, None])
    live = (det != 0)[:, None, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        z = np.abs(det)[:, None, None] / ((E[0] + E[1]) + E[2])
    kept = live & (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0) & (z >= zn) & (z <= zf)
    depth = np.where(kept, z, np.inf).min(0)
    passes = [(E[k] >= 0) | near[k] for k in range(3)]
    und = (live & (near[0] | near[1] | near[2]) & passes[0] & passes[1] & passes[2]).any(0)
    und |= np.isfinite(depth) & ((np.abs(depth - zn) <= TOL * zn) | (np.abs(depth - zf) <= TOL * zf))
    return depth, und


def pose(rng):
    """a rigid camera-to-world pose near the identity"""
    R, _ = np.linalg.qr(np.eye(3) + 0.3 * rng.standard_normal((3, 3)))
    R *= np.sign(np.diag(R))
    R[:, 2] *= np.linalg.det(R)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, 0.3 * rng.standard_normal(3)
    return M


@functools.lru_cache(maxsize=None)
def scene(H, W, F, views):
    """(verts, faces, c2w, K, z_near, references): triangles of mixed sizes in a box that straddles the camera, so some
    cross z_near, some lie behind, beyond z_far or off-screen; with F >= 4 the last three faces span every tile,
    are degenerate and hold an out-of-range index"""
    rng = np.random.RandomState(H * 1000 + W)
    K, zn = (40.0, 40.0, W / 2 - 0.5, H / 2 - 0.5), (1.0 if F > 100 else 0.01)  # z_near = 1: crossing faces of modest size
    c2w = np.stack([np.eye(4)] + [pose(rng) for _ in range(views - 1)])
    if F == 1:
        v = np.array([[-100.0, -100.0, 3.0], [100.0, -90.0, 4.0], [5.0, 200.0, 5.0]])
        f = np.array([[0, 1, 2]])
    else:
        centre = rng.uniform([-3, -3, -2], [3, 3, 25], (F, 1, 3))
        centre[::3, :, 2] = rng.uniform(-1, 3, (len(centre[::3]), 1))  # a third of them about the camera and z_near
        if W == 1:
            centre[:, :, 0] *= 0.02
        size = rng.choice([0.002, 0.05, 0.3, 0.6, 2.0], (F, 1, 1), p=[0.2, 0.3, 0.3, 0.17, 0.03])
        v = (centre + size * rng.uniform(-1, 1, (F, 3, 3))).reshape(-1, 3)
        f = np.arange(3 * F).reshape(F, 3)
        m = np.arange(0, F // 3, 2)  # face m + 1 becomes face m's mirror across their shared edge, traversed the other way
        v[3 * m + 5] = v[3 * m] + v[3 * m + 1] - v[3 * m + 2]
        f[m + 1] = np.stack([3 * m + 1, 3 * m, 3 * m + 5], 1)
        if F >= 4:
            corners = [(-5.3, -4.7, 15.0), (W + 5.6, -5.2, 16.0), (-4.9, H + 5.4, 17.0)]  # (u, v, z): half the image
            v[-9:-6] = [[(u - K[2]) * z / K[0], (w - K[3]) * z / K[1], z] for u, w, z in corners]
            f[-2] = [5, 5, 9]
            f[-1] = [0, 1, 3 * F]
    return v, f, c2w, K, zn, [reference(v, f, M, H, W, K, zn) for M in c2w]


@pytest.mark.parametrize('ftype', [torch.int32, torch.int64])
@pytest.mark.parametrize('H,W,F,views,view_batch', [(50, 70, 300, 2, 1), (50, 70, 300, 2, 2), (32, 32, 1, 1, None),
                                                    (33, 1, 40, 1, None)])
def test_images(dev, H, W, F, views, view_batch, ftype):
    v, f, c2w, K, zn, refs = scene(H, W, F, views)
    args = (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev, ftype), torch.from_numpy(c2w).to(dev), H, W, *K, zn)
    got = recon().render_depth(*args, view_batch=view_batch)
    assert got.shape == (views, H, W) and got.dtype == torch.float32 and got.is_cuda
    # bitwise equal on a rerun and across view batches
    assert torch.equal(got, recon().render_depth(*args, view_batch=view_batch))
    assert torch.equal(got, recon().render_depth(*args, view_batch=3 - (view_batch or 1)))
    got = got.cpu().numpy()
    for img, (want, und) in zip(got, refs):
        print('covered', np.isfinite(want).mean(), 'excused', und.mean())
        assert und.mean() <= 0.01
        ok = ~und
        assert ((img != 0) == np.isfinite(want))[ok].all()
        hit = ok & np.isfinite(want)
        w32 = want[hit].astype(np.float32)
        assert (np.abs(img[hit].astype(np.float64) - w32) <= np.spacing(w32)).all()
    if F > 1 and W > 1:  # the mixture the case is there for
        assert 0.3 < np.isfinite(refs[0][0]).mean() < 0.9 and (got[0] < 14).any()


def plane(z, us, vs, K):
    """a grid of quads at depth z whose vertices project onto pixel coordinates us x vs: (verts, faces)"""
    fx, fy, cx, cy = K
    uu, vv = np.meshgrid(us, vs)
    v = np.stack([(uu - cx) * z / fx, (vv - cy) * z / fy, np.full(uu.shape, z)], -1).reshape(-1, 3)
    idx = np.arange(len(us) * len(vs)).reshape(len(vs), len(us))
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])


def test_watertight(dev):
    K = (16.0, 16.0, 23.5, 23.5)
    k = np.arange(25)
    grid = 2.0 * k - 0.5 * (k % 2 == 0)  # -0.5, 2, 3.5, 6, ... 47.5: half-pixels and pixel centres
    v, f = plane(2.5, grid, grid, K)
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None]
    img = recon().render_depth(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), eye, 48, 48, *K)
    assert (img == 2.5).all()
    # a nearer half-plane whose edge runs through the centres of column 24: it wins on columns 0..24 exactly
    v2, f2 = plane(1.25, np.array([-8.5, 24.0]), np.array([-8.5, 56.5]), K)
    both_v, both_f = np.concatenate([v, v2]), np.concatenate([f, f2 + len(v)])
    img = recon().render_depth(torch.from_numpy(both_v).to(dev), torch.from_numpy(both_f).to(dev), eye, 48, 48, *K)
    want = np.full((48, 48), 2.5, np.float32)
    want[:, :25] = 1.25
    assert np.array_equal(img[0].cpu().numpy(), want)


def test_depth_l1(dev):
    rng = np.random.RandomState(3)
    a, b = (rng.uniform(0, 5, (3, 50, 70)).astype(np.float32) for _ in range(2))
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    got = recon().depth_l1(ta, tb)
    assert got.dtype == torch.float64 and torch.equal(got, recon().depth_l1(ta, tb))
    want = np.abs(a.astype(np.float64) - b.astype(np.float64)).mean((1, 2))
    print('depth_l1 ulps', np.abs(got.cpu().numpy() - want) / np.spacing(want))
    assert (np.abs(got.cpu().numpy() - want) <= 4 * np.spacing(want)).all()


def seen_np(pts, c2w, H, W, K):
    """(seen (n,P), undecided (n,P)): check_proj's test as include/pnr.h `pnr_frustum_seen` states it"""
    fx, fy, cx, cy = K
    seen, und = [], []
    for M in c2w:
        p = camera(M, pts)
        zz = p[:, 2] + 1e-5
        u, v = (fx * p[:, 0] + cx * p[:, 2]) / zz, (fy * p[:, 1] + cy * p[:, 2]) / zz
        seen.append((zz > 0) & (u > 0) & (u < W) & (v > 0) & (v < H))
        und.append((np.abs(zz) <= TOL) | (np.abs(u) <= TOL) | (np.abs(u - W) <= TOL * W) | (np.abs(v) <= TOL)
                   | (np.abs(v - H) <= TOL * H))
    return np.array(seen), np.array(und)


def test_frustum_and_cull(dev):
    rng = np.random.RandomState(4)
    H, W, K = 48, 64, (40.0, 40.0, 31.5, 23.5)
    pts = rng.uniform(-6, 6, (500, 3))
    c2w = np.stack([pose(rng) for _ in range(5)])
    seen, und = seen_np(pts, c2w, H, W, K)
    assert und.mean() <= 0.01 and 0.05 < seen.any(0).mean() < 0.95
    tp, tc = torch.from_numpy(pts).to(dev), torch.from_numpy(c2w).to(dev)
    by_point = recon().points_seen(tp, tc, H, W, *K).cpu().numpy()
    ok = ~und.any(0)
    assert by_point.dtype == bool and (by_point == seen.any(0))[ok].all()
    few = (seen.sum(0) == 1).nonzero()[0][:2]  # two points that one view each sees, and all of them
    assert 0 < seen[:, few].any(1).sum() < 5
    for sub in (np.arange(500), few):
        by_view = recon().views_seeing(tp[torch.from_numpy(sub).to(dev)], tc, H, W, *K).cpu().numpy()
        assert (by_view == seen[:, sub].any(1))[~und[:, sub].any(1)].all()
    faces = rng.randint(0, 500, (300, 3))
    _, kept = recon().cull_mesh(tp, torch.from_numpy(faces).to(dev), tc, H, W, *K)
    assert ok.all() and np.array_equal(kept.cpu().numpy(), faces[seen.any(0)[faces].any(1)])


def box_mesh(lo, hi):
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def test_calc_2d_metric(dev):
    v, f = box_mesh((-2, -2, -1), (2, 2, 1))
    gt = (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
    res = recon().calc_2d_metric(gt, gt, align=False, n_imgs=4)
    assert res['depth_l1_cm'] == 0.0 and res['views'].shape == (4, 4, 4) and res['per_view'].shape == (4,)
    # from (1.5, 0, 0) down +x the wall x = 2 fills the image at depth 0.5; the copy's wall is at 0.51
    view = np.eye(4)
    view[:3, :3] = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])  # columns: camera x = +y, y = +z, z = +x
    view[:3, 3] = [1.5, 0, 0]
    rec = (torch.from_numpy(v + [0.01, 0, 0]).to(dev), gt[1])
    res = recon().calc_2d_metric(rec, gt, align=False, views=view[None])
    assert abs(res['depth_l1_cm'] - 1.0) <= 1e-4
    unseen = np.array([[0.5, 0.5, 0.3]])
    res = recon().calc_2d_metric(gt, gt, align=False, n_imgs=4, pc_unseen=unseen, seed=1)
    assert not seen_np(unseen, res['views'].cpu().numpy(), 500, 500, (300.0, 300.0, 249.5, 249.5))[0].any()
