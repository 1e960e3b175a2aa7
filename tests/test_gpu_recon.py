"""pnr.recon (csrc/recon.hip) against plain float64 numpy brute force, written inline.

nearest: the contract of include/pnr.h `pnr_nn_search`.  With c the query's bounding-box centre and
E = 16 * 2^-53 * (max |q - c| + max |r - c|)^2, every row has dist within 4 ulp of the float64 distance to the
returned index and dist^2 <= min^2 (1 + 2^-27) + 2 E; the index is the argmin wherever the runner-up exceeds that
bound, and at most 1 % of the rows may be excused (on these inputs numpy excuses none).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def pnr_recon():
    import pnr
    return pnr.recon


def brute(q, r):
    return ((q[:, None, :] - r[None, :, :]) ** 2).sum(-1)


def check_nearest(q, r, dist, idx, limit=None):
    """the per-row assertions of the module docstring; q, r float64 numpy"""
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    d2 = brute(q, r)
    rows = np.arange(len(q))
    assert idx.min() >= 0 and idx.max() < len(r)
    got = np.sqrt(d2[rows, idx])
    assert (np.abs(dist - got) <= 4 * np.spacing(got)).all()
    c = 0.5 * (q.min(0) + q.max(0))
    E = 16 * 2.0 ** -53 * (np.linalg.norm(q - c, axis=1).max() + np.linalg.norm(r - c, axis=1).max()) ** 2
    bound = d2.min(1) * (1 + 2.0 ** -27) + 2 * E
    assert (dist ** 2 <= bound).all()
    if len(r) > 1:
        decided = np.partition(d2, 1, axis=1)[:, 1] > bound
        assert (idx[decided] == d2.argmin(1)[decided]).all()
        assert (~decided).mean() <= 0.01


@functools.lru_cache(maxsize=None)
def clouds(Q, R, dtype, seed=0):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, (Q, 3)).astype(dtype), rng.uniform(-1, 1, (R, 3)).astype(dtype)


# (300, 1500): three 512-column chunks, so slices = 1, 2, 3 are all different splits
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('Q,R,slices', [(1, 1, None), (17, 15, None), (257, 1000, None), (1031, 4099, None),
                                        (300, 1500, 2), (300, 1500, 3)])
def test_nearest(dev, Q, R, slices, dtype):
    q, r = clouds(Q, R, dtype)
    tq, tr = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
    dist, idx = pnr_recon().nearest(tq, tr, slices=slices)
    assert dist.dtype == torch.float64 and idx.dtype == torch.int64 and dist.is_cuda
    check_nearest(q.astype(np.float64), r.astype(np.float64), dist, idx)
    # bitwise equal between two calls and between slice counts
    for s in (slices, 1):
        d2, i2 = pnr_recon().nearest(tq, tr, slices=s)
        assert torch.equal(d2, dist) and torch.equal(i2, idx)


def test_nearest_duplicates_take_lower_index(dev):
    q, base = clouds(200, 300, 'float64', seed=1)
    r = np.concatenate([base, base[::-1]])  # every ref point twice; the second copy in another order
    dist, idx = pnr_recon().nearest(torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev))
    assert (idx.cpu().numpy() < 300).all()
    check_nearest(q, base, dist, idx)


def test_nearest_far_from_origin(dev):
    """both clouds shifted by (100, -50, 25), 1e-3 spacing: the centring keeps E small against d^2 ~ 1e-8"""
    rng = np.random.RandomState(2)
    shift = np.array([100.0, -50.0, 25.0])
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing='ij'), -1).reshape(-1, 3)
    r = shift + 1e-3 * g[rng.permutation(len(g))]
    q = r[rng.randint(0, len(r), 300)] + 1e-3 * rng.uniform(-0.3, 0.3, (300, 3))
    dist, idx = pnr_recon().nearest(torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev))
    check_nearest(q, r, dist, idx)


def test_nearest_max_dist(dev):
    q, r = clouds(257, 1000, 'float64')
    tq, tr = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
    d0, i0 = pnr_recon().nearest(tq, tr)
    limit = float(d0.median())
    d1, i1 = pnr_recon().nearest(tq, tr, max_dist=limit)
    far = d0 > limit
    assert 0 < int(far.sum()) < 257
    assert (i1[far] == -1).all() and torch.isinf(d1[far]).all()
    assert torch.equal(d1[~far], d0[~far]) and torch.equal(i1[~far], i0[~far])


# ---- sample_surface -------------------------------------------------------------------------------------------
VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.5], [2, 0, 0]], dtype=np.float64)
FACES = np.array([[0, 5, 1], [0, 1, 2], [0, 1, 3], [1, 2, 4], [0, 2, 3]])  # face 0 is collinear: zero area


def sample_np(v, f, u):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
    target = u[:, 0] * cum[-1]
    face = np.array([np.argmax((cum >= t) & (cum > 0)) for t in target])
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    flip = u1 + u2 > 1
    u1[flip], u2[flip] = 1 - u1[flip], 1 - u2[flip]
    a, b, c = a[face], b[face], c[face]
    return ((b - a) * u1[:, None] + (c - a) * u2[:, None]) + a, face


def test_sample_surface_rule(dev):
    rng = np.random.RandomState(3)
    u = rng.uniform(0, 1, (64, 3))
    u[0] = [0.0, 0.25, 0.25]  # u0 = 0 must skip the zero-area face 0
    u[1] = [0.5, 0.75, 0.5]   # needs the reflection
    u[2] = [1.0 - 2.0 ** -53, 0.1, 0.2]
    want, face = sample_np(VERTS, FACES, u)
    v, f = torch.from_numpy(VERTS).to(dev), torch.from_numpy(FACES).to(dev)
    pts, fi = pnr_recon().sample_surface(v, f, 64, uniforms=torch.from_numpy(u).to(dev))
    assert (fi.cpu().numpy() == face).all() and (face != 0).all()
    assert (np.abs(pts.cpu().numpy() - want) <= 4 * np.spacing(np.abs(want))).all()


def test_sample_surface_generator(dev):
    v, f = torch.from_numpy(VERTS).to(dev), torch.from_numpy(FACES).to(dev)
    p0, f0 = pnr_recon().sample_surface(v, f, 1000, seed=7)
    p1, f1 = pnr_recon().sample_surface(v, f, 1000, seed=7)
    p2, _ = pnr_recon().sample_surface(v, f, 1000, seed=8)
    assert torch.equal(p0, p1) and torch.equal(f0, f1) and not torch.equal(p0, p2)
    face = f0.cpu().numpy()
    assert (face != 0).all() and face.min() >= 1 and face.max() <= 4
    a, b, c = (VERTS[FACES[face, k]] for k in range(3))
    M = np.stack([b - a, c - a], -1)  # (n,3,2): p - a = M (s, t)
    st = np.linalg.solve(M.transpose(0, 2, 1) @ M, (M.transpose(0, 2, 1) @ (p0.cpu().numpy() - a)[..., None]))[..., 0]
    assert (st >= -1e-12).all() and (st.sum(1) <= 1 + 1e-12).all()
    # area ratio 3:1 over two triangles: the share of the large one within 4 sigma of 0.75
    v2 = torch.tensor([[0, 0, 0], [3, 0, 0], [0, 1, 0], [0, -1, 0], [1, -1, 0]], dtype=torch.float64, device=dev)
    f2 = torch.tensor([[0, 1, 2], [0, 3, 4]], device=dev)
    _, fi = pnr_recon().sample_surface(v2, f2, 20000, seed=0)
    share = float((fi == 0).double().mean())
    assert abs(share - 0.75) <= 4 * np.sqrt(0.75 * 0.25 / 20000)


# ---- metrics --------------------------------------------------------------------------------------------------
def test_metrics(dev):
    rng = np.random.RandomState(4)
    gt, rec = rng.uniform(0, 0.3, (300, 3)), rng.uniform(0, 0.3, (500, 3))
    d2 = brute(gt, rec)
    to_rec, to_gt = np.sqrt(d2.min(1)), np.sqrt(d2.min(0))
    want = (to_gt.mean(), to_rec.mean(), (to_rec < 0.05).mean())
    tg, tr = torch.from_numpy(gt).to(dev), torch.from_numpy(rec).to(dev)
    R = pnr_recon()
    got = (R.accuracy(tg, tr), R.completion(tg, tr), R.completion_ratio(tg, tr))
    assert 0 < want[2] < 1
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert got == (R.accuracy(tg, tr), R.completion(tg, tr), R.completion_ratio(tg, tr, dist_th=0.05))


# ---- ICP --------------------------------------------------------------------------------------------------------
def rotation(axis, deg):
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def icp_np(src, dst, thr, iters=30):
    """the rule of pnr.recon.icp: brute NN within thr, Kabsch with the reflection fix, open3d's stop test"""
    def step(T):
        p = src @ T[:3, :3].T + T[:3, 3]
        d2 = brute(p, dst)
        idx = d2.argmin(1)
        d = np.sqrt(d2[np.arange(len(p)), idx])
        keep = d <= thr
        a, b = p[keep], dst[idx[keep]]
        ma, mb = a.mean(0), b.mean(0)
        U, _, Vt = np.linalg.svd((a - ma).T @ (b - mb))
        R = Vt.T @ np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
        Tn = np.eye(4)
        Tn[:3, :3], Tn[:3, 3] = R, mb - R @ ma
        return Tn @ T, keep.mean(), np.sqrt((d[keep] ** 2).mean())
    T = np.eye(4)
    Tn, f, r = step(T)
    for _ in range(iters):
        T, before = Tn, (f, r)
        Tn, f, r = step(T)
        if abs(before[0] - f) < 1e-6 and abs(before[1] - r) < 1e-6:
            break
    return T, f, r


def test_icp(dev):
    rng = np.random.RandomState(0)
    src = rng.uniform(-1, 1, (2000, 3))
    t = rng.randn(3)
    t *= 0.02 / np.linalg.norm(t)
    dst = src @ rotation([1, 2, 3], 3.0).T + t
    want, _, _ = icp_np(src, dst, 0.1)
    T, fitness, rmse = pnr_recon().icp(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), threshold=0.1)
    T = T.cpu().numpy()
    print('icp |dR|', np.abs(T[:3, :3] - want[:3, :3]).max(), '|dt|', np.abs(T[:3, 3] - want[:3, 3]).max(), rmse)
    # Spread of two float64 implementations of this iteration: icp_np against itself with the matched pairs
    # summed in reverse order, from the same start, gave max |dR| = 4.7e-16 and max |dt| = 2.9e-17 on these
    # inputs.  Allowed: 10 times that.
    assert np.abs(T[:3, :3] - want[:3, :3]).max() <= 4.7e-15
    assert np.abs(T[:3, 3] - want[:3, 3]).max() <= 2.9e-16
    assert np.abs(src @ T[:3, :3].T + T[:3, 3] - dst).max() < 1e-9
    assert fitness == 1.0 and (T[3] == [0, 0, 0, 1]).all()


# ---- calc_3d_metric ---------------------------------------------------------------------------------------------
def test_calc_3d_metric_cube(dev, tmp_path):
    """A unit cube through write_ply / read_ply.  Against itself both means stay below the sample spacing.  A
    copy shifted by 0.03 along x leaves every point within 0.03 of the other surface, so its ratio is 100 % and
    its completion lies in (0, 3] cm; the ratio strictly between 0 and 100 needs a shift above dist_th = 0.05
    (0.06: the two faces across x leave the band, the other four stay on the surface)."""
    import pnr
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    n = 20000
    paths = {}
    for name, dx in (('gt', 0.0), ('near', 0.03), ('far', 0.06)):
        paths[name] = str(tmp_path / (name + '.ply'))
        pnr.mesher.write_ply(paths[name], v + [dx, 0, 0], f)
    rv, rf = pnr.recon.read_ply(paths['gt'], dev)
    assert rv.dtype == torch.float64 and (rv.cpu().numpy() == v).all() and (rf.cpu().numpy() == f).all()
    m = pnr.calc_3d_metric(paths['gt'], paths['gt'], n_points=n)
    spacing_cm = 100 * np.sqrt(6.0 / n)
    assert 0 < m['accuracy_cm'] < spacing_cm and 0 < m['completion_cm'] < spacing_cm
    assert m['completion_ratio_pct'] == 100.0
    assert torch.allclose(m['transformation'], torch.eye(4, dtype=torch.float64, device=dev), atol=1e-12)
    m = pnr.calc_3d_metric(paths['near'], (rv, rf), align=False, n_points=n)
    assert 0 < m['completion_cm'] <= 3.0 and m['completion_ratio_pct'] == 100.0
    m = pnr.calc_3d_metric(paths['far'], paths['gt'], align=False, n_points=n)
    assert 0 < m['completion_ratio_pct'] < 100
