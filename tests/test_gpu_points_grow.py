"""Growing the neural-point map on the GPU (pnr.NeuralPoints.add_frame -> pnr_points_add_frame) against
the numpy restatement tests/points_grow_ref.py.

Positions are held to a rounding bound against a float64 back-projection; every decision is then
compared EXACTLY: the restatement is fed the device's own float32 candidate positions (teacher
forcing), and every rule is a function of those positions alone, so flags, counters and the appended
rows must be equal bit for bit -- no tolerance and no left-out share.  The rows a call must not touch
are pre-filled with a NaN bit pattern and compared as integers.

Camera: the 48x64 camera of tests/test_gpu_parity.py (fx 50, fy 51, cx 31.5, cy 23.5) at golden pose 1
of the room0 scene."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_params
import points_grow_ref as G

pytestmark = pytest.mark.gpu

H, W, FX, FY, CX, CY = 48, 64, 50.0, 51.0, 31.5, 23.5
RADIUS = 0.03
RHO3 = (-0.02, 0.0, 0.02)
NAN_BITS = 0x7FC01234


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def pnr_mod():
    import pnr
    pnr.library()
    return pnr


def scene():
    s = load_golden('scene.npz')
    return s['bound'].astype(np.float64), s['poses'][1].astype(np.float32)


def frame_depth(seed=0, special=True):
    """A surface 0.25-0.6 from the camera that leaves the room on the image's right side, with the
    depth values a sensor can hand over: 0, negative, NaN and +inf."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = 0.42 + 0.1 * np.sin(u / 9.0 + seed) + 0.07 * np.cos(v / 7.0) + np.where(u > 54, 0.9, 0.0)
    d = d.astype(np.float32)
    if special:
        rng = np.random.default_rng(100 + seed)
        k = rng.integers(0, 8, (H, W))
        d[k == 0] = np.array([0.0, -0.3, np.nan, np.inf], np.float32)[rng.integers(0, 4, int((k == 0).sum()))]
    return d


def random_cloud(bound, n=3000, seed=3):
    gen = torch.Generator().manual_seed(seed)
    lo, hi = torch.from_numpy(bound[:, 0]).float(), torch.from_numpy(bound[:, 1]).float()
    xyz = lo + (hi - lo) * torch.rand((n, 3), generator=gen)
    feats = torch.randn((n, 32), generator=gen) * 0.5
    return xyz, feats


def make_cloud(pnr, dev, xyz, feats, capacity, bound, **kw):
    kw.setdefault('radius', RADIUS)
    pts = pnr.NeuralPoints(xyz.to(dev), None if feats is None else feats.to(dev), mode='idw', k=8,
                           capacity=capacity, bound=bound, **kw).to(dev)
    n = pts.n_points
    with torch.no_grad():  # the rows a call must leave alone carry a NaN pattern
        pts.xyz[n:].view(torch.int32).fill_(NAN_BITS)
        pts.feats.data[n:].view(torch.int32).fill_(NAN_BITS)
    return pts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def grow_and_check(pts, depth, c2w, bound, dev, radius_add=RADIUS, thin=None, pixels=None, stride=1, rho=(0.0,),
                   init=None):
    """One add_frame on `pts`, compared with the teacher-forced restatement in every output."""
    n = pts.n_points
    x0, f0 = pts.xyz.cpu().numpy().copy(), pts.feats.detach().cpu().numpy().copy()
    n_new = pts.add_frame(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY, CX, CY, bound,
                          pixels=None if pixels is None else torch.as_tensor(pixels), stride=stride, rho=rho,
                          radius_add=radius_add, thin=thin, init_feats=None if init is None else init.to(dev),
                          return_candidates=True)
    cx, cf = (t.cpu().numpy() for t in pts.last_candidates)
    ref = G.add_frame(x0, f0, n, depth, c2w, FX, FY, CX, CY, bound, pts.origin, radius_add, thin, pixels, stride, rho,
                      None if init is None else init.numpy(), cand_xyz=cx)
    la = pts.last_add
    print('counters', la)
    assert np.array_equal(cf, ref['flags'])
    assert [la['candidates'], la['valid'], la['free'], la['survivors'], la['dropped']] == ref['counters']
    assert n_new == ref['n_new'] == la['added'] and pts.n_points == n + n_new
    # old rows, appended rows and the rows beyond them, all as bits
    assert np.array_equal(bits(pts.xyz.cpu().numpy()), bits(ref['xyz']))
    assert np.array_equal(bits(pts.feats.detach().cpu().numpy()), bits(ref['feats']))
    return ref


def test_candidate_positions(pnr_mod, dev):
    """cand_xyz against the float64 back-projection.  Roundings on the path, each at its worst: the
    direction (division, product, two sums: 4 u on sum_b |R_ab d_b|), the depth (1 + rho, its product:
    2 u), rd z (u) and the final sum (u on |p_a| <= |t_a| + sum_b |R_ab d_b| z): 8 u in all."""
    bound, c2w = scene()
    depth = frame_depth(special=False)
    pts = make_cloud(pnr_mod, dev, torch.zeros((0, 3)), None, 16, bound)
    pts.add_frame(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY, CX, CY, bound,
                  rho=RHO3, return_candidates=True)
    got = pts.last_candidates[0].cpu().numpy().astype(np.float64)
    assert got.shape == (3 * H * W, 3)
    p64, _ = G.candidates(depth, c2w, FX, FY, CX, CY, rho=RHO3, dtype=np.float64)
    u_, v_, _ = G.candidate_pixels(H, W)
    dirs = np.stack([(u_ - CX) / FX, -(v_ - CY) / FY, -np.ones(u_.shape)], -1)               # (P, 3)
    S = (np.abs(c2w[:3, :3].astype(np.float64))[None, :, :] * np.abs(dirs)[:, None, :]).sum(-1)  # (P, 3)
    z = depth.reshape(-1).astype(np.float64)[:, None] * (1.0 + np.asarray(RHO3, np.float32).astype(np.float64))[None, :]
    lim = 8 * 2.0 ** -24 * (np.abs(c2w[:3, 3].astype(np.float64))[None, None, :] + S[:, None, :] * z[:, :, None])
    err = np.abs(got - p64).reshape(H * W, 3, 3)
    print('worst |p - p64| / bound', float((err / lim).max()))
    assert (err <= lim).all()
    own, _ = G.candidates(depth, c2w, FX, FY, CX, CY, rho=RHO3)
    print('bitwise equal to the float32 restatement:', bool(np.array_equal(bits(got.astype(np.float32)), bits(own))))


@pytest.fixture(scope='module')
def base_case():
    """The 3,000-point random cloud in the room0 bound and the frame that cuts through it."""
    bound, c2w = scene()
    xyz, feats = random_cloud(bound)
    return bound, c2w, xyz, feats, frame_depth()


def test_decisions_exact(pnr_mod, dev, base_case):
    bound, c2w, xyz, feats, depth = base_case
    n = xyz.shape[0]
    # the case itself, on the restatement's own positions: every outcome is well represented
    origin = (bound[:, 0] - 0.06 * 1.004).astype(np.float32)
    own = G.add_frame(np.concatenate([xyz.numpy(), np.zeros((9216, 3), np.float32)]), np.zeros((n + 9216, 32), np.float32),
                      n, depth, c2w, FX, FY, CX, CY, bound, origin, RADIUS, 0.02, rho=RHO3)
    c = own['counters']
    assert c[0] == 9216
    for share in (c[1], c[0] - c[1], c[1] - c[2], c[2] - c[3], c[3]):  # valid, invalid, near, thinned, surviving
        assert share >= 0.05 * c[0], c
    pts = make_cloud(pnr_mod, dev, xyz, feats, n + 9216, bound)
    init = torch.randn((9216, 32), generator=torch.Generator().manual_seed(8))
    ref = grow_and_check(pts, depth, c2w, bound, dev, thin=0.02, rho=RHO3, init=init)
    assert abs(ref['counters'][3] - c[3]) <= 0.02 * c[3]  # the forced run is the same case


PERM = np.random.default_rng(5).permutation(H * W)
SIZE_CASES = {
    'cand0': dict(pixels=np.zeros(0, np.int64)),
    'all_invalid': dict(depth='zeros'),
    'cand1': dict(pixels=PERM[3:4]),   # (a pixel whose candidate survives)
    'cand63': dict(pixels=PERM[:63]),
    'cand1025': dict(pixels=PERM[:1025]),
    # past the one-block scan, in descending order, with repeats and two indices outside the image
    'cand4097_desc_repeats': dict(pixels=np.concatenate([np.sort(np.concatenate([PERM, PERM[:1023]]))[::-1],
                                                         [-1, H * W]]).astype(np.int64)),
    'cand9216': dict(rho=RHO3),
    'empty_cloud': dict(empty=True, rho=RHO3),
    'thin0': dict(thin=0.0, rho=RHO3),
    'thin_tiny_full_table': dict(thin=1e-4, pixels=PERM[:1024], empty=True, depth='plain'),
    'thin_huge': dict(thin=10.0),
    'stride3': dict(stride=3, rho=(0.0, 0.01)),
}


@pytest.mark.parametrize('name', list(SIZE_CASES))
def test_sizes_and_paths(pnr_mod, dev, base_case, name):
    bound, c2w, xyz, feats, depth = base_case
    case = dict(SIZE_CASES[name])
    if case.pop('empty', False):
        xyz, feats = torch.zeros((0, 3)), None
    dsel = case.pop('depth', None)
    if dsel == 'zeros':
        depth = np.zeros_like(depth)
    elif dsel == 'plain':
        depth = np.full_like(depth, 0.3)
    pts = make_cloud(pnr_mod, dev, xyz, feats, xyz.shape[0] + 9300, bound)
    ref = grow_and_check(pts, depth, c2w, bound, dev, **case)
    c = ref['counters']
    if name == 'cand0':
        assert c == [0, 0, 0, 0, 0]
    elif name == 'all_invalid':
        assert c == [H * W, 0, 0, 0, 0]
    elif name == 'cand4097_desc_repeats':
        assert c[0] == 4097 and c[3] > 0
    elif name == 'thin_tiny_full_table':  # 1,024 voxels in the 2,048-entry table: its minimum size, half full
        assert c == [1024, 1024, 1024, 1024, 0]
    elif name == 'thin_huge':             # one voxel holds them all: the first free candidate survives
        assert c[2] > 100 and c[3] == 1
        first = int(np.nonzero(ref['flags'] & G.FREE)[0][0])
        assert np.array_equal(bits(pts.xyz[xyz.shape[0]].cpu().numpy()), bits(ref['cand_xyz'][first]))
    elif name == 'thin0':
        assert c[3] == c[2] > 0
    elif name == 'stride3':
        assert c[0] == 16 * 22 * 2 and c[3] > 0
    elif name == 'cand1':
        assert c == [1, 1, 1, 1, 0]
    else:
        assert c[0] == { 'cand63': 63, 'cand1025': 1025, 'cand9216': 9216, 'empty_cloud': 9216}[name]
    if name in ('cand9216', 'empty_cloud'):  # invalid depths and points outside the bound are both present
        d = np.repeat(depth.reshape(-1), 3)
        assert (~np.isfinite(d)).any() and (d <= 0).any()
        assert ((ref['flags'] & G.VALID) == 0)[np.isfinite(d) & (d > 0)].any()
        assert c[3] > 0


def test_capacity_clip(pnr_mod, dev, base_case):
    bound, c2w, xyz, feats, depth = base_case
    n = xyz.shape[0]
    pts = make_cloud(pnr_mod, dev, xyz, feats, n + 10, bound)
    ref = grow_and_check(pts, depth, c2w, bound, dev)
    c = ref['counters']
    assert c[3] > 10 and c[4] == c[3] - 10 and pts.n_points == n + 10
    kept = np.nonzero(ref['flags'] & G.KEPT)[0][:10]   # the first 10 in candidate order
    assert np.array_equal(bits(pts.xyz[n:].cpu().numpy()), bits(ref['cand_xyz'][kept]))
    ref2 = grow_and_check(pts, depth, c2w, bound, dev)  # full: adds nothing, writes nothing
    assert ref2['n_new'] == 0 and ref2['counters'][4] == ref2['counters'][3] and pts.n_points == n + 10


def test_determinism(pnr_mod, dev, base_case):
    bound, c2w, xyz, feats, depth = base_case
    out = []
    for _ in range(2):
        pts = make_cloud(pnr_mod, dev, xyz, feats, xyz.shape[0] + 9216, bound)
        pts.add_frame(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY, CX, CY, bound,
                      rho=RHO3, thin=0.02)
        out.append((pts.xyz.view(torch.int32).clone(), pts.feats.data.view(torch.int32).clone(), dict(pts.last_add)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def raw_gather(pnr, pts, q):
    lib = pnr.library()
    P, dev = q.shape[0], q.device
    c = torch.empty((P, 32), device=dev)
    idx = torch.empty((P, pts.k), device=dev, dtype=torch.int32)
    w = torch.empty((P, pts.k), device=dev)
    s, _ = pts.descriptor()
    ws = torch.empty(lib.pnr_point_gather_workspace_bytes(P), dtype=torch.uint8, device=dev)
    assert lib.pnr_point_gather(ctypes.byref(s), q.data_ptr(), P, c.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    return c, idx, w


@pytest.mark.parametrize('feat_dtype', ['float32', 'float16'])
def test_grown_cloud_is_an_ordinary_cloud(pnr_mod, dev, base_case, feat_dtype):
    bound, c2w, xyz, feats, depth = base_case
    n0 = xyz.shape[0]
    pts = make_cloud(pnr_mod, dev, xyz, feats, n0 + 4000, bound, feat_dtype=feat_dtype)
    gen = torch.Generator().manual_seed(21)
    q0 = (xyz[torch.randint(0, n0, (512,), generator=gen)] + 0.02 * torch.randn((512, 3), generator=gen)).double()
    raw_gather(pnr_mod, pts, q0.to(dev))   # (the float16 feature copy exists before the cloud grows)
    added = []
    for k, rho in enumerate(((0.0,), RHO3)):
        d = frame_depth(seed=k)
        init = 0.5 * torch.randn((H * W * len(rho), 32), generator=gen)
        n = pts.n_points
        pts.add_frame(torch.from_numpy(d).to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY, CX, CY, bound, rho=rho,
                      thin=0.02, init_feats=init.to(dev))
        added.append(pts.n_points - n)
    n = pts.n_points
    assert min(added) > 50
    direct = pnr_mod.NeuralPoints(pts.xyz[:n].clone(), pts.feats.data[:n].clone(), mode='idw', k=8, radius=RADIUS,
                                  cell=pts.cell, origin=pts.origin, table_bits=pts.table_bits,
                                  feat_dtype=feat_dtype).to(dev)
    new = pts.xyz[n0:n].cpu()
    q = torch.cat([q0, (new[torch.randint(0, n - n0, (1536,), generator=gen)]
                        + 0.01 * torch.randn((1536, 3), generator=gen)).double()]).to(dev)
    (c, idx, w), (c_d, idx_d, w_d) = raw_gather(pnr_mod, pts, q), raw_gather(pnr_mod, direct, q)
    assert torch.equal(idx, idx_d) and torch.equal(w.view(torch.int32), w_d.view(torch.int32))
    assert torch.equal(c.view(torch.int32), c_d.view(torch.int32))
    only_new = (idx >= n0).any(1) & ((idx >= n0) | (idx < 0)).all(1)
    assert only_new.sum() > 100 and (c[only_new].abs().sum(1) > 0).all()  # the new rows' initial features are seen


def map_setup(pnr, dev, n=256):
    from test_gpu_points import make_renderer, surface_cloud
    from oracle import ref_points as RP
    ro, rd, gt, xyz, feats = surface_cloud(dev)
    gen = torch.Generator().manual_seed(17)
    batches = [(ro[:n].to(dev), rd[:n].to(dev), gt[:n].to(dev), torch.rand((n, 3), generator=gen).to(dev),
                torch.rand((n, 32), generator=gen).to(dev)) for _ in range(3)]
    params = RP.init_fc_c(golden_params('trained'), seed=1)
    bound, c2w = scene()
    # the frame to grow from, and a batch of its own rays (gt = its depth): their samples meet the new points
    depth = frame_depth(special=False)
    pix = torch.from_numpy(np.random.default_rng(9).permutation(H * 54)[:n])
    u, v = (pix % 54), (pix // 54)                      # the image's left part: inside the room
    fro, frd = pnr.get_rays_from_uv(u.float().to(dev), v.float().to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY,
                                    CX, CY, dev)
    fgt = torch.from_numpy(depth)[v, u].to(dev)
    fbatch = (fro.reshape(-1, 3).float().contiguous(), frd.reshape(-1, 3).float().contiguous(), fgt,
              torch.rand((n, 3), generator=gen).to(dev), torch.rand((n, 32), generator=gen).to(dev))

    def make(capacity):
        dec = pnr.MLP(name='color', dim=3, c_dim=32, color=True, skips=[], n_blocks=4, hidden_size=256)
        dec.load_state_dict({k: t.clone() for k, t in params.items()})
        kw = dict(mode='idw', radius=0.04, k=8, cell=0.0804, origin=[-0.5, -0.5, -0.5], table_bits=12)
        f = feats.to(dev)
        if capacity:
            f = torch.cat([f, torch.full((capacity - f.shape[0], 32), 0.37, device=dev)])
            pts = pnr.NeuralPoints(xyz.to(dev), feats.to(dev), capacity=capacity, **kw).to(dev)
            with torch.no_grad():
                pts.feats.data.copy_(f)  # the rows that are not live hold a value Adam must leave alone
        else:
            pts = pnr.NeuralPoints(xyz.to(dev), f, **kw).to(dev)
        return make_renderer(pnr, torch.from_numpy(bound)), dec.to(dev), pts
    return make, batches, fbatch, (depth, c2w, bound), xyz.shape[0]


def test_map_step_over_capacity_cloud(pnr_mod, dev):
    from pnr.mapping import MapStep
    make, batches, fbatch, (depth, c2w, bound), M = map_setup(pnr_mod, dev)
    steps = []
    for capacity in (None, M + 4096):
        r, dec, pts = make(capacity)
        ms = MapStep(r, dec, points=pts, feat_lr=1e-2)
        assert ms.renderer.precision == 'f16x3'
        loss = float(ms(*batches[0]))
        torch.cuda.synchronize()
        steps.append((loss, ms.flat.grad.clone(), ms.flat.data.clone(), ms, pts))
    (l_a, g_a, w_a, _, _), (l_b, g_b, w_b, ms, pts) = steps
    nd, live = ms.n_dec, ms.n_dec + M * 32
    assert l_a == l_b
    assert torch.equal(g_a[:nd], g_b[:nd]) and torch.equal(g_a[nd:], g_b[nd:live])   # decoder, live rows
    assert torch.equal(w_a[:nd], w_b[:nd]) and torch.equal(w_a[nd:], w_b[nd:live])
    assert g_a[nd:].abs().sum() > 0
    assert not g_b[live:].any()                                                        # dead rows: no gradient,
    assert torch.equal(w_b[live:], torch.full_like(w_b[live:], 0.37))                  # and the same bits
    # grow, then step on the frame's own rays
    n_new = pts.add_frame(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY, CX, CY, bound,
                          radius_add=0.02, thin=0.02)
    assert n_new > 100 and pts.n_points == M + n_new
    loss = float(ms(*fbatch))
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    g_new = ms.flat.grad[live:live + n_new * 32].reshape(n_new, 32)
    print('new rows with gradient:', int((g_new != 0).any(1).sum()), 'of', n_new)
    assert torch.isfinite(ms.flat.grad).all() and (g_new != 0).any(1).sum() > 20
    assert not ms.flat.grad[live + n_new * 32:].any()


def test_map_graph_after_growth(pnr_mod, dev):
    """A captured step holds the cloud's size and index by value: replaying it after add_frame raises; a
    new graph over the grown cloud replays what the eager step computes, bit for bit."""
    from pnr.mapping import MapGraph, MapStep
    make, batches, fbatch, (depth, c2w, bound), M = map_setup(pnr_mod, dev)
    runs = []
    for graph in (False, True):
        r, dec, pts = make(M + 4096)
        ms = MapStep(r, dec, points=pts, feat_lr=1e-2)
        ms.opt.use_device_step()
        old = MapGraph(ms, *batches[0], warmup=1)
        assert pts.add_frame(torch.from_numpy(depth).to(dev), torch.from_numpy(c2w).to(dev), H, W, FX, FY, CX, CY, bound,
                             radius_add=0.02, thin=0.02) > 100
        with pytest.raises(RuntimeError):
            old(*batches[0])
        losses = []
        if graph:
            mg = MapGraph(ms, *fbatch, warmup=2)
            for b in batches[1:]:
                losses.append(float(mg(*b)))
        else:
            for _ in range(2):
                ms(*fbatch)
            for b in batches[1:]:
                losses.append(float(ms(*b)))
        torch.cuda.synchronize()
        runs.append((losses, ms.flat.data.detach().cpu().clone(), int(ms.opt.step_dev[0].item())))
    (l_e, w_e, s_e), (l_g, w_g, s_g) = runs
    assert s_e == s_g == 5 and all(np.isfinite(l_e))
    assert l_g == l_e, (l_g, l_e)
    assert torch.equal(w_g, w_e)
