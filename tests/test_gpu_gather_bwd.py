"""pnr_point_gather_bwd through the raw C ABI, held to its contract (include/pnr.h).

Feature gradient: bit for bit the fixed-point model tests/gather_bwd_model.py (int32 views compared with
torch.equal), in the sparse and the dense accumulator path, at the guard boundaries P = 2^n, with unused
neighbour slots, with the guard's worst case (one row named by every sample, same-sign terms), in any
row order, at the half-wave run lengths 2 / 4 / 16, and with a non-finite dL/dc.  Every call starts from
a workspace of 0xFF bytes, dL/dp filled with NaN and a known non-zero g_feats (+-{1,2,3} 2^k, the
pattern of tests/test_gpu_decoder_layers.py, no -0.0), so `+=`, "rows no sample names stay untouched"
and stale workspace contents are all observed.  The index / weight / c rows come from pnr_point_gather
on the same points (the forward is pinned in tests/test_gpu_points.py): the backward is teacher-forced.

dL/dp: every row written; elementwise against the float64 gradient on the kernel's own neighbour rows
with the bound of tests/test_gpu_points.py (rtol 1e-3, atol 1e-6, MAG_ULPS = 64 of the summation
magnitude), for IDW and for trilinear weights (samples on lattice planes and points: sign(d) = 0),
samples exactly on a cloud point (the d <= eps skip) and float16 features.
"""
import ctypes
import math

import pytest
import torch

import gather_bwd_model as GM
from oracle import ref_points as RP
from test_gpu_points import _gather_c_abi, grad_elementwise, idw_grad_p_cr, random_cloud

pytestmark = pytest.mark.gpu

E_WORKSPACE = -2


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


# ---- the launcher's branches, as the header / csrc/points.hip state them (asserted per case, so a case
# ---- that no longer reaches its branch says so) -------------------------------------------------
def is_sparse(P, k, M):
    return P * k < 4 * M


def run_length(P):
    run = 32
    while run > 2 and P // run < 2 * 5 * 1024 * 8:
        run >>= 1
    return run


# ---- inputs ---------------------------------------------------------------------------------------
def ray_samples(xyz, P, seed, device='cpu', S=10, spread=0.01, half_len=0.03):
    """P samples along short rays through the cloud (consecutive rows share neighbours); every 7th ray
    lies far outside it: rows without any neighbour.  float32-representable float64."""
    gen = torch.Generator(device=device).manual_seed(seed)
    n_rays = (P + S - 1) // S
    x = xyz.to(device)
    o = x[torch.randint(0, x.shape[0], (n_rays,), generator=gen, device=device)] + \
        spread * torch.randn((n_rays, 3), generator=gen, device=device)
    d = torch.nn.functional.normalize(torch.randn((n_rays, 3), generator=gen, device=device), dim=1)
    t = torch.linspace(-half_len, half_len, S, device=device)
    q = o[:, None, :] + t[None, :, None] * d[:, None, :]
    q[torch.arange(n_rays, device=device) % 7 == 3] += 10.0
    return q.reshape(-1, 3)[:P].float().double().contiguous()


def randn_rows(P, seed, device='cpu'):
    return torch.randn((P, 32), generator=torch.Generator(device=device).manual_seed(seed), device=device)


def scaled_rows(P, seed):
    """Per-row scales 2^U(-30, 0) and one row in ten all zero."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn((P, 32), generator=gen) * 2.0 ** (-30.0 * torch.rand((P, 1), generator=gen))
    g[torch.rand(P, generator=gen) < 0.1] = 0.0
    return g.float()


def prefill(M, g_c, dev):
    """+-{1, 2, 3} 2^k with 2^k <= max |dL/dc| / 8 (the finite entries), exact in float32, no -0.0."""
    fin = g_c[torch.isfinite(g_c)]
    gm = float(fin.abs().max()) if fin.numel() else 0.0
    s = 2.0 ** math.floor(math.log2(gm / 8)) if gm > 0 else 0.125
    i = torch.arange(M * 32, device=dev)
    return (s * (1 + i % 3) * (1 - 2 * (i % 2))).float().view(M, 32).contiguous()


def make_points(pnr, dev, xyz, feats, **kw):
    return pnr.NeuralPoints(xyz.to(dev), feats.to(dev), **kw).to(dev)


def lattice(n=12, h=1.0 / 16):
    """n^3 points on a dyadic lattice (spacing h) in a random index order, features N(0, 0.5)."""
    gen = torch.Generator().manual_seed(41)
    ii = torch.stack(torch.meshgrid(torch.arange(n), torch.arange(n), torch.arange(n), indexing='ij'), -1).reshape(-1, 3)
    xyz = ii[torch.randperm(ii.shape[0], generator=gen)].float() * h
    return xyz, torch.randn((xyz.shape[0], 32), generator=gen) * 0.5, h


# ---- one call ---------------------------------------------------------------------------------------
def backward(pnr, pts, q, idx, w, c, g_c, g_feats, want_gp=True, short=0):
    """pnr_point_gather_bwd on a poisoned workspace.  Returns (rc, g_p, atomics or None, ws)."""
    lib = pnr.library()
    dev = q.device
    P = q.shape[0]
    s, keep = pts.descriptor(g_feats=g_feats)
    nbytes = lib.pnr_point_gather_bwd_workspace_bytes(ctypes.byref(s), P)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    g_p = torch.full((P, 3), float('nan'), device=dev) if want_gp else None
    ptr = pnr._lib.ptr
    rc = lib.pnr_point_gather_bwd(ctypes.byref(s), ptr(q), P, ptr(idx), ptr(w), ptr(c), ptr(g_c), ptr(g_p), ptr(ws),
                                  nbytes - short, None)
    torch.cuda.synchronize()
    n = None
    if rc == 0 and g_feats is not None:
        n_at = ctypes.c_int64(-1)
        assert lib.pnr_point_gather_bwd_atomics(ctypes.byref(s), ptr(ws), P, ctypes.byref(n_at), None) == 0
        n = n_at.value
    return rc, g_p, n, ws


def run_case(pnr, pts, q, g_c, tag, model_device='cpu', fwd=None):
    """Forward (teacher), backward with both outputs, and every assertion shared by the cases: g_feats
    bit for bit the model, unnamed rows bit for bit the prefill, the atomics count, dL/dp written."""
    dev = q.device
    c, idx, w = fwd if fwd is not None else _gather_c_abi(pnr, dev, pts, q, pts.k)
    M = pts.n_points
    g_c = g_c.to(dev).contiguous()
    pre = prefill(M, g_c, dev)
    g_feats = pre.clone()
    rc, g_p, n, _ = backward(pnr, pts, q, idx, w, c, g_c, g_feats)
    assert rc == 0, tag
    md = torch.device(model_device)
    exp, info = GM.gather_bwd_feats(idx.to(md), w.to(md), g_c.to(md), pre.to(md))
    got = g_feats.to(md)
    named = info['named']
    if info['s'] is not None:
        diff = got.view(torch.int32) != exp.view(torch.int32)
        print(f'{tag}: P {q.shape[0]} guard {info["guard"]} s {info["s"]} slots {info["slots"]} named rows '
              f'{int(named.sum())} / {M}, atomics {n}, elements off the model: {int(diff.sum())}')
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), f'{tag}: g_feats is not the model\'s bit pattern'
    else:
        print(f'{tag}: non-finite max |dL/dc|, named rows {int(named.sum())} / {M}')
        assert bool(torch.isnan(got[named]).all()), f'{tag}: NaN on every named row'
        assert GM.same_bits(got, exp), f'{tag}: NaN exactly on the named rows'
    assert torch.equal(got[~named].view(torch.int32), pre.to(md)[~named].view(torch.int32)), \
        f'{tag}: rows no sample names are the prefill, bit for bit'
    if info['slots'] > 0:
        assert 0 < n <= info['slots'], f'{tag}: {n} atomic instructions for {info["slots"]} neighbour slots'
    else:
        assert n == 0, tag
    finite_rows = torch.isfinite(g_c).all(1)  # (a row's own non-finite dL/dc reaches its own dL/dp)
    assert not bool(torch.isnan(g_p[finite_rows]).any()), f'{tag}: every dL/dp row written'
    assert bool((g_p[idx[:, 0] < 0] == 0).all()), f'{tag}: dL/dp is zero on rows without neighbours'
    return dict(c=c, idx=idx, w=w, g_c=g_c, pre=pre, g_feats=g_feats, g_p=g_p, info=info, n=n)


@pytest.fixture(scope='module')
def cloud():
    xyz, feats, _ = random_cloud(3000, seed=3)
    return xyz, feats


# ---- feature gradient: bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 63, 1000, 1023, 1024, 1025, 1500, 4096])
def test_feats_bits_sparse_dense_and_guard_boundaries(pnr_mod, dev, cloud, P):
    """M = 3000, k = 8, IDW.  P k < 4 M selects the sparse accumulators (P < 1500), P = 1500 sits exactly
    on the threshold (dense), 4096 is dense; the guard changes at P = 1024; every P but 1024 and 4096
    leaves a ragged tail of the work list's half-wave runs."""
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    assert is_sparse(P, 8, 3000) == (P < 1500) and run_length(P) == 2
    assert GM.guard_bits(P) == {1: 1, 63: 6, 1000: 10, 1023: 10, 1024: 11, 1025: 11, 1500: 11, 4096: 13}[P]
    q = ray_samples(xyz, P, seed=100 + P).to(dev)
    r = run_case(pnr_mod, pts, q, randn_rows(P, 200 + P), f'idw k=8 P={P}')
    assert r['info']['slots'] > 0
    if P >= 63:
        assert bool((r['idx'][:, 0] < 0).any()) and not bool(r['info']['named'].all())


@pytest.mark.parametrize('k', [1, 3])
def test_feats_bits_fewer_neighbour_slots(pnr_mod, dev, cloud, k):
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=k)
    q = ray_samples(xyz, 1000, seed=300 + k).to(dev)
    r = run_case(pnr_mod, pts, q, randn_rows(1000, 310 + k), f'idw k={k}')
    assert r['info']['slots'] > 500


@pytest.mark.parametrize('P', [500, 2000])
def test_feats_bits_trilinear_lattice(pnr_mod, dev, P):
    """Trilinear weights over a 12^3 lattice (k = 8): samples inside cells (8 neighbours), sparse and dense."""
    xyz, feats, h = lattice()
    pts = make_points(pnr_mod, dev, xyz, feats, mode='trilinear', k=8, radius=h, spacing=[h] * 3)
    assert is_sparse(P, 8, xyz.shape[0]) == (P == 500)
    q = ray_samples(xyz, P, seed=400 + P, spread=0.02).to(dev)
    r = run_case(pnr_mod, pts, q, randn_rows(P, 410 + P), f'trilinear P={P}')
    assert bool((r['idx'][:, 7] >= 0).any()), 'samples with all 8 cell corners'


@pytest.mark.parametrize('P', [1000, 4096])
def test_feats_bits_wide_range_and_zero_rows(pnr_mod, dev, cloud, P):
    """dL/dc rows scaled by 2^U(-30, 0), one in ten all zero: terms far below the largest one (those under
    2^(23 - s) are the ones the rounding to a multiple of 2^-s changes).  Once on the non-zero prefill and
    once from g_feats = 0, as the autograd wrapper calls it: there the feature rows that only small-scale
    samples name show every bit of their sum."""
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    q = ray_samples(xyz, P, seed=500 + P).to(dev)
    g_c = scaled_rows(P, 510 + P)
    r = run_case(pnr_mod, pts, q, g_c, f'scaled rows P={P}')
    info = r['info']
    g0 = torch.zeros_like(r['pre'])
    rc, _, _, _ = backward(pnr_mod, pts, q, r['idx'], r['w'], r['c'], r['g_c'], g0)
    assert rc == 0
    exp, _ = GM.gather_bwd_feats(r['idx'].cpu(), r['w'].cpu(), r['g_c'].cpu(), torch.zeros(g0.shape))
    small = (info['acc'].abs() < 2 ** 23) & (info['acc'] != 0)
    print(f'from zero: {int(small.sum())} elements whose whole sum is below 2^23 units of 2^-s')
    if P == 1000:  # (sparse: most feature rows are named by one or two samples)
        assert int(small.sum()) > 0, 'the case must hold elements that show the rounding of single terms'
    assert torch.equal(g0.cpu().view(torch.int32), exp.view(torch.int32)), 'g_feats from zero is the model\'s bit pattern'


def test_zero_gradient_and_empty_work_list(pnr_mod, dev, cloud):
    """max |dL/dc| = 0 (s = 0, zero terms), and a batch in which no sample has a neighbour (an empty work
    list; dL/dc and even a NaN in it are then irrelevant): g_feats stays the prefill, dL/dp is zero."""
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    for P in (1000, 4096):
        q = ray_samples(xyz, P, seed=600 + P).to(dev)
        r = run_case(pnr_mod, pts, q, torch.zeros((P, 32)), f'zero dL/dc P={P}')
        assert r['info']['gmax'] == 0.0 and r['info']['slots'] > 0
        assert torch.equal(r['g_feats'].view(torch.int32), r['pre'].view(torch.int32))
        assert bool((r['g_p'] == 0).all())
        g_c = randn_rows(P, 610 + P)
        g_c[5, 3] = float('nan')
        r = run_case(pnr_mod, pts, (q + 10.0).contiguous(), g_c, f'no neighbours P={P}')
        assert r['info']['slots'] == 0 and r['n'] == 0
        assert torch.equal(r['g_feats'].view(torch.int32), r['pre'].view(torch.int32))
        assert bool((r['g_p'] == 0).all())


@pytest.mark.parametrize('sign', [1.0, -1.0])
@pytest.mark.parametrize('P', [1023, 1024, 4096])
def test_feats_bits_one_hot_point(pnr_mod, dev, P, sign):
    """The guard's worst case: k = 1, every sample within the radius of ONE point (weight exactly 1),
    dL/dc = the float32 just below 2 everywhere: P same-sign terms of nearly 2^(62 - guard) units in each
    element of one row.  257 points: sparse for P = 1023 and 1024 (guards 10 and 11), dense for 4096."""
    gen = torch.Generator().manual_seed(7)
    xyz, feats, _ = random_cloud(256, seed=8)
    hot = torch.tensor([[2.0, 2.0, 2.0]])
    xyz, feats = torch.cat([xyz, hot]), torch.cat([feats, torch.randn((1, 32), generator=gen)])
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=1)
    assert is_sparse(P, 1, 257) == (P < 4096)
    q = (hot + 0.04 * (torch.rand((P, 3), generator=gen) - 0.5)).float().double().to(dev)
    fwd = _gather_c_abi(pnr_mod, dev, pts, q, 1)
    assert bool((fwd[1] == 256).all()), 'every sample names the hot point'
    assert bool((fwd[2] <= 1.0).all()) and bool((fwd[2] >= 1.0 - 2.0 ** -22).all()), 'with weight 1 (to rounding)'
    g1 = float(torch.tensor(1.9999999))
    assert g1 == 2.0 - 2.0 ** -23
    r = run_case(pnr_mod, pts, q, torch.full((P, 32), sign * g1), f'hot point P={P} sign={sign:+.0f}', fwd=fwd)
    info = r['info']
    assert info['s'] == 62 - info['guard'] - 1 and int(info['named'].sum()) == 1
    total = info['acc'][256].tolist()
    assert total == [total[0]] * 32 and total[0] * sign > 0
    assert P * 2 ** (61 - info['guard']) <= abs(total[0]) < 2 ** 62, 'the sum fills the guard bits'


@pytest.mark.parametrize('P', [1000, 4096])
def test_row_order_gives_equal_bits(pnr_mod, dev, cloud, P):
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    q = ray_samples(xyz, P, seed=700 + P).to(dev)
    g_c = randn_rows(P, 710 + P)
    a = run_case(pnr_mod, pts, q, g_c, f'ray order P={P}')
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(3))
    pd = perm.to(dev)
    fwd = tuple(t[pd].contiguous() for t in (a['c'], a['idx'], a['w']))
    b = run_case(pnr_mod, pts, q[pd].contiguous(), g_c[perm], f'random order P={P}', fwd=fwd)
    assert torch.equal(a['g_feats'].view(torch.int32), b['g_feats'].view(torch.int32))
    assert torch.equal(a['g_p'][pd].view(torch.int32), b['g_p'].view(torch.int32)), 'dL/dp rows are independent'


@pytest.mark.parametrize('P', [327_680, 1_310_720])
def test_feats_bits_longer_half_wave_runs(pnr_mod, dev, cloud, P):
    """Ray-ordered batches at which the launcher takes 4- and 16-row half-wave runs (the carry of a
    neighbour shared with the previous row spans more rows); the model runs on the device, slot by slot."""
    xyz, feats = cloud
    assert run_length(P) == {327_680: 4, 1_310_720: 16}[P] and run_length(P - 1) == run_length(P) // 2
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    q = ray_samples(xyz, P, seed=800, device=dev, S=32)
    g_c = randn_rows(P, 801, device=dev)
    r = run_case(pnr_mod, pts, q, g_c, f'run {run_length(P)} P={P}', model_device=dev)
    idx = r['idx']
    rows = idx[idx[:, 0] >= 0]
    shared = ((rows[1:, :, None] == rows[:-1, None, :]) & (rows[1:, :, None] >= 0)).any(2).sum().item()
    print(f'neighbour slots shared with the previous row: {shared} of {r["info"]["slots"]}')
    assert shared > r['info']['slots'] // 4, 'consecutive rows must share neighbours (the carry path)'
    assert r['n'] < r['info']['slots'], 'carried partial sums save atomics'


@pytest.mark.parametrize('bad', [float('nan'), float('-inf')])
@pytest.mark.parametrize('P', [1000, 4096])
def test_non_finite_gradient_marks_exactly_the_named_rows(pnr_mod, dev, cloud, P, bad):
    """A non-finite dL/dc in a row WITHOUT neighbours has no effect at all (the result is the finite
    call's, bit for bit); in a row WITH neighbours every row some sample names becomes NaN and every other
    row keeps the prefill -- in the sparse call (P = 1000) and in the dense one (P = 4096), which converts
    every row."""
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    assert is_sparse(P, 8, 3000) == (P == 1000)
    q = ray_samples(xyz, P, seed=900 + P).to(dev)
    g_c = randn_rows(P, 910 + P)
    ref = run_case(pnr_mod, pts, q, g_c, f'finite P={P}')
    fwd = (ref['c'], ref['idx'], ref['w'])
    has = (ref['idx'][:, 0] >= 0).cpu()
    g1 = g_c.clone()
    g1[int(torch.nonzero(~has)[-1]), 31] = bad
    r1 = run_case(pnr_mod, pts, q, g1, f'{bad} in a row without neighbours P={P}', fwd=fwd)
    assert math.isfinite(r1['info']['gmax'])
    assert torch.equal(r1['g_feats'].view(torch.int32), ref['g_feats'].view(torch.int32))
    assert torch.equal(r1['g_p'].view(torch.int32), ref['g_p'].view(torch.int32))
    g2 = g_c.clone()
    g2[int(torch.nonzero(has)[-1]), 0] = bad
    r2 = run_case(pnr_mod, pts, q, g2, f'{bad} in a row with neighbours P={P}', fwd=fwd)
    named = r2['info']['named'].to(dev)
    assert r2['info']['s'] is None and 0 < int(named.sum()) < 3000
    assert bool(torch.isnan(r2['g_feats'][named]).all())
    assert torch.equal(r2['g_feats'][~named].view(torch.int32), r2['pre'][~named].view(torch.int32))


# ---- dL/dp ------------------------------------------------------------------------------------------
def trilinear_grad_p_cr(p, xyz, feats, idx, gc, spacing):
    """d(sum c(p) . gc)/dp of the trilinear gather, c = sum_k wn_k f_k with w_k = prod_a (1 - |d_a| / h_a),
    in float64 on a fixed neighbour set, and each component's summation magnitude M: the sum over k of
    |wn_k / (h_a t_ka)| (|g.f_k| + sum_j wn_j |g.f_j|) with |g.f| summed in absolute values."""
    p = p.clone().requires_grad_(True)
    sp = torch.as_tensor(spacing, dtype=torch.float64)
    valid = idx >= 0
    ic = idx.clamp(min=0)
    dl = p[:, None, :] - xyz[ic]
    t = 1.0 - dl.abs() / sp
    w = torch.where(valid, t.prod(-1), torch.zeros_like(t[..., 0]))
    W = w.sum(1)
    W = torch.where(W > 0, W, torch.ones_like(W))
    wn = w / W[:, None]
    fk = feats[ic]
    c = (wn[:, :, None] * fk).sum(1)
    (c * gc).sum().backward()
    with torch.no_grad():
        gabs = torch.where(valid, (fk.abs() * gc.abs()[:, None, :]).sum(-1), torch.zeros_like(w))
        a = gabs + (wn * gabs).sum(1, keepdim=True)
        dw = torch.where(valid[..., None] & (dl != 0), wn[..., None] / (sp * t), torch.zeros_like(dl))
        mag = (dw.abs() * a[..., None]).sum(1)
    return p.grad.detach(), mag.numpy()


def oracle_f32_grad_p(q, xyz, feats, idx, gc, mode, spacing=None):
    """The oracle's float32 gather (RP.neighbour_weights, sequential sums) on the given neighbour rows."""
    qr = q.clone().requires_grad_(True)
    wn = RP.neighbour_weights(qr, xyz, idx, mode, spacing, 1e-6)
    fk = feats.float()[idx.clamp(min=0)]
    c = torch.zeros((q.shape[0], 32))
    for j in range(idx.shape[1]):
        c = c + wn[:, j:j + 1] * fk[:, j]
    (c * gc).sum().backward()
    return qr.grad


def dp_case(pnr, dev, pts, xyz, feats_read, q, tag, spacing=None):
    """Both outputs on a poisoned call, then dL/dp elementwise; feats_read = the features the kernel reads."""
    P = q.shape[0]
    r = run_case(pnr, pts, q.to(dev), randn_rows(P, 1000 + P), tag)
    idx = r['idx'].cpu().long()
    gc = r['g_c'].cpu()
    if pts.mode == 'idw':
        gcr, mag = idw_grad_p_cr(q.float().double(), xyz.double(), feats_read.double(), idx, gc.double())
    else:
        gcr, mag = trilinear_grad_p_cr(q.float().double(), xyz.double(), feats_read.double(), idx, gc.double(), spacing)
    g32 = oracle_f32_grad_p(q, xyz, feats_read, idx, gc, pts.mode, spacing)
    assert bool(torch.isfinite(gcr).all()) and float(gcr.abs().max()) > 0
    grad_elementwise(r['g_p'], gcr, g32, f'dL/dp {tag}', mag=mag)
    return r


@pytest.mark.parametrize('k', [3, 8])
def test_grad_p_idw(pnr_mod, dev, cloud, k):
    """Rays through the cloud plus 64 samples exactly ON a cloud point: that neighbour's distance is 0 <=
    eps, so its own term is skipped and only the normalisation carries its weight."""
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=k)
    q = torch.cat([ray_samples(xyz, 1000, seed=1100 + k), xyz[100:164].double()])
    r = dp_case(pnr_mod, dev, pts, xyz, feats, q, f'idw k={k}')
    on = r['idx'][1000:, 0].cpu()
    assert torch.equal(on, torch.arange(100, 164, dtype=torch.int32)), 'the point itself is the nearest neighbour'
    assert bool((r['idx'][1000:, 1] >= 0).any()), 'and it has further neighbours'


def test_grad_p_idw_f16_features(pnr_mod, dev, cloud):
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8, feat_dtype='float16')
    q = torch.cat([ray_samples(xyz, 1000, seed=1200), xyz[200:232].double()])
    dp_case(pnr_mod, dev, pts, xyz, feats.half().float(), q, 'idw f16 features')


def test_grad_p_trilinear(pnr_mod, dev):
    """Samples inside cells, exactly on a lattice plane (d_a = 0 for four corners: sign 0) and exactly on a
    lattice point (one neighbour with weight 1)."""
    xyz, feats, h = lattice()
    pts = make_points(pnr_mod, dev, xyz, feats, mode='trilinear', k=8, radius=h, spacing=[h] * 3)
    gen = torch.Generator().manual_seed(43)
    inside = ray_samples(xyz, 700, seed=1300, spread=0.02)
    plane = (2 + 8 * torch.rand((200, 3), generator=gen)) * h
    plane[:, 1] = torch.randint(2, 10, (200,), generator=gen).float() * h
    point = torch.randint(2, 10, (100, 3), generator=gen).float() * h
    q = torch.cat([inside, plane.float().double(), point.double()])
    r = dp_case(pnr_mod, dev, pts, xyz, feats, q, 'trilinear', spacing=[h] * 3)
    nb = (r['idx'] >= 0).sum(1).cpu()
    assert bool((nb[700:900] == 4).all()), 'a sample on a lattice plane has the 4 corners of its face'
    assert bool((nb[900:] == 1).all()) and bool((r['w'][900:, 0] == 1.0).all()), 'a sample on a lattice point has that point'
    assert bool((r['g_p'][900:] == 0).all()), 'and no gradient: sign(0) = 0 on every axis'
    assert bool((r['g_p'][700:900, 1] == 0).all()), 'no gradient across the plane a sample lies on'


# ---- output forms -------------------------------------------------------------------------------------
def test_output_forms(pnr_mod, dev, cloud):
    xyz, feats = cloud
    pts = make_points(pnr_mod, dev, xyz, feats, mode='idw', radius=0.06, k=8)
    P = 1000
    q = ray_samples(xyz, P, seed=1400).to(dev)
    both = run_case(pnr_mod, pts, q, randn_rows(P, 1401), 'both outputs')
    args = (both['idx'], both['w'], both['c'], both['g_c'])
    # g_feats only
    gf = both['pre'].clone()
    rc, g_p, n, _ = backward(pnr_mod, pts, q, *args, gf, want_gp=False)
    assert rc == 0 and g_p is None and 0 < n <= both['info']['slots']
    assert torch.equal(gf.view(torch.int32), both['g_feats'].view(torch.int32))
    # dL/dp only
    rc, g_p, _, _ = backward(pnr_mod, pts, q, *args, None)
    assert rc == 0
    assert torch.equal(g_p.view(torch.int32), both['g_p'].view(torch.int32))
    # neither: nothing is touched
    rc, _, _, ws = backward(pnr_mod, pts, q, *args, None, want_gp=False)
    assert rc == 0 and bool((ws == 0xFF).all())
    # a workspace one byte short
    gf = both['pre'].clone()
    rc, g_p, _, ws = backward(pnr_mod, pts, q, *args, gf, short=1)
    assert rc == E_WORKSPACE
    assert torch.equal(gf.view(torch.int32), both['pre'].view(torch.int32)) and bool(torch.isnan(g_p).all())
    assert bool((ws == 0xFF).all())
