"""Every decoder precision held to the float64 split-operand model, layer by layer (tests/split_model.py).

Through the raw C ABI (pnr_mlp_fwd_train[_c], pnr_eval_points*, pnr_mlp_bwd[_c]), for precision in
{fp32, bf16, bf16x3, f16x3} and both decoder forms (the reference decoder; c_dim = 32 with the feature
branch), at point counts that take every tile form: 1, 63 (under one 64-point tile of the 4-wave f16x3
forward), 129 (one point in a second 128-row segment), 128 * 3 + 37, and -- reference decoder only --
2 * 128 * CUs + 37, where every persistent workgroup takes a second tile and f16x3 runs its 8-wave form.

Forward: the workspace is filled with 0xFF bytes (NaN activations, all-ones masks) before the call.  Each
layer's model is evaluated on the kernel's OWN saved input of that layer, so the only difference a
correct kernel leaves is its fp32 accumulation order: saved h_l against relu(z_l) (+ f_l), the saved mask
bit against [z_l > 0] wherever |z_l| is beyond the bound (the undecided share capped at EDGE_CAP, a
condition tests/test_split_model.py shows on the model alone), raw_out against the model's output layer
on the saved h4, all at BOUND_ULPS u M; the padding rows of the save area hold the finite activations of
x = 0.  The large case models the first tile, one tile of the second sweep and the ragged last tile.

Eval entry points: the per-point arithmetic is the training kernel's, so their outputs are bitwise the
training call's; with a bound, channel 3 is exactly 100 on the rows the float64 / float32 comparison
puts outside (a point on a face is outside) and every other value is bitwise unchanged.

Backward: on the save area its own forward wrote, into gradients pre-filled with a known pattern (the
call accumulates), every element of (gradient - pre-fill) and of dL/dp (dL/dc) within split_model
.grad_bound of the float64 gradient formed from the saved activations and the kernel's own mask bits: no
flip allowance, the biases as tensors of their own.  (rtol 1e-3 cannot see a lost split term of the
backward GEMMs: split_model's docstring.)  Every non-fp32 precision shares the delta chain and the
weight-gradient GEMMs and the save layout does not depend on the precision: on one save area the
backward called with bf16x3 and bf16 gives bitwise the gradients of the call with f16x3.
"""
import ctypes

import pytest
import torch

import split_model as SM
from conftest import golden_params, load_golden
from oracle import ref_points as RP

pytestmark = pytest.mark.gpu

DEC = ['embedder._B'] + [f'pts_linears.{i}.{w}' for i in range(4) for w in ('weight', 'bias')] + \
      ['output_linear.weight', 'output_linear.bias']
FC = [f'fc_c.{i}.{w}' for i in range(4) for w in ('weight', 'bias')]
RAGGED = 128 * 3 + 37
COUNTS = {False: (1, 63, 129, RAGGED, 'two-sweeps'), True: (1, 63, 129, RAGGED)}
CASES = [(prec, feat, P) for prec in SM.PRECISIONS for feat in (False, True) for P in COUNTS[feat]]


def _id(case):
    return f'{case[0]}-{"c32" if case[1] else "reference"}-{case[2]}'


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


class Env:
    """The library, the trained decoder (+ fc_c) on the device and its packed images."""

    def __init__(self, dev):
        from pnr import _lib
        self.L, self.lib, self.dev = _lib, _lib.load(), dev
        self.st = _lib.stream_of(dev)
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.bound = torch.from_numpy(load_golden('scene.npz')['bound'])
        self.params = {k: v.to(dev).contiguous() for k, v in RP.init_fc_c(golden_params('trained'), seed=3).items()}
        self.packed = torch.empty(self.lib.pnr_mlp_packed_floats(), device=dev)
        self.fcp = torch.empty(self.lib.pnr_fc_packed_floats(), device=dev)
        _lib.check(self.lib.pnr_mlp_pack(_lib.PtrArray(*[self.params[k].data_ptr() for k in DEC]),
                                         _lib.ptr(self.packed), self.st), 'mlp_pack')
        _lib.check(self.lib.pnr_fc_pack(_lib.FcPtrArray(*[self.params[k].data_ptr() for k in FC]),
                                        _lib.ptr(self.fcp), self.st), 'fc_pack')
        torch.cuda.synchronize()

    def count(self, P):
        return 2 * 128 * self.cus + 37 if P == 'two-sweeps' else P

    def fwd_train(self, prec, x, c):
        """pnr_mlp_fwd_train[_c] into a workspace of 0xFF bytes: (raw, ws)."""
        L, lib, P = self.L, self.lib, x.shape[0]
        ws = torch.full((lib.pnr_mlp_train_workspace_bytes(P),), 0xFF, dtype=torch.uint8, device=self.dev)
        raw = torch.full((P, 4), float('nan'), device=self.dev)
        code = L.precision_code(prec)
        if c is None:
            L.check(lib.pnr_mlp_fwd_train(L.ptr(self.packed), L.ptr(x), P, L.ptr(raw), L.ptr(ws), ws.numel(), code,
                                          self.st), 'mlp_fwd_train')
        else:
            L.check(lib.pnr_mlp_fwd_train_c(L.ptr(self.packed), L.ptr(self.fcp), L.ptr(x), L.ptr(c), P, L.ptr(raw),
                                            L.ptr(ws), ws.numel(), code, self.st), 'mlp_fwd_train_c')
        torch.cuda.synchronize()
        return raw, ws

    def eval(self, prec, entry, pts, c, bound6=None):
        """pnr_eval_points ('f64'), pnr_eval_points_f32 ('f32') or pnr_eval_points_c ('c', float64 points)."""
        L, lib, P = self.L, self.lib, pts.shape[0]
        raw = torch.full((P, 4), float('nan'), device=self.dev)
        b = None if bound6 is None else (ctypes.c_double * 6)(*bound6)
        code = L.precision_code(prec)
        assert pts.dtype == (torch.float32 if entry == 'f32' else torch.float64) and pts.is_contiguous()
        if entry == 'c':
            L.check(lib.pnr_eval_points_c(L.ptr(self.packed), L.ptr(self.fcp), L.ptr(pts), L.ptr(c), P, b, L.ptr(raw),
                                          code, self.st), 'eval_points_c')
        else:
            fn = lib.pnr_eval_points if entry == 'f64' else lib.pnr_eval_points_f32
            L.check(fn(L.ptr(self.packed), L.ptr(pts), P, b, L.ptr(raw), code, self.st), 'eval_points')
        torch.cuda.synchronize()
        return raw

    def bwd(self, prec, P, ws, g_raw, c, prefill):
        """pnr_mlp_bwd[_c] on the save area `ws`, the gradients starting from `prefill` (name -> tensor) and
        the backward scratch from 0xFF bytes: ({name: gradient}, g_p, g_c)."""
        L, lib = self.L, self.lib
        names = DEC + (FC if c is not None else [])
        grads = {k: prefill[k].clone() for k in names}
        g_p = torch.full((P, 3), float('nan'), device=self.dev)
        code = L.precision_code(prec)
        arr = L.PtrArray(*[grads[k].data_ptr() for k in DEC])
        if c is None:
            bws = torch.full((lib.pnr_mlp_bwd_workspace_bytes(P),), 0xFF, dtype=torch.uint8, device=self.dev)
            g_c = None
            L.check(lib.pnr_mlp_bwd(L.ptr(self.packed), P, L.ptr(g_raw), arr, L.ptr(g_p), L.ptr(ws), ws.numel(),
                                    L.ptr(bws), bws.numel(), code, self.st), 'mlp_bwd')
        else:
            bws = torch.full((lib.pnr_mlp_bwd_workspace_bytes_c(P),), 0xFF, dtype=torch.uint8, device=self.dev)
            g_c = torch.full((P, SM.C_DIM), float('nan'), device=self.dev)
            farr = L.FcPtrArray(*[grads[k].data_ptr() for k in FC])
            L.check(lib.pnr_mlp_bwd_c(L.ptr(self.packed), L.ptr(self.fcp), L.ptr(c), P, L.ptr(g_raw), arr, farr,
                                      L.ptr(g_c), L.ptr(g_p), L.ptr(ws), ws.numel(), L.ptr(bws), bws.numel(), code,
                                      self.st), 'mlp_bwd_c')
        torch.cuda.synchronize()
        return grads, g_p, g_c


@pytest.fixture(scope='module')
def env(dev):
    return Env(dev)


class Run:
    """One training forward: its inputs, raw output and decoded save area."""

    def __init__(self, env, prec, feat, P):
        self.prec, self.feat, self.P = prec, feat, P
        self.x = SM.room_points(env.bound, P).to(env.dev)
        self.c = SM.room_features(P).to(env.dev) if feat else None
        self.raw, self.ws = env.fwd_train(prec, self.x, self.c)
        self.sv = SM.decode_save(self.ws, P)
        ld = self.sv['ld']
        if ld <= 1024:
            self.rows = torch.arange(ld, device=env.dev)
        else:  # first tile, one tile of the second sweep, the ragged last tile with its padding
            assert P == 2 * 128 * env.cus + 37
            self.rows = torch.cat([torch.arange(0, 128), torch.arange(128 * env.cus, 128 * env.cus + 128),
                                   torch.arange(2 * 128 * env.cus, ld)]).to(env.dev)
        assert self.rows.numel() <= 512


@pytest.fixture(scope='module', params=CASES, ids=_id)
def run(request, env):
    prec, feat, P = request.param
    return Run(env, prec, feat, env.count(P))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_forward_layers(env, run):
    prm, sv, prec, P, rows = env.params, run.sv, run.prec, run.P, run.rows
    ld, real = sv['ld'], run.rows < run.P
    tag = f'{prec} {"c32" if run.feat else "reference"} P={P}'
    # padding rows: zero inputs, finite activations; no NaN left anywhere in the rows of real points
    assert torch.equal(sv['x'][P:], torch.zeros_like(sv['x'][P:])), 'padding rows of x are zero'
    assert torch.equal(sv['x'][:P, :3], run.x) and bool((sv['x'][:P, 3] == 1).all())
    assert bool(torch.isfinite(sv['h']).all()), 'every row of h1..h4, padding included, was written'
    assert bool(torch.isfinite(run.raw).all())
    x = sv['x'][rows, :3].contiguous()
    c_all = None
    if run.feat:  # the kernels read zero features for the rows past P
        c_all = torch.zeros((ld, SM.C_DIM), device=env.dev)
        c_all[:P] = run.c
    for li in range(4):
        W, b = prm[f'pts_linears.{li}.weight'], prm[f'pts_linears.{li}.bias']
        T = 0.0
        if li == 0 and prec == 'fp32':  # the fp32 forward saves e: first e itself, then layer 0 from it
            assert bool(torch.isfinite(sv['e']).all())
            _, e64, de = SM.fourier(x, prm['embedder._B'])
            e = sv['e'][rows]
            r = float(((e[:, :SM.N_FOURIER].double() - e64).abs() / de).max())
            print(f'{tag} e: worst |e - sin| / de = {r:.3f}')
            assert r <= 1.0 and bool((e[:, SM.N_FOURIER:] == 0).all())
            z, M = SM.layer(W, b, e[:, :SM.N_FOURIER].contiguous(), prec)
        elif li == 0:
            z, M, T = SM.layer0(W, b, x, prm['embedder._B'], prec)
        else:
            z, M = SM.layer(W, b, sv['h'][li - 1][rows], prec)
        tol = SM.BOUND_ULPS * SM.U32 * M + T
        hv, tol_h = torch.relu(z), tol
        if run.feat:
            f, Mf = SM.feature_term(prm[f'fc_c.{li}.weight'], prm[f'fc_c.{li}.bias'], c_all, prec)
            hv, tol_h = hv + f[rows], tol + SM.BOUND_ULPS * SM.U32 * Mf[rows]
        r = float(((sv['h'][li][rows].double() - hv).abs() / tol_h).max())
        print(f'{tag} layer {li}: worst |h - model| / bound = {r:.4f} (= {r * SM.BOUND_ULPS:.2f} u M)')
        assert r <= 1.0, f'{tag}: saved h{li + 1} against the model'
        edge = z.abs() <= tol
        share = float(edge[real].double().mean())
        wrong = (sv['masks'][li][rows] != (z > 0)) & ~edge
        print(f'{tag} layer {li}: undecided share {share:.1e}, mask bits differing off the edge {int(wrong.sum())}')
        assert share <= SM.EDGE_CAP
        assert not bool(wrong.any()), f'{tag}: ReLU mask bits of layer {li}'
    zo, Mo = SM.output(prm['output_linear.weight'], prm['output_linear.bias'], sv['h'][3][rows[real]], prec, run.feat)
    r = float(((run.raw[rows[real]].double() - zo).abs() / (SM.BOUND_ULPS * SM.U32 * Mo)).max())
    print(f'{tag} output: worst |raw - model| / bound = {r:.4f} (= {r * SM.BOUND_ULPS:.2f} u M)')
    assert r <= 1.0, f'{tag}: raw_out against the model'


def test_eval_is_the_training_arithmetic(env, run):
    """pnr_eval_points / _f32 (no bound) and pnr_eval_points_c return bitwise the training call's raw_out."""
    if run.feat:
        got = {'pnr_eval_points_c': env.eval(run.prec, 'c', run.x.double(), run.c)}
    else:
        got = {'pnr_eval_points_f32': env.eval(run.prec, 'f32', run.x, None),
               'pnr_eval_points': env.eval(run.prec, 'f64', run.x.double(), None)}
    for name, raw in got.items():
        n = int((_bits(raw) != _bits(run.raw)).sum())
        print(f'{run.prec} P={run.P} {name}: {n} of {raw.numel()} values differ from the training forward')
        assert n == 0, name


def _prefill(ref, names, dev):
    """A known non-zero start of every gradient: +-{1, 2, 3} 2^k with 2^k <= max|g| / 8 (exact in fp32,
    so (result - prefill) loses at most 2 u max|g|, far inside the bound's atol term)."""
    out = {}
    for k in names:
        g = ref[k][0]
        s = 2.0 ** torch.floor(torch.log2(g.abs().max().clamp(min=1e-30) / 8))
        i = torch.arange(g.numel(), device=dev)
        out[k] = (s * (1 + i % 3) * (1 - 2 * (i % 2))).float().view(g.shape).contiguous()
    return out


def _g_raw(P, dev):
    return torch.randn((P, 4), generator=torch.Generator().manual_seed(23 + P), dtype=torch.float64).float().to(dev)


def test_backward(env, run):
    prm, sv, P = env.params, run.sv, run.P
    tag = f'{run.prec} {"c32" if run.feat else "reference"} P={P}'
    g_raw = _g_raw(P, env.dev)
    assert bool((g_raw[:, 3] != 0).all())
    last = {}
    ref = SM.backward(prm, sv['x'][:P, :3].contiguous(), [sv['h'][l][:P] for l in range(4)], sv['masks'][:, :P], g_raw,
                      run.c, last_sum=last)
    names = DEC + (FC if run.feat else [])
    pre = _prefill(ref, names, env.dev)
    grads, g_p, g_c = env.bwd(run.prec, P, run.ws, g_raw, run.c, pre)
    got = {k: grads[k].double() - pre[k].double() for k in names}
    got['x'] = g_p.double()
    if run.feat:
        got['c'] = g_c.double()
    worst = {}
    for k, t in got.items():
        g, M = ref[k]
        assert bool(torch.isfinite(t).all()), f'{tag}: {k} is finite'
        worst[k] = float(((t - g).abs() / SM.grad_bound(g, M)).max())
    print(f'{tag} backward, worst |g - model| / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    print(f'{tag} backward, for information, against the last sum\'s magnitude alone: ' + ', '.join(
        f'{k} {float(((got[k] - ref[k][0]).abs() / SM.grad_bound(ref[k][0], M)).max()):.3f}' for k, M in last.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f'{tag}: gradients beyond the bound: {bad}'


@pytest.mark.parametrize('feat', [False, True], ids=['reference', 'c32'])
def test_backward_dispatch_is_one_kernel_set(env, feat):
    """bf16x3 and bf16 run the f16x3 delta chain and weight-gradient GEMMs on the same save layout."""
    P = RAGGED
    x = SM.room_points(env.bound, P).to(env.dev)
    c = SM.room_features(P).to(env.dev) if feat else None
    _, ws = env.fwd_train('f16x3', x, c)
    g_raw = _g_raw(P, env.dev)
    names = DEC + (FC if feat else [])
    shapes = {k: env.params[k].shape for k in names}
    pre = {k: torch.full(tuple(s), 0.25, device=env.dev) for k, s in shapes.items()}
    want = env.bwd('f16x3', P, ws, g_raw, c, pre)
    assert all(bool(torch.isfinite(t).all()) and not torch.equal(t, pre[k]) for k, t in want[0].items())
    for prec in ('bf16x3', 'bf16'):
        got = env.bwd(prec, P, ws, g_raw, c, pre)
        for k in names:
            assert torch.equal(_bits(got[0][k]), _bits(want[0][k])), f'{prec}: {k}'
        assert torch.equal(_bits(got[1]), _bits(want[1])), f'{prec}: dL/dp'
        if feat:
            assert torch.equal(_bits(got[2]), _bits(want[2])), f'{prec}: dL/dc'


@pytest.mark.parametrize('prec', SM.PRECISIONS)
def test_eval_bound_mask(env, prec):
    """With a bound: channel 3 is exactly 100 on the rows outside (float64 comparison for float64 points,
    float32 for float32 points; strict, so a point on a face is outside), everything else bitwise the
    unbounded call's."""
    P, b = RAGGED, env.bound
    q = SM.room_points(b, P).double()
    q[0, 0] = b[0, 1]                                                   # on the upper x face
    q[1, 1] = b[1, 0]                                                   # on the lower y face
    q[2, 2] = torch.nextafter(b[2, 1], torch.tensor(-1.0, dtype=torch.float64))  # inside in float64 only
    q[3, 0] = b[0, 1] + 0.1                                             # outside
    q[4, 0] = b[0, 0].float().double()                                  # the float32 face value
    q[5, 1] = torch.nextafter(b[1, 0].float(), torch.tensor(1.0)).double()  # one float32 step inside
    q[130, 2] = b[2, 0] - 1e-9
    q[P - 1, 0] = b[0, 1]                                               # a face point in the ragged last tile
    p32 = q.float()
    out64 = ~((q < b[:, 1]) & (q > b[:, 0])).all(1)
    b32 = b.float()
    out32 = ~((p32 < b32[:, 1]) & (p32 > b32[:, 0])).all(1)
    assert bool(out64[0]) and bool(out64[1]) and not bool(out64[2]) and bool(out32[2]) and bool(out64[P - 1])
    assert 4 <= int(out64.sum()) <= 8 and 4 <= int(out32.sum()) <= 8
    c = SM.room_features(P).to(env.dev)
    bound6 = [float(v) for v in b.reshape(-1)]
    for entry, pts, outside in (('f64', q, out64), ('f32', p32, out32), ('c', q, out64)):
        pts = pts.to(env.dev).contiguous()
        cc = c if entry == 'c' else None
        free = env.eval(prec, entry, pts, cc)
        got = env.eval(prec, entry, pts, cc, bound6)
        want = free.clone()
        want[outside.to(env.dev), 3] = 100.0
        assert bool(torch.isfinite(free).all()) and not bool((free[:, 3] == 100.0).any())
        assert torch.equal(_bits(got), _bits(want)), f'{prec} {entry}'
