"""The float64 split-operand model of tests/split_model.py, checked on the CPU: its parts and scales, its
save-area decode, its backward against autograd -- and that the bound the GPU test
(tests/test_gpu_decoder_layers.py) asserts CAN fail: every mutant of the model (a lost cross term, a
weight scale whose inverse does not match, a truncated lo part) leaves BOUND_ULPS u M on the very inputs
the GPU test uses, while the share of ReLU pre-activations too close to zero to decide stays under the
cap the GPU test relies on."""
import numpy as np
import pytest
import torch

import split_model as SM
from conftest import golden_params, load_golden
from oracle import ref_points as RP

CUS = 256  # the MI355X; the GPU test takes the count from the device
POINT_COUNTS = (1, 63, 129, 128 * 3 + 37)


@pytest.fixture(scope='module')
def params():
    return RP.init_fc_c(golden_params('trained'), seed=3)


@pytest.fixture(scope='module')
def bound():
    return torch.from_numpy(load_golden('scene.npz')['bound'])


def test_parts_reproduce_the_value():
    g = torch.Generator().manual_seed(1)
    x = torch.exp(torch.rand(20000, generator=g, dtype=torch.float64) * np.log(60000 / 0.125) + np.log(0.125))
    x = (x * torch.sign(torch.rand(20000, generator=g, dtype=torch.float64) - 0.5)).float()
    for prec, rel in (('fp32', 0.0), ('bf16', 2.0 ** -8), ('bf16x3', 2.0 ** -16), ('f16x3', 2.0 ** -22)):
        p = SM.parts(x, prec)
        assert len(p) == (2 if prec.endswith('x3') else 1)
        err = ((sum(p) - x.double()).abs() / x.double().abs()).max()
        print(f'{prec}: max |sum(parts) - x| / |x| = {float(err):.3e} (bound {rel:.3e})')
        assert float(err) <= rel
    # every part is a value of its 16-bit format
    for prec, fmt in (('bf16x3', torch.bfloat16), ('f16x3', torch.float16)):
        for q in SM.parts(x, prec):
            assert torch.equal(q.float().to(fmt).double(), q)


def test_weight_scale_rule(params):
    # the two cases tests/test_gpu_step_tail.py pins for the packer, the clamps and the binade edges
    assert SM.weight_scale(torch.zeros(4, 4)) == 2.0 ** 20
    assert SM.weight_scale(torch.tensor([[3.0, -100.0], [0.5, 7.0]])) == 2.0 ** 7
    assert SM.weight_scale(torch.tensor([1.0])) == 2.0 ** 14
    assert SM.weight_scale(torch.tensor([1.0000001])) == 2.0 ** 13
    assert SM.weight_scale(torch.tensor([1e-9])) == 2.0 ** 20
    assert SM.weight_scale(torch.tensor([1e12])) == 2.0 ** -20
    for k, W in params.items():
        if k.endswith('weight'):
            s = SM.weight_scale(W)
            assert 2.0 ** 13 < float(W.abs().max()) * s <= 2.0 ** 14, k


def test_row_scale_is_wave_uniform():
    c = torch.zeros(70, 32)
    c[3, 5], c[40, 0], c[41, 1] = 0.1, -3.0, 1e-4
    s = SM.row_scale(c)
    assert s.shape == (70, 1)
    assert torch.all(s[:32] == 2.0 ** 17) and torch.all(s[32:64] == 2.0 ** 12) and torch.all(s[64:] == 1.0)


def test_decode_save_bit_mapping():
    """The mask decode against the forward's own statement of where a bit goes (csrc/mlp16.h conv1: unit
    32 t + perm(r, hh) of the lane's point is bit 16 (t & 1) + r of word t >> 1, perm = (r & 3) + 8 (r >> 2)
    + 4 hh), written out as plain loops over a synthetic workspace."""
    P, ld = 200, 256
    g = torch.Generator().manual_seed(2)
    want = torch.rand((4, ld, 256), generator=g) < 0.5
    ws = torch.zeros((96 + 4 * 256) * 4 * ld + 16 * ld + 128 * ld, dtype=torch.uint8)
    off = (96 + 4 * 256) * 4 * ld + 16 * ld
    words = np.zeros((4, ld // 32, 64, 4), dtype=np.uint32)
    w_np = want.numpy()
    for t in range(8):
        for r in range(16):
            for hh in range(2):
                u = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh
                for j in range(32):
                    sel = w_np[:, j::32, u][:, :ld // 32]  # (4, groups): point 32 g + j
                    words[:, :, 32 * hh + j, t >> 1] |= sel.astype(np.uint32) << np.uint32(16 * (t & 1) + r)
    ws[off:] = torch.from_numpy(words.view(np.uint8).reshape(-1))
    x = torch.arange(ld * 4, dtype=torch.float32).view(ld, 4)
    ws[off - 16 * ld:off] = x.view(-1).view(torch.uint8)
    sv = SM.decode_save(ws, P)
    assert sv['ld'] == ld and sv['e'].shape == (ld, 96) and sv['h'].shape == (4, ld, 256)
    assert torch.equal(sv['x'], x)
    assert torch.equal(sv['masks'], want)


def test_backward_matches_autograd(params):
    """split_model.backward is the gradient of the decoder: float64 autograd on the same activations."""
    P = 37
    x = SM.room_points(torch.tensor([[-1.0, 1.0]] * 3), P, seed=5)
    c = SM.room_features(P, seed=5)
    g_raw = torch.randn((P, 4), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for feat in (False, True):
        p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
        xd, cd = x.double().requires_grad_(True), c.double().requires_grad_(True)
        h, hs, ms = torch.sin(xd @ p64['embedder._B']), [], []
        for li in range(4):
            z = h @ p64[f'pts_linears.{li}.weight'].t() + p64[f'pts_linears.{li}.bias']
            ms.append(z.detach() > 0)
            h = torch.relu(z)
            if feat:
                h = h + cd @ p64[f'fc_c.{li}.weight'].t() + p64[f'fc_c.{li}.bias']
            hs.append(h.detach())
        raw = h @ p64['output_linear.weight'].t() + p64['output_linear.bias']
        (raw * g_raw).sum().backward()
        got = SM.backward(params, x, hs, torch.stack(ms), g_raw, c if feat else None)
        want = {k: v.grad for k, v in p64.items() if feat or not k.startswith('fc_c')}
        want['x'] = xd.grad
        if feat:
            want['c'] = cd.grad
        assert set(got) == set(want)
        for k, w in want.items():
            gk, Mk = got[k]
            # (the model forms the Fourier argument in fp32, as the kernels do: 1e-6-class differences)
            np.testing.assert_allclose(gk.numpy(), w.numpy(), rtol=1e-5, atol=1e-5 * float(w.abs().max()), err_msg=k)
            assert Mk.shape == gk.shape and bool((Mk >= gk.abs() * (1 - 1e-12)).all()), k


def _trunc_lo(x32, prec):
    """parts() with the lo part truncated towards zero instead of rounded (a mutant)."""
    hi = x32.to(torch.bfloat16).float()
    lo = ((x32 - hi).view(torch.int32) & -65536).view(torch.float32)
    return [hi.double(), lo.double()]


MUTANTS = [
    ('bf16x3', 'no Wl.xh', dict(terms=(1, 2))),
    ('bf16x3', 'no Wh.xl', dict(terms=(0, 2))),
    ('f16x3', 'no Wl.xh', dict(terms=(1, 2))),
    ('f16x3', 'no Wh.xl', dict(terms=(0, 2))),
    ('f16x3', 'scale one binade up, inverse not', 'scale'),
    ('bf16x3', 'lo truncated', dict(split=_trunc_lo)),
]


@pytest.mark.parametrize('prec,what,mut', MUTANTS, ids=[f'{m[0]}-{m[1].replace(" ", "_")}' for m in MUTANTS])
def test_model_mutants_leave_the_bound(params, bound, prec, what, mut):
    """On the GPU test's inputs (trained weights, 421 points in the room0 bound) a mutant of one hidden
    layer, fed the true model's input of that layer, moves at least one element beyond BOUND_ULPS u M: the
    GPU assertion would catch a kernel with that defect."""
    P = POINT_COUNTS[-1]
    x = SM.room_points(bound, P)
    layers, _ = SM.forward(params, x, prec)
    worst = []
    for li in range(1, 4):
        W, b = params[f'pts_linears.{li}.weight'], params[f'pts_linears.{li}.bias']
        kw = dict(scale=2 * SM.weight_scale(W), inv=1 / SM.weight_scale(W)) if mut == 'scale' else mut
        zm, _ = SM.layer(W, b, layers[li - 1]['h'], prec, **kw)
        worst.append(float(((zm - layers[li]['z']).abs() / (SM.BOUND_ULPS * SM.U32 * layers[li]['M'])).max()))
    print(f'{prec}, {what}: worst |z_mutant - z| / (64 u M) per layer 1..3 = ' + ', '.join(f'{w:.1f}' for w in worst))
    assert max(worst) > 1.0


@pytest.mark.parametrize('prec', SM.PRECISIONS)
def test_accumulation_order_stays_inside_the_bound(params, bound, prec):
    """The other side of the mutants: the same products accumulated in fp32 in 16-deep chunks (an MFMA-like
    blocked order) stay well inside BOUND_ULPS u M of the float64 model."""
    x = SM.room_points(bound, POINT_COUNTS[-1])
    layers, _ = SM.forward(params, x, prec)
    for li in range(1, 4):
        W, b = params[f'pts_linears.{li}.weight'], params[f'pts_linears.{li}.bias']
        s = SM.weight_scale(W) if prec == 'f16x3' else 1.0
        Wp, xp = SM.parts(W * s, prec), SM.parts(layers[li - 1]['h'], prec)
        prods = [(Wp[1], xp[0]), (Wp[0], xp[1]), (Wp[0], xp[0])] if len(Wp) == 2 else [(Wp[0], xp[0])]
        acc = torch.zeros((x.shape[0], 256), dtype=torch.float32)
        for k0 in range(0, 256, 16):
            for wa, xb in prods:
                acc = (acc.double() + xb[:, k0:k0 + 16] @ wa[:, k0:k0 + 16].t()).float()
        z32 = ((acc.double() / s).float().double() + b.double()).float().double()
        r = float(((z32 - layers[li]['z']).abs() / (SM.U32 * layers[li]['M'])).max())
        print(f'{prec} layer {li}: fp32 16-deep accumulation within {r:.2f} u M of the float64 model')
        assert r < SM.BOUND_ULPS / 4


@pytest.mark.parametrize('feat', [False, True], ids=['reference', 'c32'])
@pytest.mark.parametrize('prec', SM.PRECISIONS)
def test_edge_share_under_the_cap(params, bound, prec, feat):
    """The condition the GPU test's mask comparison rests on, shown on the reference alone: for its
    points (every point count, and the rows its large case models on a 256-CU device) at most EDGE_CAP of a
    layer's pre-activations lie within the bound of zero."""
    counts = POINT_COUNTS if feat else POINT_COUNTS + (2 * 128 * CUS + 37,)
    for P in counts:
        x = SM.room_points(bound, P)
        c = SM.room_features(P) if feat else None
        if P > 1024:  # the rows the GPU test models: first tile, one tile of the second sweep, the ragged tail
            rows = torch.cat([torch.arange(0, 128), torch.arange(128 * CUS, 128 * CUS + 128),
                              torch.arange(2 * 128 * CUS, P)])
            x = x[rows]
        layers, _ = SM.forward(params, x, prec, c)
        shares = [SM.edge_share(L['z'], L['M'], L['T']) for L in layers]
        print(f'{prec} {"c32" if feat else "reference"} P={P}: edge share per layer ' +
              ', '.join(f'{s:.1e}' for s in shares))
        assert max(shares) <= SM.EDGE_CAP
