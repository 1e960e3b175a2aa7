"""tests/gather_bwd_model.py on its own (no GPU): the fixed-point model of the gather backward's feature
gradient against a float64 scatter within the header's bound, its independence of the row order, the
guard's worst case without int64 overflow, and the contract's edges (unnamed rows, NaN, all zero)."""
import math
from fractions import Fraction

import pytest
import torch

import gather_bwd_model as GM


def synthetic(P, M, k, seed, p_none=0.2):
    """Index / weight rows shaped like the gather's: distinct ids per row, nearest first, -1 padded,
    normalised weights; some rows without any neighbour."""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(M, generator=gen)[:k] for _ in range(P)]).int()
    n_nb = torch.randint(1, k + 1, (P,), generator=gen)
    n_nb[torch.rand(P, generator=gen) < p_none] = 0
    idx[torch.arange(k)[None, :] >= n_nb[:, None]] = -1
    w = torch.rand((P, k), generator=gen) + 0.05
    w[idx < 0] = 0
    w = w / w.sum(1, keepdim=True).clamp(min=1e-30)
    g = torch.randn((P, 32), generator=gen) * 2.0 ** torch.randint(-30, 1, (P, 1), generator=gen).float()
    return idx, w.float(), g.float()


def test_guard_bits():
    assert [GM.guard_bits(P) for P in (0, 1, 2, 3, 4, 1023, 1024, 1025)] == [1, 1, 2, 2, 3, 10, 11, 11]
    assert GM.guard_bits(2 ** 31 - 1) == 31
    assert GM.guard_bits(2 ** 45) == 40


def test_shift():
    assert GM.shift_of(0.0, 5) == 0
    assert GM.shift_of(1.0, 1) == 62 - 1 - 1        # 1.0 = 0.5 x 2^1
    assert GM.shift_of(0.75, 11) == 62 - 11 - 0
    assert GM.shift_of(2.0 ** -30, 3) == 62 - 3 + 29


def test_terms_round_half_even_after_a_float32_product():
    # s = 1: multiples of 1/2 are exact, quarters tie to even
    w = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0])
    g = torch.tensor([0.25, 0.75, 1.25, -0.25, -0.75])[:, None].expand(-1, 32).contiguous()
    assert GM.terms(w, g, 1)[:, 0].tolist() == [0, 2, 2, 0, -2]
    # the product rounds to float32 BEFORE the scaling: (1 + 2^-12)^2 loses its 2^-24 bit
    x = torch.tensor([1.0 + 2.0 ** -12])
    T = GM.terms(x, x[:, None].expand(-1, 32).contiguous(), 30)
    assert int(T[0, 0]) == (1 << 30) + (1 << 19)
    # s > 127 (a float32 ldexp would overflow its scale factor)
    T = GM.terms(torch.tensor([1.0]), torch.full((1, 32), 2.0 ** -100), 150)
    assert int(T[0, 0]) == 1 << 50


@pytest.mark.parametrize('P,M,k', [(1000, 300, 8), (257, 40, 3), (64, 5, 1)])
def test_model_against_float64_scatter(P, M, k):
    """|acc 2^-s - sum of the float32 products in float64| <= (term count) x 2^-(63 - guard) x max |dL/dc|
    (the header's bound; one more float64 ulp of the sum's magnitude for the float64 scatter's own
    rounding), and the result is prefill + that, rounded to float32 twice."""
    idx, w, g = synthetic(P, M, k, seed=P)
    pre = torch.zeros((M, 32))
    out, info = GM.gather_bwd_feats(idx, w, g, pre)
    assert info['guard'] == GM.guard_bits(P) and info['s'] == GM.shift_of(info['gmax'], info['guard'])
    valid = (idx >= 0) & (idx[:, :1] >= 0)
    rows = torch.arange(P)[:, None].expand(-1, k)[valid]
    prod = (w[valid][:, None] * g[rows]).double()        # the float32 products, exactly
    ref = torch.zeros((M, 32), dtype=torch.float64).index_add_(0, idx[valid].long(), prod)
    mag = torch.zeros((M, 32), dtype=torch.float64).index_add_(0, idx[valid].long(), prod.abs())
    count = torch.zeros(M, dtype=torch.float64).index_add_(0, idx[valid].long(), torch.ones(rows.numel(), dtype=torch.float64))
    assert info['slots'] == rows.numel()
    fixed = info['acc'].double() * 2.0 ** -info['s']
    bound = count[:, None] * 2.0 ** -(63 - info['guard']) * info['gmax'] + 2.0 ** -52 * mag
    err = (fixed - ref).abs()
    print(f'worst |fixed - f64| / bound = {(err / bound.clamp(min=1e-300)).max().item():.3e}')
    assert bool((err <= bound).all())
    assert bool((err[count == 0] == 0).all())
    assert torch.equal(info['named'], count > 0)
    assert GM.same_bits(out, fixed.float())


def test_every_term_is_within_half_a_unit():
    idx, w, g = synthetic(500, 100, 8, seed=7)
    _, info = GM.gather_bwd_feats(idx, w, g, torch.zeros((100, 32)))
    s = info['s']
    rows = torch.nonzero(idx[:, 0] >= 0).flatten()
    T = GM.terms(w[rows, 0], g[rows], s)
    exact = (w[rows, 0][:, None] * g[rows]).double() * 2.0 ** s
    assert bool(((T.double() - exact).abs() <= 0.5).all())
    assert bool((T.abs() < 2 ** (62 - info['guard'])).all())


def test_row_order_does_not_matter():
    idx, w, g = synthetic(1000, 300, 8, seed=11)
    pre = torch.randn((300, 32), generator=torch.Generator().manual_seed(1))
    out, info = GM.gather_bwd_feats(idx, w, g, pre)
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(2))
    out_p, info_p = GM.gather_bwd_feats(idx[perm], w[perm], g[perm], pre)
    assert torch.equal(info['acc'], info_p['acc'])
    assert torch.equal(out.view(torch.int32), out_p.view(torch.int32))


@pytest.mark.parametrize('P', [1023, 1024, 4096])
def test_worst_case_does_not_overflow(P):
    """One feature row named by every sample with weight 1 and dL/dc = the float32 below 2 everywhere:
    P same-sign terms in one element.  The int64 sum equals the sum in unbounded integers."""
    g1 = float(torch.tensor(1.9999999))
    assert g1 == 2.0 - 2.0 ** -23
    idx = torch.zeros((P, 1), dtype=torch.int32)
    w = torch.ones((P, 1))
    g = torch.full((P, 32), g1)
    for sign in (1.0, -1.0):
        out, info = GM.gather_bwd_feats(idx, w, sign * g, torch.zeros((3, 32)))
        s = info['s']
        assert s == 62 - GM.guard_bits(P) - 1
        term = int(Fraction(g1) * 2 ** s)
        assert Fraction(term, 2 ** s) == Fraction(g1), 'the term is exact'
        total = int(sign) * P * term
        assert abs(total) < 2 ** 62
        assert info['acc'][0].tolist() == [total] * 32
        assert bool((info['acc'][1:] == 0).all())
        assert out[0].tolist() == [float(torch.tensor(float(Fraction(total, 2 ** s))).float())] * 32
        assert bool((out[1:] == 0).all())


def test_unnamed_rows_keep_their_bits_and_prefill_accumulates():
    idx, w, g = synthetic(200, 400, 3, seed=13)
    pre = torch.randn((400, 32), generator=torch.Generator().manual_seed(3))
    pre[5] = -0.0  # (bit for bit: even a negative zero stays)
    idx[idx == 5] = 6
    out0, info = GM.gather_bwd_feats(idx, w, g, torch.zeros((400, 32)))
    out, _ = GM.gather_bwd_feats(idx, w, g, pre)
    named = info['named']
    assert 0 < int(named.sum()) < 400 and not bool(named[5])
    assert torch.equal(out[~named].view(torch.int32), pre[~named].view(torch.int32))
    assert torch.equal(out[named], pre[named] + out0[named])


def test_zero_gradient_and_no_neighbours():
    idx, w, g = synthetic(100, 50, 8, seed=17)
    pre = torch.randn((50, 32), generator=torch.Generator().manual_seed(4))
    out, info = GM.gather_bwd_feats(idx, w, torch.zeros_like(g), pre)
    assert info['gmax'] == 0.0 and info['s'] == 0 and bool((info['acc'] == 0).all())
    assert torch.equal(out.view(torch.int32), pre.view(torch.int32))
    none = torch.full_like(idx, -1)
    out, info = GM.gather_bwd_feats(none, torch.zeros_like(w), g, pre)
    assert info['slots'] == 0 and not bool(info['named'].any())
    assert torch.equal(out.view(torch.int32), pre.view(torch.int32))


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf')])
def test_non_finite_gradient(bad):
    idx, w, g = synthetic(100, 200, 3, seed=19, p_none=0.3)
    pre = torch.randn((200, 32), generator=torch.Generator().manual_seed(5))
    ref, info = GM.gather_bwd_feats(idx, w, g, pre)
    has = idx[:, 0] >= 0
    # in a row without neighbours: no effect at all
    g1 = g.clone()
    g1[int(torch.nonzero(~has)[0]), 7] = bad
    out, _ = GM.gather_bwd_feats(idx, w, g1, pre)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    # in a row with neighbours: NaN on every named row (not only that sample's), the rest untouched
    g2 = g.clone()
    g2[int(torch.nonzero(has)[0]), 7] = bad
    out, info2 = GM.gather_bwd_feats(idx, w, g2, pre)
    named = info['named']
    assert torch.equal(info2['named'], named) and info2['s'] is None and not math.isfinite(info2['gmax'])
    assert bool(torch.isnan(out[named]).all())
    assert torch.equal(out[~named].view(torch.int32), pre[~named].view(torch.int32))
    assert GM.same_bits(out, torch.where(named[:, None], torch.full_like(pre, float('nan')), pre))
