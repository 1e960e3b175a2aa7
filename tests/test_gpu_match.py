"""pnr.match_two_way (csrc/match.hip) against nn_match_two_way (src/Tracker.py:398-440) restated in float64.

Tolerance, derived: for unit columns any summation order gives |fl(dot) - dot| <= D 2^-24; tau = 2 D 2^-24
(the factor 2 covers the MFMA's internal order and the 5e-7 norm error of float32 unit vectors).  A row is
"decided" when its best-to-second gap and the gap of its best column exceed 2 tau and 2 - 2 dot is more
than 3 tau from nn_thresh^2; only there must the kept flag and idx2 equal the reference.  Shapes: the
kernel's tile is 64 x 64 (four 32 x 32 waves), so 1 x 1 is the smallest call, 33 x 31 one ragged tile, 129
and 65 cross a row-tile boundary by one row, 130 and 257 a column-tile boundary, 300 x 257 is several tiles
each way and D = 512 the largest.  In the tie test rows 7 and 40 lie in different waves of one workgroup,
columns 3 and 129 in different workgroups."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THRESH = 0.7
SHAPES = [(1, 1, 32), (33, 31, 32), (129, 64, 64), (65, 130, 256), (300, 257, 256), (200, 70, 512)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def unit(x):
    return (x / np.linalg.norm(x, axis=0, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(N, M, D):
    """a (D,N), b (D,M) float32 unit columns: b holds distractors, and at 2/3 min(N, M) random positions
    noisy copies of random columns of a (sigma ~ U(0, 0.08) per component); dot = the float64 product."""
    rng = np.random.RandomState(0)
    a, b = unit(rng.randn(D, N)), unit(rng.randn(D, M))
    k = 2 * min(N, M) // 3
    pos, src = rng.choice(M, k, replace=False), rng.randint(0, N, k)
    b[:, pos] = unit(a[:, src] + rng.uniform(0, 0.08, k) * rng.randn(D, k))
    return a, b, np.clip(a.astype(np.float64).T @ b.astype(np.float64), -1, 1)


def best_and_gap(dot):
    """per row: argmax, max, max - second (inf for a single column)"""
    s = np.sort(dot, axis=1)
    gap = s[:, -1] - s[:, -2] if dot.shape[1] > 1 else np.full(dot.shape[0], np.inf)
    return dot.argmax(1), s[:, -1], gap


def run(pnr, dev, a, b, **kw):
    out = pnr.match_two_way(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), THRESH, **kw)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize('N,M,D', SHAPES)
def test_parity(dev, N, M, D):
    import pnr
    a, b, dot = case(N, M, D)
    tau = 2 * D * 2.0 ** -24
    i1, i2, sc, best = run(pnr, dev, a, b, return_best=True)
    rows = np.arange(N)
    assert best.shape == (N,) and (best >= 0).all() and (best < M).all()
    # every row: the chosen column is within tau of the row's maximum
    jstar, top, gap = best_and_gap(dot)
    assert (top - dot[rows, best] <= tau).all()
    assert (np.diff(i1) > 0).all() and (i2 == best[i1]).all()
    own = 1.0 - sc.astype(np.float64) ** 2 / 2                   # the kernel's own dot of a kept row
    assert (np.abs(own - dot[i1, i2]) <= 1.5 * tau).all()        # (the 3 tau bound on score^2 below, halved)
    # decided rows: kept flag and idx2 equal the reference
    istar, _, cgap = best_and_gap(dot.T)
    d2 = 2 - 2 * top
    decided = (gap > 2 * tau) & (cgap[jstar] > 2 * tau) & (np.abs(d2 - THRESH ** 2) > 3 * tau)
    assert (~decided).sum() <= 0.05 * N, 'the inputs leave too many undecided rows: change the seed'
    keep_ref = (d2 < THRESH ** 2) & (istar[jstar] == rows)
    kept = np.zeros(N, bool)
    kept[i1] = True
    assert (kept[decided] == keep_ref[decided]).all() and (best[decided] == jstar[decided]).all()
    dk = decided[i1]
    assert (np.abs(sc[dk].astype(np.float64) ** 2 - d2[i1[dk]]) <= 3 * tau).all()
    table = pnr.nn_match_two_way(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), THRESH)
    assert table.dtype == torch.float64 and table.shape == (3, len(i1))
    assert np.array_equal(table.cpu().numpy(), np.stack([i1, i2, sc]).astype(np.float64))


def test_ties_and_clip(dev):
    import pnr
    a, b, _ = case(65, 130, 256)
    a, b = a.copy(), b.copy()
    b[:, 3] = b[:, 129] = a[:, 40] = a[:, 7]
    i1, i2, sc, best = run(pnr, dev, a, b, return_best=True)
    assert best[7] == 3 and best[40] == 3                        # the lowest column among equal dots
    at = np.nonzero(i2 == 3)[0]
    assert len(at) == 1 and i1[at[0]] == 7 and 40 not in i1      # column 3 chose the lowest row
    assert 0.0 <= sc[at[0]] <= np.sqrt(2 * 2 * 256 * 2.0 ** -24)  # 0 exactly once the dot reaches 1 (the clip)


def test_deterministic_and_dirty_buffers(dev):
    import pnr
    a, b, _ = case(300, 257, 256)
    first = run(pnr, dev, a, b, return_best=True)
    again = run(pnr, dev, a, b, return_best=True)
    bufs = pnr.matching.MatchBuffers(300, 257, dev)
    for t in (bufs.idx1, bufs.idx2, bufs.score, bufs.count, bufs.workspace):
        t.view(torch.uint8).fill_(0xFF)
    dirty = run(pnr, dev, a, b, return_best=True, buffers=bufs)
    reused = run(pnr, dev, a, b, return_best=True, buffers=bufs)
    assert len(first[0]) > 0
    for other in (again, dirty, reused):
        for x, y in zip(first, other):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_refusals(dev):
    import pnr
    a = torch.from_numpy(case(33, 31, 32)[0]).to(dev)
    b = torch.from_numpy(case(33, 31, 32)[1]).to(dev)
    with pytest.raises(ValueError):
        pnr.match_two_way(a, b, -0.1)
    with pytest.raises(ValueError):
        pnr.nn_match_two_way(a, b, -0.1)
    with pytest.raises(ValueError):
        pnr.match_two_way(torch.zeros((48, 5), device=dev), torch.zeros((48, 4), device=dev))
    with pytest.raises(RuntimeError):
        pnr.match_two_way(a.cpu(), b)
    with pytest.raises(ValueError):
        pnr.match_two_way(a.double(), b.double())
    with pytest.raises(ValueError):
        pnr.match_two_way(a.t(), b.t()[:, :33])                  # not contiguous
    empty = pnr.nn_match_two_way(a[:, :0], b, 0.7)
    assert empty.shape == (3, 0) and empty.dtype == torch.float64 and empty.is_cuda
    assert pnr.nn_match_two_way(a, b[:, :0], 0.7).shape == (3, 0)
    L = pnr.library()
    one = a.data_ptr()
    assert L.pnr_match_workspace_bytes(33, 31) == 64 * 8 and L.pnr_match_workspace_bytes(-1, 4) == 0
    assert L.pnr_match_two_way(one, one, 48, 33, 31, 0.7, one, one, one, one, one, 1 << 20, None) == -1
    assert L.pnr_match_two_way(one, one, 32, 33, 31, -0.1, one, one, one, one, one, 1 << 20, None) == -1
    assert L.pnr_match_two_way(one, one, 32, 33, 31, 0.7, one, one, one, one, one, 8, None) == -2
