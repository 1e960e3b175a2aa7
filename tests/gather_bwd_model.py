"""The feature gradient of pnr_point_gather_bwd as ONE bit pattern (include/pnr.h, the comment above
pnr_point_gather_bwd_workspace_bytes), restated in plain torch integer arithmetic on any device.

The header's contract, not the kernel's loops:

  rows    a sample row is in the call when idx[row, 0] >= 0 (neighbours are stored nearest first)
  guard   the smallest integer >= 1 with 2^guard > P, at most 40
  gmax    max |dL/dc| over every channel of the call's rows
  e       the frexp exponent of gmax (gmax = m 2^e, 0.5 <= m < 1)
  s       62 - guard - e, or 0 when gmax is 0
  term    T = round_half_even(float64(fl32(w_k dL/dc)) 2^s) as int64: the product is formed in float32,
          the power-of-two scaling is exact, one rounding to an integer
  sum     acc[id, ch] = sum of T over the (row, slot) pairs that name id: exact, any order
  result  g_feats = fl32(g_feats + fl32(float64(acc) 2^-s)) on the rows some sample names; every other
          row is returned bit for bit
  gmax not finite: NaN on the named rows, the others untouched

The sum runs over one neighbour slot at a time, so the largest case needs P x 32 int64 words.
"""
import math

import torch

C_DIM = 32
MAX_GUARD = 40


def guard_bits(P: int) -> int:
    g = 1
    while g < MAX_GUARD and (1 << g) <= P:
        g += 1
    return g


def shift_of(gmax: float, guard: int) -> int:
    """s of the fixed point (gmax finite)."""
    if gmax == 0.0:
        return 0
    return 62 - guard - math.frexp(gmax)[1]


def terms(w_col, g_rows, s):
    """T (n,32) int64 of one neighbour slot: w_col (n) float32, g_rows (n,32) float32."""
    prod = w_col[:, None] * g_rows                      # float32 product, rounded once
    assert prod.dtype == torch.float32
    return torch.round(prod.double() * 2.0 ** s).to(torch.int64)  # exact scale, half-to-even


def accumulate(idx, w, g_c, M, s):
    """acc (M,32) int64 and the named-row mask (M) of a call; idx (P,k) int32, w (P,k), g_c (P,32)."""
    dev = g_c.device
    acc = torch.zeros((M, C_DIM), dtype=torch.int64, device=dev)
    named = torch.zeros(M, dtype=torch.bool, device=dev)
    has = idx[:, 0] >= 0
    n_slots = 0
    for j in range(idx.shape[1]):
        rows = torch.nonzero(has & (idx[:, j] >= 0)).flatten()
        if rows.numel() == 0:
            continue
        ids = idx[rows, j].long()
        named[ids] = True
        n_slots += rows.numel()
        if s is not None:
            acc.index_add_(0, ids, terms(w[rows, j], g_c[rows], s))
    return acc, named, n_slots


def gather_bwd_feats(idx, w, g_c, prefill):
    """(g_feats after the call, info) for g_feats = prefill (M,32) float32 before it.  info: guard, gmax,
    s (None when gmax is not finite), acc (int64), named (M bool), slots (valid neighbour slots)."""
    P = idx.shape[0]
    M = prefill.shape[0]
    guard = guard_bits(P)
    has = idx[:, 0] >= 0
    gsel = g_c[has].abs()
    gmax = float(gsel.max()) if gsel.numel() else 0.0  # (torch.max propagates NaN)
    finite = math.isfinite(gmax)
    s = shift_of(gmax, guard) if finite else None
    acc, named, n_slots = accumulate(idx, w, g_c, M, s)
    out = prefill.clone()
    if finite:
        delta = (acc[named].double() * 2.0 ** -s).float()  # one conversion
        out[named] = prefill[named] + delta                # float32 +=
    else:
        out[named] = float('nan')
    return out, dict(guard=guard, gmax=gmax, s=s, acc=acc, named=named, slots=n_slots)


def same_bits(a, b):
    """Equal as bit patterns, any NaN matching any NaN (the contract names no payload)."""
    a, b = a.contiguous(), b.contiguous()
    an, bn = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(an, bn)) and bool(torch.equal(a.view(torch.int32)[~an], b.view(torch.int32)[~bn]))
