"""Two-way nearest-neighbour matching of unit descriptors on the device (src/Tracker.py:398-455:
`nn_match_two_way` as `match_frames` calls it for the SuperPoint track step).

`desc1` (D, N) and `desc2` (D, M) are contiguous float32 device tensors with unit-norm columns, D a
multiple of 32 in [32, 512].  pnr_match_two_way (include/pnr.h, csrc/match.hip) forms desc1^T desc2 on
fp32 MFMA with both arg-max reductions in its epilogue; the N x M matrix is never stored.  Non-finite
descriptors are the caller's error: they are not looked for, and a NaN product counts as a dot of -1.
There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib


class MatchBuffers(object):
    """Outputs and workspace of one (N, M) call: idx1, idx2 (N,) int32, score (N,) float32, count (1,)
    int32, workspace uint8.  `match_two_way(..., buffers=b)` reuses them frame after frame; their
    contents before a call do not matter."""

    def __init__(self, N, M, device):
        nbytes = _lib.load().pnr_match_workspace_bytes(N, M)
        if nbytes == 0:
            raise ValueError(f'pnr.match_two_way: sizes N = {N}, M = {M} are out of range')
        self.N, self.M = N, M
        self.idx1 = torch.empty(N, dtype=torch.int32, device=device)
        self.idx2 = torch.empty(N, dtype=torch.int32, device=device)
        self.score = torch.empty(N, dtype=torch.float32, device=device)
        self.count = torch.empty(1, dtype=torch.int32, device=device)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)


def _check(desc1, desc2, nn_thresh):
    _lib.require_cuda(desc1, desc2)
    for d in (desc1, desc2):
        if d.dtype != torch.float32 or d.dim() != 2 or not d.is_contiguous():
            raise ValueError('pnr.match_two_way: descriptors are contiguous float32 (D, n) tensors')
    D = desc1.shape[0]
    if desc2.shape[0] != D or desc2.device != desc1.device:
        raise ValueError('pnr.match_two_way: desc1 and desc2 differ in D or in device')
    if D < 32 or D > 512 or D % 32:
        raise ValueError(f'pnr.match_two_way: D = {D} is not a multiple of 32 in [32, 512]')
    if not nn_thresh >= 0.0:
        raise ValueError("'nn_thresh' should be non-negative")


def match_two_way(desc1, desc2, nn_thresh=0.7, return_best=False, buffers=None):
    """(idx1, idx2, score): the L mutual nearest neighbours with distance sqrt(2 - 2 dot) < nn_thresh, in
    ascending idx1 -- int64, int64, float32 device tensors; one host read (the count) trims them.
    return_best: also `best` (N,) int64, every row's nearest column of desc2, kept or not (decoded from
    the workspace's row keys)."""
    _check(desc1, desc2, nn_thresh)
    N, M, dev = desc1.shape[1], desc2.shape[1], desc1.device
    if N == 0 or M == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        out = (e, e.clone(), torch.empty(0, dtype=torch.float32, device=dev))
        return out + (torch.empty(0, dtype=torch.int64, device=dev),) if return_best else out
    b = buffers if buffers is not None else MatchBuffers(N, M, dev)
    if (b.N, b.M) != (N, M) or b.workspace.device != dev:
        raise ValueError('pnr.match_two_way: buffers were made for other sizes or another device')
    _lib.check(_lib.load().pnr_match_two_way(
        _lib.ptr(desc1), _lib.ptr(desc2), desc1.shape[0], N, M, float(nn_thresh), _lib.ptr(b.idx1), _lib.ptr(b.idx2),
        _lib.ptr(b.score), _lib.ptr(b.count), _lib.ptr(b.workspace), b.workspace.numel(), _lib.stream_of(dev)),
        'match_two_way')
    L = int(b.count.item())
    out = (b.idx1[:L].long(), b.idx2[:L].long(), b.score[:L].clone())
    if return_best:
        row_key = b.workspace[:8 * N].view(torch.int64)
        out += (0xFFFFFFFF - (row_key & 0xFFFFFFFF),)
    return out


def nn_match_two_way(desc1, desc2, nn_thresh):
    """The reference's call shape: a (3, L) float64 device tensor [idx1; idx2; score], (3, 0) without a
    launch when either set is empty."""
    if desc1.shape[1] == 0 or desc2.shape[1] == 0:   # (the reference returns before it looks at nn_thresh)
        _lib.require_cuda(desc1, desc2)
        return torch.zeros((3, 0), dtype=torch.float64, device=desc1.device)
    i1, i2, s = match_two_way(desc1, desc2, nn_thresh)
    return torch.stack([i1.double(), i2.double(), s.double()])
