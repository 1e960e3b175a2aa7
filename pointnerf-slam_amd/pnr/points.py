"""Neural points: positions + learnable features, gathered per sample on the HIP path.

SURVEY.md §8 row A15 (build-defined; the reference has no neural-point stage).  The decoder's
feature input c(p) is aggregated from the k nearest points around p (include/pnr.h `pnr_points`,
oracle/ref_points.py is the spec):

  mode='idw'        points within `radius`, weights 1/max(|p-x|, eps)
  mode='trilinear'  points within one lattice `spacing` per axis, weights prod(1-|dp|/h) --
                    with points on the vertices of a feature grid this is the reference's
                    MLP.sample_grid_feature (src/conv_onet/models/decoder.py:168-175)

A `NeuralPoints` rides in the Renderer's `c` dict under 'points_<decoder name>' (an empty dict
keeps the reference behaviour).  Features are an nn.Parameter; gradients reach them (and the
sample positions, for tracking) through the gather backward.  The spatial hash (pnr_points_build)
is rebuilt on the device whenever the positions change.

A cloud made with a `capacity` can grow: `add_frame` back-projects a keyframe's depth on the device
and appends points where the map has none (include/pnr.h pnr_points_add_frame).  `xyz` and `feats`
are then allocated at capacity, rows [0, n_points) are live, and every C call sees the live count.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _lib

_MODES = {'idw': _lib.GATHER_IDW, 'trilinear': _lib.GATHER_TRILINEAR}


class NeuralPoints(nn.Module):
    def __init__(self, xyz: torch.Tensor, feats: torch.Tensor = None, c_dim: int = 32, mode: str = 'idw',
                 k: int = 8, radius: float = 0.02, eps: float = 1e-6, spacing=None, cell: float = None,
                 origin=None, table_bits: int = None, feat_dtype: str = 'float32', capacity: int = None,
                 bound=None):
        super().__init__()
        if feat_dtype not in ('float32', 'float16'):
            raise ValueError("pnr.NeuralPoints: feat_dtype must be 'float32' or 'float16'")
        if c_dim != _lib.C_DIM:
            raise NotImplementedError(f'pnr.NeuralPoints: c_dim must be {_lib.C_DIM}')
        if mode not in _MODES:
            raise ValueError(f'pnr.NeuralPoints: mode must be one of {sorted(_MODES)}')
        if not 1 <= k <= _lib.MAX_K:
            raise ValueError(f'pnr.NeuralPoints: 1 <= k <= {_lib.MAX_K}')
        xyz = xyz.detach().float().reshape(-1, 3).contiguous()
        M = xyz.shape[0]
        if feats is None:
            feats = torch.zeros((M, c_dim), device=xyz.device)
        feats = feats.detach().float().reshape(M, c_dim).contiguous().clone()
        # capacity: rows [0, n_points) are live, rows up to `capacity` are room for add_frame (zero
        # until then; no sample has them as neighbours, so they receive no gradient)
        if capacity is not None:
            capacity = int(capacity)
            if capacity < M:
                raise ValueError(f'pnr.NeuralPoints: capacity {capacity} is below the {M} points given')
            if M == 0 and origin is None and bound is None:
                raise ValueError('pnr.NeuralPoints: an empty cloud with a capacity needs `origin` or `bound` '
                                 '(the hash origin cannot come from the points)')
            xyz = torch.cat([xyz, torch.zeros((capacity - M, 3), device=xyz.device)], 0)
            feats = torch.cat([feats, torch.zeros((capacity - M, c_dim), device=feats.device)], 0)
        self.capacity = capacity
        self._n = M
        self.last_add = None
        self.register_buffer('xyz', xyz)
        self.feats = nn.Parameter(feats)
        self.mode = mode
        self.k = int(k)
        self.radius = float(radius)
        self.eps = float(eps)
        self.spacing = [float(v) for v in (spacing if spacing is not None else (radius, radius, radius))]
        reach = self.radius if mode == 'idw' else max(self.spacing)
        # the search probes the 2x2x2 cells covering [p - reach, p + reach]: cell >= 2 reach, with a
        # margin so that float rounding of the cell coordinates never misses a neighbour
        # (points.hip kCellMargin: the search's widened reach must stay within half a cell)
        self.cell = float(cell) if cell is not None else 2.0 * reach * (1.0 + 4e-3)
        if self.cell < 2.0 * reach * (1.0 + 2.0 ** -9):
            raise ValueError('pnr.NeuralPoints: cell must be >= 2 x the neighbourhood reach x (1 + 2^-9)')
        if origin is None and bound is not None and capacity is not None:
            lo = torch.as_tensor(bound, dtype=torch.float64).reshape(3, 2)[:, 0]
            origin = (lo - self.cell).tolist()
        if origin is None:
            origin = (xyz[:M].min(0).values - self.cell).tolist() if M > 0 else [0.0, 0.0, 0.0]
        self.origin = [float(v) for v in origin]
        if table_bits is None:  # ~2 buckets per occupied cell (a surface cell holds ~4-16 points)
            rows = M if capacity is None else capacity
            table_bits = min(24, max(10, int(math.ceil(math.log2(max(rows // 2, 1))))))
        self.table_bits = int(table_bits)
        self._index = None
        self._index_key = None
        # float16 features (the C5 budget): the gather reads an f16 copy of the fp32
        # master `feats` (the optimiser's parameter); the copy is refreshed when feats changed
        self.feat_dtype = feat_dtype
        self._feats_h = None
        self._feats_h_key = None

    @property
    def n_points(self) -> int:
        """Live points: rows [0, n_points) of `xyz` / `feats` (all of them without a capacity)."""
        return self._n

    def invalidate_feats(self):
        """Mark the f16 copy stale (after an in-place update torch does not version, e.g. the
        pnr Adam kernel writing through a raw pointer)."""
        self._feats_h_key = None

    def mark_feats_fresh(self):
        """The f16 copy holds float16(feats) again (written by pnr_adam_multi_dev_h with the master)."""
        if self._feats_h is not None:
            self._feats_h_key = (self.feats.data_ptr(), self.feats._version)

    def _feats_for_gather(self):
        if self.feat_dtype == 'float32':
            return self.feats
        f = self.feats
        key = (f.data_ptr(), f._version)
        if self._feats_h is None or self._feats_h.shape != f.shape or self._feats_h.device != f.device:
            self._feats_h = torch.empty(f.shape, dtype=torch.float16, device=f.device)
            self._feats_h_key = None
        if self._feats_h_key != key:
            with torch.no_grad():
                self._feats_h.copy_(f)
            self._feats_h_key = key
        return self._feats_h

    @classmethod
    def from_grid(cls, grid: torch.Tensor, bound: torch.Tensor, **kw):
        """Points on the vertices of an align_corners=True feature grid (1,C,D,H,W) over `bound`
        (x <-> W, y <-> H, z <-> D), trilinear weights: reproduces F.grid_sample on interior samples."""
        _, C, D, H, W = grid.shape
        b = torch.as_tensor(bound, dtype=torch.float64).reshape(3, 2).cpu()
        lo, hi = b[:, 0], b[:, 1]
        sp = (hi - lo) / torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float64)
        d, h, w = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij')
        ijk = torch.stack([w, h, d], -1).reshape(-1, 3).double()
        xyz = (lo + ijk * sp).float().to(grid.device)
        feats = grid[0].reshape(C, -1).t().contiguous()
        return cls(xyz, feats, c_dim=C, mode='trilinear', spacing=sp.float().tolist(), **kw)

    # -- device index -----------------------------------------------------------------------------
    def _struct(self) -> _lib.Points:
        s = _lib.Points()
        s.xyz = self.xyz.data_ptr()
        s.feats = self._feats_for_gather().data_ptr()
        s.feat_half = 1 if self.feat_dtype == 'float16' else 0
        s.n_points = self._n
        s.mode = _MODES[self.mode]
        s.k = self.k
        s.radius = self.radius
        s.eps = self.eps
        for i in range(3):
            s.spacing[i] = self.spacing[i]
            s.origin[i] = self.origin[i]
        s.cell = self.cell
        s.table_bits = self.table_bits
        return s

    def index(self) -> torch.Tensor:
        """The spatial hash (device bytes), rebuilt when positions or the hash layout changed."""
        _lib.require_cuda(self.xyz)
        key = (self.xyz.data_ptr(), self.xyz._version, self._n, self.cell, tuple(self.origin), self.table_bits)
        if self._index is not None and key == self._index_key:
            return self._index
        lib = _lib.load()
        # (sized for every row: the layout for n_points <= capacity rows fits, so growing never reallocates)
        nbytes = lib.pnr_points_index_bytes(self.xyz.shape[0], self.table_bits)
        if self._index is None or self._index.numel() < nbytes or self._index.device != self.xyz.device:
            self._index = torch.empty(nbytes, dtype=torch.uint8, device=self.xyz.device)
        s = self._struct()
        s.index = self._index.data_ptr()
        _lib.check(lib.pnr_points_build(ctypes.byref(s), _lib.stream_of(self.xyz.device)), 'points_build')
        self._index_key = key
        return self._index

    def descriptor(self, fc_packed=None, g_feats=None, g_fc=None):
        """(pnr_points struct, keep-alive list) for one C call."""
        s = self._struct()
        s.index = self.index().data_ptr()
        keep = []
        if fc_packed is not None:
            s.fc_packed = fc_packed.data_ptr()
        if g_feats is not None:
            s.g_feats = g_feats.data_ptr()
        if g_fc is not None:
            arr = _lib.FcPtrArray(*[t.data_ptr() for t in g_fc])
            keep.append(arr)
            s.g_fc = ctypes.cast(arr, ctypes.c_void_p).value
        return s, keep

    def gather(self, p: torch.Tensor) -> torch.Tensor:
        """c(p) (P,32) float32 for points p (P,3); differentiable w.r.t. p and `feats`."""
        p = p.reshape(-1, 3)
        _lib.require_cuda(p)
        return _GatherFn.apply(p.double().contiguous(), self, self.feats)

    def add_frame(self, depth, c2w, H, W, fx, fy, cx, cy, bound, pixels=None, stride=1, rho=(0.0,),
                  radius_add=None, thin=None, init_feats=None, return_candidates=False) -> int:
        """Grow the map from one keyframe (Point-SLAM's add_neural_points; include/pnr.h
        pnr_points_add_frame states the rules, tests/points_grow_ref.py restates them).  depth (H,W)
        float32 and c2w (4,4) / (3,4) device tensors in the renderer's convention; the candidates are
        the `pixels` (int64 flat indices v W + u) or every `stride`-th pixel of both axes, each at the
        relative depth offsets `rho`.  A candidate inside `bound` with no existing point within
        `radius_add` (default: the gather radius) is added, one per voxel of edge `thin` (default
        radius_add; 0 = no thinning), with row c of `init_feats` (n_cand,32) or zero features.  Returns
        the number of rows appended; `last_add` holds the counters (one host read per frame).  The index
        is rebuilt by the next call that needs it.  return_candidates: keep the pass's candidate
        positions and PNR_ADD_* flag bytes in `last_candidates` (tests)."""
        if self.capacity is None:
            raise RuntimeError('pnr.NeuralPoints.add_frame: the cloud was made without a capacity')
        radius_add = self.radius if radius_add is None else float(radius_add)
        thin = radius_add if thin is None else float(thin)
        rho = [float(r) for r in rho]
        if not 1 <= len(rho) <= _lib.MAX_RHO:
            raise ValueError(f'pnr.NeuralPoints.add_frame: 1 <= len(rho) <= {_lib.MAX_RHO}')
        if not radius_add > 0 or thin < 0 or int(stride) < 1:
            raise ValueError('pnr.NeuralPoints.add_frame: radius_add > 0, thin >= 0 and stride >= 1 are required')
        if radius_add > self.cell / (2.0 * (1.0 + 2.0 ** -9)):
            raise ValueError('pnr.NeuralPoints.add_frame: radius_add must be <= cell / (2 (1 + 2^-9)) '
                             '(the 2x2x2 probe must cover the ball)')
        _lib.require_cuda(self.xyz, depth)
        dev = self.xyz.device
        H, W = int(H), int(W)
        depth = depth.to(device=dev, dtype=torch.float32).reshape(H, W).contiguous()
        c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev)
        if c2w.shape[-2] == 3:
            c2w = torch.cat([c2w, torch.tensor([[0., 0., 0., 1.]], device=dev)], 0)
        c2w = c2w.reshape(4, 4).contiguous()
        a = _lib.PointsAdd()
        a.depth, a.c2w, a.H, a.W = depth.data_ptr(), c2w.data_ptr(), H, W
        a.fx, a.fy, a.cx, a.cy = float(fx), float(fy), float(cx), float(cy)
        if pixels is not None:
            pixels = torch.as_tensor(pixels, dtype=torch.int64, device=dev).reshape(-1).contiguous()
            n_pix = pixels.numel()
            if n_pix == 0:  # (an empty tensor has a null pointer, which would select the stride lattice)
                pixels = torch.zeros(1, dtype=torch.int64, device=dev)
            a.pixels, a.n_pixels = pixels.data_ptr(), n_pix
        else:
            n_pix = ((H + stride - 1) // stride) * ((W + stride - 1) // stride)
        a.stride, a.n_rho = int(stride), len(rho)
        for i, r in enumerate(rho):
            a.rho[i] = r
        a.radius_add, a.thin = radius_add, thin
        for i, v in enumerate(torch.as_tensor(bound, dtype=torch.float64).reshape(6).tolist()):
            a.bound[i] = v
        n_cand = n_pix * len(rho)
        if n_cand >= 2 ** 31:
            raise ValueError('pnr.NeuralPoints.add_frame: at most 2^31 - 1 candidates per call')
        if init_feats is not None:
            init_feats = init_feats.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(init_feats.shape) != (n_cand, _lib.C_DIM):
                raise ValueError(f'pnr.NeuralPoints.add_frame: init_feats must be ({n_cand}, {_lib.C_DIM})')
            a.init_feats = init_feats.data_ptr()
        cand = None
        if return_candidates:
            cand = (torch.empty((n_cand, 3), device=dev), torch.empty(n_cand, dtype=torch.uint8, device=dev))
            a.cand_xyz, a.cand_flags = cand[0].data_ptr(), cand[1].data_ptr()
        lib = _lib.load()
        s = self._struct()
        s.index = self.index().data_ptr()
        ws = torch.empty(lib.pnr_points_add_workspace_bytes(n_cand), dtype=torch.uint8, device=dev)
        counters = torch.empty(5, dtype=torch.int64, device=dev)
        _lib.check(lib.pnr_points_add_frame(ctypes.byref(s), self.capacity, _lib.ptr(self.xyz), _lib.ptr(self.feats),
                                            ctypes.byref(a), _lib.ptr(ws), ws.numel(), _lib.ptr(counters),
                                            _lib.stream_of(dev)), 'points_add_frame')
        n_c, n_valid, n_free, n_kept, n_drop = counters.tolist()  # the frame's one host read
        n_new = n_kept - n_drop
        self._n += n_new  # the index key carries the live count: the next index() rebuilds
        self.invalidate_feats()
        self.last_add = {'candidates': n_c, 'valid': n_valid, 'free': n_free, 'survivors': n_kept,
                         'dropped': n_drop, 'added': n_new}
        self.last_candidates = cand
        return n_new

    def __getstate__(self):
        st = self.__dict__.copy()  # (carries the live count `_n` and the capacity)
        st['_index'] = None  # device caches never cross pickling / deepcopy
        st['_index_key'] = None
        st['_feats_h'] = None
        st['_feats_h_key'] = None
        st['last_candidates'] = None
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        if '_n' not in self.__dict__:  # a state from before clouds could grow: every row is live
            self.capacity = None
            self._n = self.xyz.shape[0]
            self.last_add = None


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, pts, feats):
        lib = _lib.load()
        P = p.shape[0]
        dev = p.device
        c = torch.empty((P, _lib.C_DIM), device=dev, dtype=torch.float32)
        need = any(ctx.needs_input_grad)
        idx = torch.empty((P, pts.k), device=dev, dtype=torch.int32) if need else None
        w = torch.empty((P, pts.k), device=dev, dtype=torch.float32) if need else None
        s, keep = pts.descriptor()
        ws = torch.empty(lib.pnr_point_gather_workspace_bytes(P), dtype=torch.uint8, device=dev)
        _lib.check(lib.pnr_point_gather(ctypes.byref(s), _lib.ptr(p), P, _lib.ptr(c), _lib.ptr(idx), _lib.ptr(w),
                                        _lib.ptr(ws), ws.numel(), _lib.stream_of(dev)), 'point_gather')
        if need:
            ctx.pts = pts
            ctx.save_for_backward(p, idx, w, c)
        return c

    @staticmethod
    def backward(ctx, g_c):
        lib = _lib.load()
        p, idx, w, c = ctx.saved_tensors
        pts = ctx.pts
        dev = p.device
        P = p.shape[0]
        g_feats = torch.zeros_like(pts.feats) if ctx.needs_input_grad[2] else None
        g_p = torch.empty((P, 3), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        s, keep = pts.descriptor(g_feats=g_feats)
        ws = torch.empty(lib.pnr_point_gather_bwd_workspace_bytes(ctypes.byref(s), P), dtype=torch.uint8, device=dev)
        _lib.check(lib.pnr_point_gather_bwd(ctypes.byref(s), _lib.ptr(p), P, _lib.ptr(idx), _lib.ptr(w), _lib.ptr(c),
                                            _lib.ptr(g_c.contiguous()), _lib.ptr(g_p), _lib.ptr(ws), ws.numel(),
                                            _lib.stream_of(dev)), 'point_gather_bwd')
        return (None if g_p is None else g_p.double(), None, g_feats)


def find_points(c, decoders):
    """The NeuralPoints of decoder `decoders` in the Renderer's `c` dict (None = reference path)."""
    if not getattr(decoders, 'c_dim', 0):
        return None
    name = getattr(decoders, 'name', '')
    if isinstance(c, NeuralPoints):
        return c
    if isinstance(c, dict):
        for key in ('points_' + name, 'grid_' + name):
            v = c.get(key)
            if isinstance(v, NeuralPoints):
                return v
    raise ValueError(f"pnr: decoder '{name}' has c_dim={decoders.c_dim}: pass its NeuralPoints as "
                     f"c['points_{name}']")
