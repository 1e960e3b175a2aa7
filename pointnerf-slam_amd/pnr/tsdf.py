"""A block-sparse TSDF volume fused from keyframe depth on the device (csrc/tsdf.hip; the rules are stated in
include/pnr.h at `pnr_tsdf`): the volume behind the reference's mesh bound (src/utils/Mesher.py:231-266, open3d's
ScalableTSDFVolume.integrate per keyframe) and the usual way a neural-point SLAM map is turned into a surface.

Blocks of 16^3 voxels behind a dense directory over `bound` padded by `sdf_trunc`; the slot arrays hold
`max_blocks` blocks.  Nothing here reads the device except the two counters (`n_blocks`, `dropped_blocks`) and
the counts of `extract_points` and `extract_triangle_mesh`, as marching cubes reads its counts.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

BLOCK = 16            # voxels per block edge
DEPTH_TRUNC = 1000.0  # src/utils/Mesher.py:261 (open3d's depth_trunc)


class TSDFVolume(object):
    """pnr_tsdf over `bound` (3,2): origin = float32(bound[:,0]) - float32(sdf_trunc), and as many blocks per
    axis as reach bound[:,1] + sdf_trunc.  Surface outside that box is dropped (open3d's hash is unbounded)."""

    def __init__(self, bound, voxel_length, sdf_trunc, H, W, fx, fy, cx, cy, max_blocks, depth_trunc=DEPTH_TRUNC,
                 device='cuda:0', color=True):
        self.lib = _lib.load()
        self.device = torch.device(device)
        b = np.asarray(bound.detach().cpu() if isinstance(bound, torch.Tensor) else bound, dtype=np.float64).reshape(3, 2)
        self.voxel_length, self.sdf_trunc = np.float32(voxel_length), np.float32(sdf_trunc)
        self.block_length = np.float32(BLOCK) * self.voxel_length
        self.origin = b[:, 0].astype(np.float32) - self.sdf_trunc
        span = b[:, 1] + float(self.sdf_trunc) - self.origin.astype(np.float64)
        self.dims = np.maximum(np.ceil(span / float(self.block_length)), 1).astype(np.int64)
        self.max_blocks = int(max_blocks)
        self.H, self.W = int(H), int(W)
        v = _lib.Tsdf()
        v.origin[:] = [float(x) for x in self.origin]
        v.voxel_length, v.sdf_trunc, v.depth_trunc = float(voxel_length), float(sdf_trunc), float(depth_trunc)
        v.dims[:] = [int(x) for x in self.dims]
        v.max_blocks, v.H, v.W = self.max_blocks, self.H, self.W
        v.fx, v.fy, v.cx, v.cy = float(fx), float(fy), float(cx), float(cy)
        nbytes = self.lib.pnr_tsdf_directory_bytes(ctypes.byref(v))
        self.ws_bytes = self.lib.pnr_tsdf_workspace_bytes(ctypes.byref(v))
        if nbytes == 0 or self.ws_bytes == 0:
            raise ValueError('pnr.tsdf: unsupported volume (0 < sdf_trunc < 16 voxel_length, fx, fy > 0, '
                             f'1 <= max_blocks <= 2^17, at most 2^27 directory entries; got {tuple(self.dims)} blocks)')
        # the slot arrays need no clearing: rows at or above n_blocks are never read
        self.directory = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
        self.tsdf = torch.empty((self.max_blocks, BLOCK ** 3), dtype=torch.float32, device=self.device)
        self.weight = torch.empty_like(self.tsdf)
        self.rgb = torch.empty((self.max_blocks, 3, BLOCK ** 3), dtype=torch.float32, device=self.device) if color else None
        self.block_index = torch.empty(self.max_blocks, dtype=torch.int32, device=self.device)
        _lib.require_cuda(self.directory)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.mesh_ws = None   # allocated by the first extract_triangle_mesh
        v.directory, v.tsdf, v.weight = self.directory.data_ptr(), self.tsdf.data_ptr(), self.weight.data_ptr()
        v.rgb = self.rgb.data_ptr() if color else None
        v.block_index = self.block_index.data_ptr()
        self.vol = v
        self.reset()

    def _ref(self):
        return ctypes.byref(self.vol)

    def reset(self):
        _lib.check(self.lib.pnr_tsdf_reset(self._ref(), _lib.stream_of(self.device)), 'tsdf_reset')

    def integrate(self, depth, color, c2w):
        """Fuses one frame (depth (H,W), color (H,W,3) or None, c2w (4,4)) or a stack (K,...) of them, in order."""
        depth = torch.as_tensor(depth).detach().to(self.device).float()
        c2w = torch.as_tensor(c2w).detach().to(self.device).float()
        if depth.dim() == 2:
            depth, c2w = depth[None], c2w[None]
            color = None if color is None else torch.as_tensor(color)[None]
        K = depth.shape[0]
        if depth.shape != (K, self.H, self.W) or c2w.shape != (K, 4, 4):
            raise ValueError('pnr.tsdf: depth (K,H,W) and c2w (K,4,4) expected')
        depth, c2w = depth.contiguous(), c2w.contiguous()
        if color is not None:
            if self.rgb is None:
                raise ValueError('pnr.tsdf: the volume keeps no colour')
            color = torch.as_tensor(color).detach().to(self.device).float().contiguous()
            if color.shape != (K, self.H, self.W, 3):
                raise ValueError('pnr.tsdf: color (K,H,W,3) expected')
        _lib.check(self.lib.pnr_tsdf_integrate(self._ref(), _lib.ptr(depth), _lib.ptr(color), _lib.ptr(c2w), K,
                                               _lib.ptr(self.ws), self.ws_bytes, _lib.stream_of(self.device)),
                   'tsdf_integrate')

    def integrate_frames(self, keyframe_dict):
        """One call over the keyframes' 'depth', 'color' (when every keyframe has one) and 'est_c2w'."""
        if len(keyframe_dict) == 0:
            return
        depth = torch.stack([kf['depth'].to(self.device).reshape(self.H, self.W) for kf in keyframe_dict])
        c2w = torch.stack([torch.as_tensor(kf['est_c2w']).detach().to(self.device).float().reshape(4, 4)
                           for kf in keyframe_dict])
        color = None
        if self.rgb is not None and all(kf.get('color') is not None for kf in keyframe_dict):
            color = torch.stack([kf['color'].to(self.device).reshape(self.H, self.W, 3) for kf in keyframe_dict])
        self.integrate(depth, color, c2w)

    def extract_points(self):
        """(xyz (N,3), rgb (N,3)) float32 on the device: the zero crossings between neighbouring voxels, in
        (slot, voxel index, axis) order.  rgb is zeros for a volume without colour."""
        st = _lib.stream_of(self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.pnr_tsdf_extract_count(self._ref(), _lib.ptr(self.ws), self.ws_bytes, _lib.ptr(count), st),
                   'tsdf_extract_count')
        n = int(count.item())
        xyz = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=self.device) if self.rgb is not None else None
        if n > 0:
            _lib.check(self.lib.pnr_tsdf_extract_emit(self._ref(), _lib.ptr(self.ws), self.ws_bytes, _lib.ptr(xyz),
                                                      _lib.ptr(rgb), st), 'tsdf_extract_emit')
        return xyz, (rgb if rgb is not None else torch.zeros_like(xyz))

    def extract_triangle_mesh(self):
        """(verts (V,3) float32, faces (F,3) int32, rgb (V,3) float32) on the device: marching cubes over the
        blocks, the cells that touch unobserved space left out, vertices shared across block faces and ordered
        by (slot, voxel index, axis) (include/pnr.h `pnr_tsdf_mesh_count`).  rgb is zeros for a volume without
        colour.  The two counts are the only host reads."""
        if self.mesh_ws is None:
            nbytes = self.lib.pnr_tsdf_mesh_workspace_bytes(self._ref())
            if nbytes == 0:
                raise ValueError('pnr.tsdf: max_blocks 4096 5 faces do not fit an int32 index')
            self.mesh_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        st, ws = _lib.stream_of(self.device), self.mesh_ws
        counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.pnr_tsdf_mesh_count(self._ref(), _lib.ptr(ws), ws.numel(), _lib.ptr(counts),
                                                _lib.ptr(counts[1:]), st), 'tsdf_mesh_count')
        n_v, n_f = (int(x) for x in counts.tolist())
        verts = torch.empty((n_v, 3), dtype=torch.float32, device=self.device)
        faces = torch.empty((n_f, 3), dtype=torch.int32, device=self.device)
        rgb = torch.empty((n_v, 3), dtype=torch.float32, device=self.device) if self.rgb is not None else None
        if n_v > 0:
            _lib.check(self.lib.pnr_tsdf_mesh_emit(self._ref(), _lib.ptr(ws), ws.numel(), _lib.ptr(verts),
                                                   _lib.ptr(rgb), _lib.ptr(faces), st), 'tsdf_mesh_emit')
        return verts, faces, (rgb if rgb is not None else torch.zeros_like(verts))

    @property
    def n_blocks(self):
        return int(self.directory[0].item())

    @property
    def dropped_blocks(self):
        return int(self.directory[1].item())

    def blocks(self):
        """Views of the live slots: dict(tsdf (n,16,16,16) indexed [k][j][i], weight, rgb (n,3,16,16,16) or None,
        coord (n,3) int64 block coordinates (bx, by, bz), index (n,) int32 directory entries)."""
        n = self.n_blocks
        idx = self.block_index[:n]
        e = idx.long()
        nx, ny = int(self.dims[0]), int(self.dims[1])
        coord = torch.stack([e % nx, (e // nx) % ny, e // (nx * ny)], 1)
        shape = (n, BLOCK, BLOCK, BLOCK)
        return dict(tsdf=self.tsdf[:n].view(shape), weight=self.weight[:n].view(shape),
                    rgb=None if self.rgb is None else self.rgb[:n].view(n, 3, BLOCK, BLOCK, BLOCK), coord=coord, index=idx)
