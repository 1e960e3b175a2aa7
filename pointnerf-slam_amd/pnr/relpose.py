"""Relative pose from matches on the device (src/Tracker.py:356-360 `estimatePose`, :458-548
`track_reference_frame`, :571-610 the pseudo-depth map; src/utils/utils_geom.py:140-207).

Everything is float64 on the device (csrc/relpose.hip, include/pnr.h): a five-point solver run on `samples`
minimal samples, Sampson scoring of every hypothesis on f64 MFMA, the decomposition and cheirality vote of
cv2.recoverPose, DLT triangulation and the pseudo-depth painting.  Deviations from the reference, stated:
`samples` is fixed and every sample is scored (no adaptive stop from `prob`; 1024 is cv2's maxIters rounded
up); the painting pairs point i with depth i, compares u with W and has background 0 (include/pnr.h);
undistortion is not built.  There is no CPU path.
"""
from __future__ import annotations

import collections

import torch

from . import _lib

PoseResult = collections.namedtuple('PoseResult', 'Trc E mask num_inliers R t hypothesis samples')


def _points(name, *ts):
    _lib.require_cuda(*ts)
    out = []
    for t in ts:
        if t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous() or t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f'pnr.relpose.{name}: points are contiguous (L,2) float32 or float64 tensors')
        if t.shape[0] != ts[0].shape[0] or t.device != ts[0].device:
            raise ValueError(f'pnr.relpose.{name}: the point sets differ in length or device')
        out.append(t.double())
    return out


class PoseBuffers(object):
    """Outputs and workspace of one (L, S) call: pose (37,) float64 = E | R | t | Trc, mask (L,) uint8, count
    (1,) int32, workspace uint8.  `estimate_pose(..., buffers=b)` reuses them frame after frame; their contents
    before a call do not matter."""

    def __init__(self, L, S, device):
        nbytes = _lib.load().pnr_relpose_workspace_bytes(L, S)
        if nbytes == 0:
            raise ValueError(f'pnr.estimate_pose: sizes L = {L}, samples = {S} are out of range')
        self.L, self.S = L, S
        self.pose = torch.empty(37, dtype=torch.float64, device=device)
        self.mask = torch.empty(L, dtype=torch.uint8, device=device)
        self.count = torch.empty(1, dtype=torch.int32, device=device)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)


def estimate_pose(kpn_ref, kpn_cur, threshold=0.0003, samples=1024, seed=0, return_samples=False, buffers=None):
    """`Tracker.estimatePose(kpn_ref, kpn_cur)`: the pose Trc of the current frame in the reference frame
    (p_ref = Trc p_cur, unit baseline) from (L,2) normalised matches, as findEssentialMat(kpn_cur, kpn_ref) and
    recoverPose give it.  Returns a PoseResult of device tensors: Trc (4,4), E (3,3), mask (L,) bool, num_inliers
    (int32 scalar), R, t, hypothesis (the winner's index 10 sample + root, -1 for none) and, with
    return_samples, the (samples,5) int32 draws.  No host synchronisation."""
    if kpn_ref.shape[0] < 5:
        raise ValueError('pnr.estimate_pose: the five-point solver needs at least 5 matches')
    if samples < 1:
        raise ValueError("'samples' should be at least 1")
    if not threshold >= 0.0:
        raise ValueError("'threshold' should be non-negative")
    x2, x1 = _points('estimate_pose', kpn_ref, kpn_cur)
    L, dev = x1.shape[0], x1.device
    b = buffers if buffers is not None else PoseBuffers(L, samples, dev)
    if (b.L, b.S) != (L, samples) or b.workspace.device != dev:
        raise ValueError('pnr.estimate_pose: buffers were made for other sizes or another device')
    _lib.check(_lib.load().pnr_relpose_estimate(
        _lib.ptr(x1), _lib.ptr(x2), L, samples, int(seed) & 0xFFFFFFFF, float(threshold), _lib.ptr(b.pose),
        _lib.ptr(b.mask), _lib.ptr(b.count), _lib.ptr(b.workspace), b.workspace.numel(), _lib.stream_of(dev)),
        'relpose_estimate')
    key = b.workspace[:8].view(torch.int64)[0]
    hyp = torch.where(key != 0, 0xFFFFFFFF - (key & 0xFFFFFFFF), torch.full_like(key, -1))
    smp = None
    if return_samples:
        off = 64 + 720 * samples
        smp = b.workspace[off:off + 20 * samples].view(torch.int32).view(samples, 5).clone()
    p = b.pose
    return PoseResult(p[21:37].view(4, 4).clone(), p[0:9].view(3, 3).clone(), b.mask.bool(), b.count[0].clone(),
                      p[9:18].view(3, 3).clone(), p[18:21].clone(), hyp, smp)


def five_point(x1, x2):
    """The solver stage: (S,5,2) point pairs with x2^T E x1 = 0 -> E (S,10,3,3) float64 of unit Frobenius norm
    in ascending root order and valid (S,10) bool."""
    _lib.require_cuda(x1, x2)
    for t in (x1, x2):
        if t.dim() != 3 or t.shape[1:] != (5, 2) or not t.is_contiguous() or t.shape != x1.shape:
            raise ValueError('pnr.relpose.five_point: x1, x2 are contiguous (S,5,2) tensors')
    x1, x2 = x1.double(), x2.double()
    S, dev = x1.shape[0], x1.device
    E = torch.empty((S, 10, 3, 3), dtype=torch.float64, device=dev)
    valid = torch.empty((S, 10), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().pnr_fivept_solve(_lib.ptr(x1), _lib.ptr(x2), S, _lib.ptr(E), _lib.ptr(valid),
                                            _lib.stream_of(dev)), 'fivept_solve')
    return E, valid.bool()


def triangulate(Tcw_1, Tcw_2, kpn_1, kpn_2, K=None):
    """`triangulate_normalized_points`: pts3d (L,3) float64 and good (L,) bool; with the (3,3) intrinsics K
    also uv1 (L,2), z1 (L,), uv2, z2: the projections K (Rcw p + tcw) into both views."""
    k1, k2 = _points('triangulate', kpn_1, kpn_2)
    dev, L = k1.device, k1.shape[0]
    _lib.require_cuda(Tcw_1, Tcw_2, K)
    T1, T2 = (T.to(torch.float64).contiguous() for T in (Tcw_1, Tcw_2))
    if T1.shape != (4, 4) or T2.shape != (4, 4) or (K is not None and K.shape != (3, 3)):
        raise ValueError('pnr.relpose.triangulate: poses are (4,4), K is (3,3)')
    Kd = None if K is None else K.to(torch.float64).contiguous()
    pts = torch.empty((L, 3), dtype=torch.float64, device=dev)
    good = torch.empty(L, dtype=torch.uint8, device=dev)
    proj = [torch.empty(s, dtype=torch.float64, device=dev) for s in ((L, 2), (L,), (L, 2), (L,))] if K is not None \
        else [None] * 4
    _lib.check(_lib.load().pnr_triangulate(_lib.ptr(T1), _lib.ptr(T2), _lib.ptr(k1), _lib.ptr(k2), L, _lib.ptr(Kd),
                                           _lib.ptr(pts), _lib.ptr(good), *[_lib.ptr(t) for t in proj],
                                           _lib.stream_of(dev)), 'triangulate')
    return (pts, good.bool()) + (tuple(proj) if K is not None else ())


def paint_pseudo_depth(uv, depth, H, W, patch):
    """The pseudo-depth map (H,W) float32 of points uv (n,2) (u column, v row) with depths (n,): include/pnr.h
    `pnr_paint_depth` states the rule."""
    _lib.require_cuda(uv, depth)
    if uv.dim() != 2 or uv.shape[1] != 2 or depth.shape != (uv.shape[0],) or patch < 0:
        raise ValueError('pnr.relpose.paint_pseudo_depth: uv is (n,2), depth (n,), patch non-negative')
    lib = _lib.load()
    nbytes = lib.pnr_paint_depth_workspace_bytes(H, W)
    if nbytes == 0:
        raise ValueError(f'pnr.relpose.paint_pseudo_depth: image size {H} x {W} is out of range')
    uv, depth = uv.double().contiguous(), depth.double().contiguous()
    out = torch.empty((H, W), dtype=torch.float32, device=uv.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=uv.device)
    _lib.check(lib.pnr_paint_depth(_lib.ptr(uv), _lib.ptr(depth), uv.shape[0], H, W, int(patch), _lib.ptr(out),
                                   _lib.ptr(ws), nbytes, _lib.stream_of(uv.device)), 'paint_depth')
    return out


def normalize_keypoints(pts, fx, fy, cx, cy):
    """Kinv [u, v, 1] of (n,2) pixel coordinates for a pinhole camera, float64 (no undistortion)."""
    p = pts.double()
    return torch.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], dim=1)


def inv_T(T):
    out = torch.eye(4, dtype=T.dtype, device=T.device)
    out[:3, :3] = T[:3, :3].t()
    out[:3, 3] = -(T[:3, :3].t() @ T[:3, 3])
    return out


def project(K, Tcw, pts):
    """src/camera.py:62-68 over Rcw p + tcw: uv (n,2), z (n,)"""
    q = (K @ (Tcw[:3, :3] @ pts.t() + Tcw[:3, 3:4])).t()
    return q[:, :2] / q[:, 2:3], q[:, 2]


TrackResult = collections.namedtuple(
    'TrackResult', 'Tcr idx_cur_inliers idx_ref_inliers depth_coord_cur depth_coord_ref depth_cur depth_ref '
    'depth_scale pose')


def track_reference(kpn_ref, kpn_cur, idxs_ref, idxs_cur, Tcw_ref, K, median_gt_depth=None, depth_scale=None,
                    **pose_args):
    """`track_reference_frame` after the matching: estimate_pose over the matched keypoints, Tcr = inv_T(Trc),
    the inliers triangulated between Tcw_cur = Tcr Tcw_ref and Tcw_ref, the median depth in the current frame
    (z[(n - 1) // 2] of the sorted depths), depth_scale -- given, or median_gt_depth / median on the first call,
    which scales the reference translation too -- applied to the translations and the points, and the
    projections K (Rcw p + tcw) into both frames.  Every inlier is kept (`good` is not applied, so the only host
    read is the inlier count).  Returns a TrackResult; Tcr carries the scaled translation."""
    if (median_gt_depth is None) == (depth_scale is None):
        raise ValueError('pnr.relpose.track_reference: give median_gt_depth (first call) or depth_scale')
    pose = estimate_pose(kpn_ref[idxs_ref].contiguous(), kpn_cur[idxs_cur].contiguous(), **pose_args)
    Tcw_ref = Tcw_ref.double()
    K = K.double()
    Tcr = inv_T(pose.Trc)
    Tcw_cur = Tcr @ Tcw_ref
    n = int(pose.num_inliers.item())
    if n == 0:
        raise RuntimeError('pnr.relpose.track_reference: no inlier matches')
    keep = torch.sort(pose.mask.to(torch.uint8), descending=True, stable=True).indices[:n]  # ascending inliers
    ic, ir = idxs_cur[keep], idxs_ref[keep]
    pts, _ = triangulate(Tcw_cur, Tcw_ref, kpn_cur[ic].contiguous(), kpn_ref[ir].contiguous())
    z = pts @ Tcw_cur[2, :3] + Tcw_cur[2, 3]
    median = torch.sort(z).values[(n - 1) // 2]
    first = depth_scale is None
    scale = median_gt_depth / median if first else torch.as_tensor(depth_scale, dtype=torch.float64, device=z.device)
    Tcw_cur = Tcw_cur.clone()
    Tcw_cur[:3, 3] *= scale
    if first:
        Tcw_ref = Tcw_ref.clone()
        Tcw_ref[:3, 3] *= scale
    Tcr = Tcr.clone()
    Tcr[:3, 3] *= scale
    pts = pts * scale
    uv1, z1 = project(K, Tcw_cur, pts)
    uv2, z2 = project(K, Tcw_ref, pts)
    return TrackResult(Tcr, ic, ir, uv1, uv2, z1, z2, scale, pose)
