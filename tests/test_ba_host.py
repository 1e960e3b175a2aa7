"""Bundle adjustment, host side (no GPU): the argument conventions of the new C entries, the
BundleAdjust bookkeeping on host tensors, and the gradient fixture tests/golden/ba_grads.npz."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, 'pointnerf-slam_amd'))

P = ctypes.c_void_p


@pytest.fixture(scope='module')
def L():
    from pnr import _lib
    return _lib.load()


def _pose_args(F=3, npf=7, ws_bytes=None, **over):
    """pnr_pose_step arguments with fake non-NULL pointers (argument errors are reported before any
    device access); `over` replaces arguments by name."""
    names = ['g_o', 'g_d', 'idx', 'F', 'npf', 'H', 'W', 'fx', 'fy', 'cx', 'cy', 'cam', 'fixed', 'm', 'v', 'lr', 'b1',
             'b2', 'eps', 'step', 'adam', 'c2w', 'g_cam', 'ws', 'ws_bytes', 'stream']
    a = dict(g_o=P(8), g_d=P(8), idx=P(8), F=F, npf=npf, H=34, W=60, fx=30., fy=30., cx=30., cy=16.5, cam=P(8),
             fixed=P(8), m=P(8), v=P(8), lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=P(8), adam=1, c2w=P(8),
             g_cam=P(8), ws=P(8), ws_bytes=0 if ws_bytes is None else ws_bytes, stream=None)
    a.update(over)
    return [a[k] for k in names]


def test_pose_step_workspace_and_arg_errors(L):
    # ticket word + one float64 partial of 12 sums per block; blocks per frame grow with the rays per frame
    one = L.pnr_pose_step_workspace_bytes(3, 7)
    assert one == 8 + 3 * 12 * 8
    assert L.pnr_pose_step_workspace_bytes(3, 257) == 8 + 3 * 2 * 12 * 8
    assert L.pnr_pose_step_workspace_bytes(5, 200) == 8 + 5 * 12 * 8
    assert L.pnr_pose_step_workspace_bytes(-1, 7) == 0 and L.pnr_pose_step_workspace_bytes(3, -1) == 0
    big = 1 << 20
    # NULL or inconsistent arguments: PNR_E_ARG
    for name in ('g_o', 'g_d', 'idx', 'cam', 'g_cam', 'ws'):
        assert L.pnr_pose_step(*_pose_args(ws_bytes=big, **{name: None})) == -1, name
    for name in ('m', 'v', 'step', 'c2w'):  # needed by the Adam step only
        assert L.pnr_pose_step(*_pose_args(ws_bytes=big, **{name: None})) == -1, name
    assert L.pnr_pose_step(*_pose_args(ws_bytes=big, F=-1)) == -1
    assert L.pnr_pose_step(*_pose_args(ws_bytes=big, npf=-1)) == -1
    assert L.pnr_pose_step(*_pose_args(ws_bytes=big, adam=2)) == -1
    assert L.pnr_pose_step(*_pose_args(ws_bytes=big, W=0)) == -1
    assert L.pnr_pose_step(*_pose_args(ws_bytes=big, fx=0.)) == -1
    assert L.pnr_pose_step(*_pose_args(ws_bytes=big, ws=P(12))) == -1  # the ticket word needs 8-byte alignment
    # a short workspace: PNR_E_WORKSPACE
    assert L.pnr_pose_step(*_pose_args(ws_bytes=one - 1)) == -2
    # no rays: a no-op that leaves the poses untouched (nothing is dereferenced: every pointer NULL)
    nul = dict(g_o=None, g_d=None, idx=None, cam=None, fixed=None, m=None, v=None, step=None, c2w=None, g_cam=None,
               ws=None)
    assert L.pnr_pose_step(*_pose_args(F=0, **nul)) == 0
    assert L.pnr_pose_step(*_pose_args(npf=0, **nul)) == 0


def test_map_ray_gradient_entries_arg_errors(L):
    from pnr import _lib
    mp = _lib.RenderParams()
    mp.n_samples, mp.n_importance, mp.precision = 32, 12, 3
    arr = _lib.PtrArray(*([8] * _lib.N_PARAMS))
    # pnr_map_bwd_rays: the ray-gradient outputs and the regulation inputs are required
    base = dict(prm=ctypes.byref(mp), packed=P(8), rays_d=P(8), gt=P(8), t_rand=P(8), n=10, g_depth=P(8), g_rgb=P(8),
                g_sigma=P(8), grads=arr, g_ro=P(8), g_rd=P(8), ws=P(8), ws_bytes=0, bws=P(8), bws_bytes=0, stream=None)

    def bwd(**over):
        a = dict(base)
        a.update(over)
        return L.pnr_map_bwd_rays(*a.values())
    assert bwd(g_ro=None) == -1 and bwd(g_rd=None) == -1
    assert bwd(gt=None) == -1 and bwd(t_rand=None) == -1
    assert bwd(packed=None) == -1 and bwd(n=-1) == -1 and bwd(ws=None) == -1
    assert bwd() == -2  # every pointer given, workspaces of zero bytes: PNR_E_WORKSPACE
    assert bwd(n=0, g_ro=None) == -1
    assert bwd(n=0, gt=None, t_rand=None) == 0  # no rays, accumulate semantics: a no-op
    bad = _lib.RenderParams()
    bad.n_samples, bad.n_importance = 40, 30
    assert bwd(prm=ctypes.byref(bad)) == -1
    # pnr_map_step_rays: pnr_map_step's conditions plus the ray-gradient outputs
    sbase = dict(prm=ctypes.byref(mp), packed=P(8), ro=P(8), rd=P(8), gt=P(8), gc=P(8), t_rand=P(8), n=10, wc=0.05,
                 wr=5e-4, loss=P(8), grads=arr, ws=P(8), ws_bytes=0, bws=P(8), bws_bytes=0, lws=P(8), tail=None,
                 fused=None, g_ro=P(8), g_rd=P(8), stream=None)

    def step(**over):
        a = dict(sbase)
        a.update(over)
        return L.pnr_map_step_rays(*a.values())
    assert step(g_ro=None) == -1 and step(g_rd=None) == -1
    assert step(loss=None) == -1 and step(lws=None) == -1 and step(t_rand=None) == -1
    assert step() == -2
    tail = _lib.AdamTail()  # a tail without its step counter / scales area, or without `fused`
    assert step(tail=ctypes.byref(tail), fused=ctypes.byref(ctypes.c_int32(0))) == -1


def _host_window(F=3, H=6, W=8):
    from pnr.mapping import WindowSampler
    s = load_golden('scene.npz')
    frames = [(torch.from_numpy(s['poses'][f]).float(), torch.ones(H, W), torch.zeros(H, W, 3)) for f in range(F)]
    return WindowSampler(frames, 5, 8., 8., 4., 3., device_rng=False), frames


def test_bundle_adjust_bookkeeping():
    """On host tensors (no kernel call): the fixed set, the table aliasing, poses() / camera_tensors()."""
    import pnr
    sampler, frames = _host_window()
    before = sampler.c2w.clone()
    ba = pnr.BundleAdjust(sampler, 1e-3)
    assert ba.fixed == (0,) and ba.fixed_mask.tolist() == [1, 0, 0]  # the oldest frame (src/Mapper.py:464-465)
    assert ba.c2w is sampler.c2w and ba.c2w.data_ptr() == sampler.c2w.data_ptr()
    assert ba.poses().shape == (3, 4, 4) and ba.camera_tensors().shape == (3, 7)
    assert ba.poses().data_ptr() != sampler.c2w.data_ptr()  # the write-back gets a copy
    assert ba.m.shape == ba.v.shape == ba.g_cam.shape == (3, 7) and not ba.m.any() and not ba.g_cam.any()
    assert int(ba.step_dev[0]) == 0
    # the fixed frame's row is untouched bit for bit; the others are get_camera_from_tensor of their tensors
    assert torch.equal(sampler.c2w[0], before[0])
    np.testing.assert_allclose(sampler.c2w.numpy(), before.numpy(), atol=2e-6)
    got = pnr.get_camera_from_tensor(ba.camera_tensors()[1:])
    assert torch.equal(sampler.c2w[1:, :3, :], got)
    assert torch.equal(sampler.c2w[:, 3, :], torch.tensor([0., 0., 0., 1.]).expand(3, 4))
    np.testing.assert_allclose(ba.camera_tensors()[2].numpy(), pnr.get_tensor_from_camera(frames[2][0]).numpy(),
                               atol=1e-7)
    # new tensors (non-unit quaternions) reach the sampler's own table, except the fixed frame's row
    cam = ba.camera_tensors() + 0.003
    ba.set_camera_tensors(cam)
    assert torch.equal(ba.camera_tensors(), cam)
    assert torch.equal(sampler.c2w[0], before[0])
    assert torch.equal(sampler.c2w[1:, :3, :], pnr.get_camera_from_tensor(cam[1:]))
    ba2 = pnr.BundleAdjust(_host_window()[0], 1e-3, fixed=(0, -1))
    assert ba2.fixed == (0, 2) and ba2.fixed_mask.tolist() == [1, 0, 1]
    ba3 = pnr.BundleAdjust(_host_window()[0], 1e-3, fixed=())
    assert ba3.fixed == () and not ba3.fixed_mask.any()


def test_bundle_adjust_refuses_host_tensors_and_foreign_batches():
    """No quiet fall-back: the pose step on host tensors raises, and so do ray gradients that do not
    match the sampler's last batch."""
    import pnr
    sampler, _ = _host_window()
    ba = pnr.BundleAdjust(sampler, 1e-3)
    g = torch.zeros(15, 3)
    with pytest.raises(ValueError):  # no batch drawn yet
        ba.step(g, g)
    sampler.idx = torch.zeros(15, dtype=torch.int64)
    with pytest.raises(ValueError):
        ba.step(g[:14], g[:14])
    with pytest.raises(RuntimeError, match='HIP path only'):
        ba.step(g, g)


def test_window_sampler_keeps_idx_in_both_rng_modes():
    import inspect
    from pnr.mapping import WindowSampler
    src = inspect.getsource(WindowSampler.__call__)
    assert src.count('self.idx = ') == 2  # the torch-RNG branch and the device-RNG branch


def test_ba_fixture():
    """tests/golden/ba_grads*.npz: the contents the GPU tests rely on, and float32 vs correctly rounded
    within the recorded ratio.  (Three files: one form of the decoder gradient alone is 892 KB.)"""
    G = {**load_golden('ba_grads.npz'), **load_golden('ba_grads_dec_f32.npz'), **load_golden('ba_grads_dec_cr.npz')}
    for name in ('ba_grads.npz', 'ba_grads_dec_f32.npz', 'ba_grads_dec_cr.npz'):
        assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', name)) < (1 << 20), name
    H, W, fx, fy, cx, cy = G['intrinsics']
    n = int(G['n_per_frame'])
    assert G['cam'].shape == (3, 7) and G['idx'].shape == (3 * n,) and G['idx'].dtype == np.int64
    assert G['gt_depth'].shape == (3 * n,) and G['gt_color'].shape == (3 * n, 3) and G['t_rand'].shape == (3 * n, 32)
    assert (G['idx'] >= 0).all() and (G['idx'] < H * W).all()
    qn = np.linalg.norm(G['cam'][:, :4], axis=1)
    assert (np.abs(qn - 1) > 1e-4).all()  # NOT unit quaternions
    d = np.abs(G['cam'] - G['cam_true'])
    assert d.max() < 5e-3 and d.min() > 5e-4
    assert (G['gt_depth'] == 0).sum() >= 3
    assert ((G['idx'].reshape(3, n) % int(W)) == cx).any()  # a camera-frame direction with a zero x component
    np.testing.assert_allclose(G['loss_f32'], G['loss_cr'], rtol=1e-5)
    names = [k[len('grad_cr/'):] for k in G if k.startswith('grad_cr/')]
    assert len(names) == 12 and 'cam' in names  # the camera tensors and the 11 decoder tensors
    for k in names:
        cr, f32, ratio = G['grad_cr/' + k], G['grad_f32/' + k], float(G['golden_vs_cr/' + k])
        assert cr.shape == f32.shape and np.isfinite(cr).all() and np.abs(cr).max() > 0
        assert ratio < 1e-4, (k, ratio)
        assert np.abs(f32 - cr).max() <= ratio * np.abs(cr).max() * (1 + 1e-6), k
    assert G['grad_cr/cam'].shape == (3, 7) and (np.abs(G['grad_cr/cam']).max(1) > 0).all()
