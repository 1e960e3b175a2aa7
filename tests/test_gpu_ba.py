"""Bundle adjustment in the Mapper step (mapping.BA, src/Mapper.py:460-500, 567-581, 675-692) on the GPU.

  1  the map pass's ray gradients = pnr_render_bwd + pnr_regulation_bwd (need_ray_grads) summed
  2  the decoder gradient and the loss do not change when `ba` is set (bitwise)
  3  pnr_pose_step alone against float64 autograd, its determinism, fixed frames, frame boundaries
  4  the camera gradient of one BA MapStep against the oracle fixture (tests/golden/ba_grads.npz)
  5  one camera Adam step = torch.optim.Adam on the autograd gradient of MapStep.loss
  6  eager = rerun = graph replay, bit for bit
  7  30 BA iterations move perturbed poses back towards the rendering poses
  8  refusals

Bounds: gradients elementwise rtol 1e-3 + atol 1e-6 max|g| (GRAD_RTOL / GRAD_ATOL of
tests/test_gpu_parity.py); the pose kernel's own float64 sums within 1e-6 |g| + 64 ulp(M), M the
element's sum of absolute terms (MAG_ULPS of tests/test_gpu_points.py).
"""
import types

import numpy as np
import pytest
import torch

from conftest import golden_params, load_golden

pytestmark = pytest.mark.gpu

GRAD_RTOL, GRAD_ATOL = 1e-3, 1e-6
MAG_ULPS = 64.0


@pytest.fixture(params=['fp32', 'f16x3'])
def precision(request, monkeypatch):
    """Both decoder precisions (include/pnr.h PNR_PREC_*), as tests/test_gpu_parity.py runs them."""
    from pnr import _lib
    monkeypatch.setattr(_lib, 'DEFAULT_PRECISION', request.param)
    return request.param


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def pnr_mod():
    import pnr
    pnr.library()
    return pnr


@pytest.fixture(scope='module')
def fix():
    G = load_golden('ba_grads.npz')
    H, W, fx, fy, cx, cy = G['intrinsics']
    G['hw'] = (int(H), int(W))
    G['k'] = (float(fx), float(fy), float(cx), float(cy))
    return G


def _renderer(pnr, hw=(680, 1200), k=(600., 600., 599.5, 339.5), precision=None):
    bound = torch.from_numpy(load_golden('scene.npz')['bound'])
    slam = types.SimpleNamespace(bound=bound, H=hw[0], W=hw[1], fx=k[0], fy=k[1], cx=k[2], cy=k[3])
    r = pnr.Renderer(pnr.ROOM0_CFG, None, slam)
    if precision is not None:
        r.precision = precision
    return r


def _decoder(pnr, dev):
    dec = pnr.get_model(pnr.ROOM0_CFG, nice=False)
    dec.load_state_dict({k: v.clone() for k, v in golden_params('trained').items()})
    return dec.to(dev)


def grad_elementwise(g, cr, f32, rel_f32, what):
    """tests/test_gpu_parity.py's rule: |g - g_cr| <= 1e-3 |g_cr| + 1e-6 max|g_cr| elementwise, and
    |g - g_f32| <= 1e-3 |g_f32| + (1e-6 + rel_f32) max|g_f32|."""
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    for ref, atol_rel, tag in ((cr, GRAD_ATOL, 'correctly rounded'), (f32, GRAD_ATOL + float(rel_f32), 'float32')):
        ref = np.asarray(ref)
        atol = atol_rel * np.abs(ref).max()
        viol = np.abs(g - ref) / (GRAD_RTOL * np.abs(ref) + atol)
        print(f'{what} vs {tag}: worst |g - g_ref| / (rtol |g_ref| + atol) = {viol.max():.3f}')
        np.testing.assert_allclose(g, ref, rtol=GRAD_RTOL, atol=atol, err_msg=f'{what} vs {tag}')


@pytest.fixture(scope='module')
def window(pnr_mod, dev, fix):
    """The fixture's window rendered on the device (fp32) at the TRUE poses: (poses (3,4,4), depth
    (3,H,W) with every 7th row / 5th column zeroed, colour (3,H,W,3), the true camera tensors)."""
    (H, W), k = fix['hw'], fix['k']
    r = _renderer(pnr_mod, (H, W), k, precision='fp32')
    dec = _decoder(pnr_mod, dev)
    poses = torch.from_numpy(load_golden('scene.npz')['poses'][:3]).float()
    depth, color = [], []
    for c2w in poses:
        d, _, c = r.render_img({}, dec, c2w.to(dev), dev, 'color')
        d = d.float().clone()
        d[::7, ::5] = 0.
        depth.append(d)
        color.append(c.float())
    return poses, torch.stack(depth), torch.stack(color), torch.from_numpy(fix['cam_true'])


def _perturbed_sampler(pnr, dev, fix, window, per, seed=5, device_rng=True):
    """A WindowSampler over the window with its poses perturbed as the fixture perturbs them."""
    _, depth, color, _ = window
    cam0 = torch.from_numpy(fix['cam'])
    bottom = torch.tensor([[0., 0., 0., 1.]])
    frames = [(torch.cat([pnr.get_camera_from_tensor(cam0[f]), bottom], 0).to(dev), depth[f], color[f])
              for f in range(3)]
    return pnr.WindowSampler(frames, per, *fix['k'], n_samples=32, seed=seed, device_rng=device_rng)


# ---- 1. the map pass's ray gradients ----------------------------------------------------------------

def _golden_rays(dev, n):
    r = load_golden('render.npz')
    ro = torch.from_numpy(r['p2_gt/rays_o'])[:n].clone()
    rd = torch.from_numpy(r['p2_gt/rays_d'])[:n].clone()
    gt = torch.from_numpy(r['p2_gt/gt_depth'])[:n].clone()
    gt[::9] = 0.  # a few zero-depth pixels: their regulation samples all sit at the ray origin
    return ro.to(dev), rd.to(dev), gt.to(dev)


def _zero_views(ms):
    """Gradient buffers shaped like a MapStep's flat views (decoder, fc_c, features)."""
    buf = torch.zeros_like(ms.flat.grad)
    return ms._split(buf)


def _ray_grads_both_ways(pnr, dev, ms, ro, rd, gt, seed):
    """(map pass ray gradients, render + regulation ray gradients) for the same upstream gradients."""
    from pnr.renderer import MapPass, TrainPass
    n = ro.shape[0]
    gen = torch.Generator().manual_seed(seed)
    t_rand = torch.rand((n, 32), generator=gen).to(dev)
    g_d = torch.randn(n, generator=gen, dtype=torch.float64).to(dev)
    g_c = torch.randn((n, 3), generator=gen).to(dev)
    g_s = (1e-3 * torch.randn(n * 32, generator=gen)).to(dev)
    r, c, dec = ms.renderer, ms.c, ms.decoder
    mp = MapPass(r, c, dec)
    mp.forward(ro, rd, gt, t_rand)
    v = _zero_views(ms)
    got = torch.full((2, n, 3), float('nan'), device=dev)
    mp.backward(v[0], g_fc=v[1], g_feats=v[2], g_depth=g_d, g_rgb=g_c, g_sigma=g_s, ray_grads=got)
    ref = torch.full((2, 2, n, 3), float('nan'), device=dev)
    ren = TrainPass(r, c, dec, 'render')
    ren.forward(ro, rd, gt)
    v = _zero_views(ms)
    ren.backward(v[0], g_fc=v[1], g_feats=v[2], g_depth=g_d, g_rgb=g_c, ray_grads=ref[0])
    reg = TrainPass(r, c, dec, 'regulation')
    reg.forward(ro, rd, gt, t_rand=t_rand)
    v = _zero_views(ms)
    reg.backward(v[0], g_fc=v[1], g_feats=v[2], g_sigma=g_s, ray_grads=ref[1])
    torch.cuda.synchronize()
    return got.cpu().double(), (ref[0].cpu().double() + ref[1].cpu().double())


def _check_ray_grads(got, ref, what):
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    for k, name in enumerate(('g_rays_o', 'g_rays_d')):
        g, e = got[k].numpy(), ref[k].numpy()
        atol = GRAD_ATOL * np.abs(e).max()
        viol = np.abs(g - e) / (GRAD_RTOL * np.abs(e) + atol)
        print(f'{what} {name}: max|ref| = {np.abs(e).max():.3e}, worst violation ratio = {viol.max():.3f}')
        assert np.abs(e).max() > 0
        np.testing.assert_allclose(g, e, rtol=GRAD_RTOL, atol=atol, err_msg=f'{what} {name}')


@pytest.mark.parametrize('n', [21, 192, 195])
def test_map_pass_ray_grads_equal_two_backwards(pnr_mod, dev, precision, n):
    """21 = 3 x 7 rays (ragged against the 16- and 32-point tiles), 3 x 64 and 3 x 65."""
    from pnr.mapping import MapStep
    ms = MapStep(_renderer(pnr_mod), _decoder(pnr_mod, dev))
    ro, rd, gt = _golden_rays(dev, n)
    got, ref = _ray_grads_both_ways(pnr_mod, dev, ms, ro, rd, gt, seed=n)
    _check_ray_grads(got, ref, f'n={n} {precision}')


def test_map_pass_ray_grads_with_points(pnr_mod, dev, precision):
    """Neural points (the surface_cloud setup of tests/test_gpu_points.py, 200 rays): the gather backward
    adds its dL/dp into the delta chain's dL/dx before the ray reduction."""
    from oracle import ref_points as RP
    from pnr.mapping import MapStep
    n = 200
    ro, rd, gt = _golden_rays(dev, n)
    gen = torch.Generator().manual_seed(4)
    surf = (ro + rd * gt[:, None]).cpu()
    xyz = (surf.repeat(4, 1) + 0.01 * torch.randn((4 * n, 3), generator=gen)).float()
    feats = torch.randn((xyz.shape[0], 32), generator=gen) * 0.5
    dec = pnr_mod.MLP(name='color', dim=3, c_dim=32, color=True, skips=[], n_blocks=4, hidden_size=256)
    dec.load_state_dict({k: v.clone() for k, v in RP.init_fc_c(golden_params('trained'), seed=1).items()})
    pts = pnr_mod.NeuralPoints(xyz.to(dev), feats.to(dev), mode='idw', radius=0.04, k=8).to(dev)
    ms = MapStep(_renderer(pnr_mod), dec.to(dev), points=pts, feat_lr=1e-2)
    got, ref = _ray_grads_both_ways(pnr_mod, dev, ms, ro, rd, gt, seed=3)
    _check_ray_grads(got, ref, f'points {precision}')
    # the hand-in matters: without the points the same rays give another gradient
    plain = MapStep(_renderer(pnr_mod), _decoder(pnr_mod, dev))
    other, _ = _ray_grads_both_ways(pnr_mod, dev, plain, ro, rd, gt, seed=3)
    assert (other - got).abs().max() > 1e-3 * got.abs().max()


# ---- 2. the decoder's gradient is untouched -----------------------------------------------------------

@pytest.mark.parametrize('path', ['one_call', 'fused', 'two_chain', 'two_chain_serial'])
def test_decoder_grads_unchanged_by_ba(pnr_mod, dev, precision, fix, window, path):
    from pnr.mapping import MapStep
    out = []
    for with_ba in (False, True):
        sampler = _perturbed_sampler(pnr_mod, dev, fix, window, 65)
        # (made either way: it rewrites the free frames' table rows from their tensors, so both runs draw
        # the same batch; only the second step is given it)
        ba = pnr_mod.BundleAdjust(sampler, 1e-3)
        kw = {'two_chain': dict(fused=False, overlap=True), 'two_chain_serial': dict(fused=False, overlap=False)}
        ms = MapStep(_renderer(pnr_mod), _decoder(pnr_mod, dev), ba=ba if with_ba else None, **kw.get(path, {}))
        ms.one_call = path == 'one_call'
        ms.opt.use_device_step()
        loss = ms(*sampler())
        torch.cuda.synchronize()
        out.append((loss.detach().cpu().clone(), ms.flat.grad.cpu().clone(), ms.flat.data.cpu().clone(),
                    ms.tail_fused))
        if with_ba:
            assert (ba.g_cam[0] == 0).all() and (ba.g_cam[1:].abs().amax(1) > 0).all()
            assert int(ba.step_dev[0]) == 1
            assert not torch.equal(ba.camera_tensors()[1:].cpu(), torch.from_numpy(fix['cam'])[1:])
            g_cam = ba.g_cam.cpu().clone()
    (l0, g0, w0, t0), (l1, g1, w1, t1) = out
    assert t0 == t1 == (path == 'one_call' and precision == 'f16x3')  # the fused tail stays eligible
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(g0, g1), int((g0 != g1).sum())
    assert torch.equal(w0, w1)
    print(f'{path} {precision}: g_cam rows 1, 2 =', g_cam[1:].numpy())


# ---- 3. the pose kernel alone ------------------------------------------------------------------------

POISON = 0x7FC0DEAD  # a NaN pattern no arithmetic produces


def _pose_inputs(pnr, dev, F, npf, seed):
    gen = torch.Generator().manual_seed(seed)
    H, W, fx, fy, cx, cy = 34, 60, 30., 30., 30., 16.5
    poses = torch.from_numpy(load_golden('scene.npz')['poses']).float()
    cam = torch.stack([pnr.get_tensor_from_camera(poses[f % 4]) for f in range(F)])
    cam = cam + 0.05 * torch.randn((F, 7), generator=gen)  # non-unit quaternions
    n = F * npf
    idx = torch.randint(0, H * W, (n,), generator=gen)
    g_o = torch.randn((n, 3), generator=gen)
    g_d = torch.randn((n, 3), generator=gen)
    return dict(F=F, npf=npf, H=H, W=W, k=(fx, fy, cx, cy), cam=cam, idx=idx, g_o=g_o, g_d=g_d)


def _pose_reference(pnr, a):
    """float64 autograd through pnr.common.get_camera_from_tensor and the _RaysFromUV adjoint (dL/dt =
    sum g_o, dL/dR = g_d^T dirs), and M = each element's sum of absolute terms."""
    F, npf, W = a['F'], a['npf'], a['W']
    fx, fy, cx, cy = a['k']
    i = (a['idx'] % W).double()
    j = torch.div(a['idx'], W, rounding_mode='floor').double()
    dirs = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1).reshape(F, npf, 3)
    g_o = a['g_o'].double().reshape(F, npf, 3)
    g_d = a['g_d'].double().reshape(F, npf, 3)
    cam = a['cam'].double().clone().requires_grad_(True)
    RT = pnr.get_camera_from_tensor(cam)  # (F,3,4)
    G = torch.einsum('fri,frj->fij', g_d, dirs)
    ((RT[:, :, :3] * G).sum() + (RT[:, :, 3] * g_o.sum(1)).sum()).backward()
    Gabs = torch.einsum('fri,frj->fij', g_d.abs(), dirs.abs())
    M = torch.zeros(F, 7, dtype=torch.float64)
    for f in range(F):
        J = torch.autograd.functional.jacobian(lambda q: pnr.quad2rotation(q[None])[0], a['cam'][f, :4].double())
        M[f, :4] = (Gabs[f][:, :, None] * J.abs()).sum((0, 1))
        M[f, 4:] = g_o[f].abs().sum(0)
    return cam.grad.detach(), M


def _run_pose_step(dev, a, fixed, adam, state=None, lr=1e-3):
    """One pnr_pose_step on copies of the inputs; returns the written state (on the host)."""
    from pnr import _lib
    L = _lib.load()
    F, npf = a['F'], a['npf']
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    cam = a['cam'].clone().to(dev)
    m = torch.zeros(F, 7, device=dev) if state is None else state['m'].clone().to(dev)
    v = torch.zeros(F, 7, device=dev) if state is None else state['v'].clone().to(dev)
    c2w = torch.zeros(F, 4, 4, device=dev)
    for f in fixed:  # a fixed frame's rows keep whatever is there
        for t in (cam, m, v, c2w):
            i32(t[f]).fill_(POISON)
    g_cam = torch.full((F, 7), float('nan'), device=dev)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    mask = torch.zeros(F, dtype=torch.uint8)
    for f in fixed:
        mask[f] = 1
    mask = mask.to(dev)
    ws = torch.zeros(L.pnr_pose_step_workspace_bytes(F, npf), dtype=torch.uint8, device=dev)
    g_o, g_d, idx = a['g_o'].to(dev), a['g_d'].to(dev), a['idx'].to(dev)
    for _ in range(1 if adam else 2):  # gradient-only: a second call on the same workspace (left zero-filled)
        _lib.check(L.pnr_pose_step(_lib.ptr(g_o), _lib.ptr(g_d), _lib.ptr(idx), F, npf, a['H'], a['W'], *a['k'],
                                   _lib.ptr(cam), _lib.ptr(mask) if fixed else None, _lib.ptr(m), _lib.ptr(v), lr,
                                   0.9, 0.999, 1e-8, _lib.ptr(step), 1 if adam else 0, _lib.ptr(c2w),
                                   _lib.ptr(g_cam), _lib.ptr(ws), ws.numel(), _lib.stream_of(dev)), 'pose_step')
    torch.cuda.synchronize()
    assert not ws[:8].any()  # the ticket word is zero again (the partials behind it are scratch)
    return {k: t.cpu() for k, t in dict(cam=cam, m=m, v=v, c2w=c2w, g_cam=g_cam, step=step).items()}


@pytest.mark.parametrize('npf', [1, 7, 64, 65, 200, 257])
@pytest.mark.parametrize('F', [1, 2, 5])
def test_pose_step_alone(pnr_mod, dev, F, npf):
    a = _pose_inputs(pnr_mod, dev, F, npf, seed=100 * F + npf)
    if F > 1:  # frame 1's gradients all zero: a ray leaking over a frame boundary would show in its row
        a['g_o'][npf:2 * npf] = 0
        a['g_d'][npf:2 * npf] = 0
    fixed = (0,) if F > 1 else ()
    free = [f for f in range(F) if f not in fixed]
    g64, M = _pose_reference(pnr_mod, a)
    i32 = lambda t: t.contiguous().view(torch.int32)  # noqa: E731

    # gradient-only mode: nothing but g_cam is written
    go = _run_pose_step(dev, a, fixed, adam=False)
    err = (go['g_cam'].double() - g64).abs()
    bound = 1e-6 * g64.abs() + MAG_ULPS * 2.0 ** -24 * M
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * float('inf'))[free]
    print(f'F={F} npf={npf}: worst |g - g64| / bound = {ratio.max():.3f}')
    assert (err[free] <= bound[free]).all(), ratio.max()
    for f in fixed:
        assert (go['g_cam'][f] == 0).all()
        for k in ('cam', 'm', 'v', 'c2w'):
            assert (i32(go[k][f]) == POISON).all(), k
    if F > 1:
        assert (go['g_cam'][1] == 0).all()
    assert torch.equal(go['cam'][free], a['cam'][free]) and not go['m'][free].any() and not go['c2w'][free].any()
    assert int(go['step'][0]) == 3

    # with the Adam step, twice from the same state: bitwise equal
    r1 = _run_pose_step(dev, a, fixed, adam=True)
    r2 = _run_pose_step(dev, a, fixed, adam=True)
    for k in r1:
        assert torch.equal(i32(r1[k]) if r1[k].dtype == torch.float32 else r1[k],
                           i32(r2[k]) if r2[k].dtype == torch.float32 else r2[k]), k
    assert torch.equal(i32(r1['g_cam']), i32(go['g_cam']))
    assert int(r1['step'][0]) == 4
    for f in fixed:
        for k in ('cam', 'm', 'v', 'c2w'):
            assert (i32(r1[k][f]) == POISON).all(), k
    # torch.optim.Adam's step number 4 from zero moments on the kernel's own gradient
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    g = go['g_cam'][free].double()
    mh = (1 - b1) * g / (1 - b1 ** 4)
    vh = (1 - b2) * g * g / (1 - b2 ** 4)
    want = a['cam'][free].double() - lr * mh / (vh.sqrt() + eps)
    assert ((r1['cam'][free].double() - want).abs() <= 1e-3 * lr).all()
    if F > 1:  # frame 1: zero gradient, so no movement
        assert torch.equal(r1['cam'][1], a['cam'][1])
    RT = pnr_mod.get_camera_from_tensor(r1['cam'][free])
    np.testing.assert_allclose(r1['c2w'][free][:, :3, :].numpy(), RT.numpy(), rtol=0, atol=1e-6)
    assert torch.equal(r1['c2w'][free][:, 3, :], torch.tensor([0., 0., 0., 1.]).expand(len(free), 4))


# ---- 4. / 5. one BA MapStep on the fixture batch ---------------------------------------------------------

def _fixture_step(pnr, dev, fix, cam_lr):
    """(MapStep, BundleAdjust, sampler, batch) with the fixture's camera tensors, pixels, gt and jitter."""
    from pnr.mapping import MapStep, window_rays
    (H, W), n = fix['hw'], int(fix['n_per_frame'])
    cam = torch.from_numpy(fix['cam'])
    bottom = torch.tensor([[0., 0., 0., 1.]])
    frames = [(torch.cat([pnr.get_camera_from_tensor(cam[f]), bottom], 0).to(dev), torch.zeros(H, W, device=dev),
               torch.zeros(H, W, 3, device=dev)) for f in range(3)]
    sampler = pnr.WindowSampler(frames, n, *fix['k'], n_samples=32, device_rng=False)
    ba = pnr.BundleAdjust(sampler, cam_lr)
    ba.set_camera_tensors(cam)
    idx = torch.from_numpy(fix['idx']).to(dev)
    ro, rd, _, _ = window_rays(idx, n, sampler.c2w, sampler.depth, sampler.color, *fix['k'])
    sampler.idx = idx
    batch = (ro, rd, torch.from_numpy(fix['gt_depth']).to(dev), torch.from_numpy(fix['gt_color']).to(dev),
             torch.from_numpy(fix['t_rand']).to(dev))
    ms = MapStep(_renderer(pnr, (H, W), fix['k']), _decoder(pnr, dev), ba=ba)
    return ms, ba, sampler, batch


def test_camera_gradient_vs_oracle(pnr_mod, dev, precision, fix):
    """ba.g_cam of one BA MapStep (cam_lr = 0) against the fixture's correctly-rounded and float32
    camera gradients; the loss at rtol 1e-4; the fixed frame's row exactly zero.  The decoder's
    gradient of the same step at the per-tensor bound of tests/test_gpu_parity.py (2e-3 max|g|)."""
    ms, ba, sampler, batch = _fixture_step(pnr_mod, dev, fix, 0.0)
    loss = ms(*batch)
    torch.cuda.synchronize()
    print(f'loss {float(loss)!r} against f32 {float(fix["loss_f32"])!r}, cr {float(fix["loss_cr"])!r}')
    print('g_cam', ba.g_cam.cpu().numpy())
    np.testing.assert_allclose(float(loss), float(fix['loss_f32']), rtol=1e-4)
    assert (ba.g_cam[0] == 0).all()
    grad_elementwise(ba.g_cam[1:], fix['grad_cr/cam'][1:], fix['grad_f32/cam'][1:], fix['golden_vs_cr/cam'],
                     f'camera tensor grad ({precision})')
    assert torch.equal(ba.camera_tensors().cpu(), torch.from_numpy(fix['cam']))  # cam_lr = 0
    D = load_golden('ba_grads_dec_cr.npz')
    for name, g in zip(pnr_mod.PARAM_ORDER, ms._views['main'][0]):
        ref = D['grad_cr/' + name]
        np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=0, atol=2e-3 * np.abs(ref).max(), err_msg=name)


def test_one_adam_step_equals_torch(pnr_mod, dev, precision, fix):
    lr = 1e-3
    ms, ba, sampler, batch = _fixture_step(pnr_mod, dev, fix, lr)
    c2w0 = sampler.c2w.clone()
    # torch.optim.Adam on the autograd gradient of MapStep.loss in its camera-tensor form
    ref, ref_ba, _, _ = _fixture_step(pnr_mod, dev, fix, lr)
    ct = torch.from_numpy(fix['cam']).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([ct], lr=lr)
    l_ref = ref.loss(None, None, *batch[2:], camera_tensors=ct, idx=sampler.idx)
    l_ref.backward()
    assert (ct.grad[0] == 0).all()  # the fixed frame is detached
    opt.step()
    loss = ms(*batch)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss), float(l_ref), rtol=1e-4)
    got = ba.camera_tensors()
    d = (got - ct.detach()).abs()
    print(f'worst |stepped - torch| / cam_lr = {float(d.max()) / lr:.2e}; autograd vs kernel gradient:',
          float((ct.grad - ba.g_cam).abs().max() / ct.grad.abs().max()))
    assert (d <= 1e-3 * lr).all(), d / lr
    assert ((got[1:] - torch.from_numpy(fix['cam']).to(dev)[1:]).abs() > 0.5 * lr).all()  # Adam's first step ~ lr
    assert torch.equal(got[0].cpu(), torch.from_numpy(fix['cam'])[0])
    # the sampler's own table: rewritten from the stepped tensors, the fixed frame's row untouched
    RT = pnr_mod.get_camera_from_tensor(got)
    np.testing.assert_allclose(sampler.c2w[1:, :3, :].cpu().numpy(), RT[1:].cpu().numpy(), rtol=0, atol=1e-6)
    assert torch.equal(sampler.c2w[:, 3, :].cpu(), torch.tensor([0., 0., 0., 1.]).expand(3, 4))
    assert torch.equal(sampler.c2w[0], c2w0[0])
    assert not torch.equal(sampler.c2w[1:], c2w0[1:])
    assert ba.poses().shape == (3, 4, 4) and torch.equal(ba.poses(), sampler.c2w)


# ---- 6. eager = rerun = graph replay ---------------------------------------------------------------------

def _ba_schedule(pnr, dev, fix, window, schedule):
    """Two warm-up iterations and three more under one schedule; the state after each of the three."""
    from pnr.mapping import MapGraph, MapStep
    sampler = _perturbed_sampler(pnr, dev, fix, window, 65, seed=9)
    ba = pnr.BundleAdjust(sampler, 1e-3)
    ms = MapStep(_renderer(pnr), _decoder(pnr, dev), ba=ba)
    ms.opt.use_device_step()
    states = []

    def state(loss):
        torch.cuda.synchronize()
        return [t.detach().cpu().clone() for t in (loss, ms.flat.data, ba.cam, ba.m, ba.v, ba.g_cam, sampler.c2w,
                                                   ba.step_dev, ms.opt.step_dev)]
    if schedule == 'graph':
        mg = MapGraph(ms, batch_fn=sampler, warmup=2)
        for _ in range(3):
            states.append(state(mg()))
    else:
        sampler()  # MapGraph draws one batch to find the device
        for _ in range(2):
            ms(*sampler())
        for _ in range(3):
            states.append(state(ms(*sampler())))
    return states, ms.tail_fused


STATE_NAMES = ('loss', 'decoder', 'cam', 'm', 'v', 'g_cam', 'c2w', 'camera step', 'decoder step')


def _assert_same_states(a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(STATE_NAMES, x, y):
            assert torch.equal(u, v), f'{tag} iteration {k}: {name} differs in {int((u != v).sum())} elements'


def test_ba_eager_equals_rerun(pnr_mod, dev, precision, fix, window):
    """Three BA iterations (after two warm-up ones) run twice from the same state: decoder parameters,
    camera tensors and moments, the pose table and the losses bitwise equal after every iteration."""
    (a, fused), (b, _) = (_ba_schedule(pnr_mod, dev, fix, window, s) for s in ('eager', 'rerun'))
    assert fused == (precision == 'f16x3')
    _assert_same_states(a, b, 'rerun')
    assert int(a[-1][7][0]) == 5 and int(a[-1][8][0]) == 5
    assert not torch.equal(a[0][2], a[2][2])  # the poses did move between iterations


def test_ba_eager_equals_graph_replay(pnr_mod, dev, precision, fix, window):
    """The same iterations as MapGraph replays (the warm-up accounting of test_map_graph_matches_eager),
    bitwise equal to the eager ones.
    Under fp32 this also holds the zero fill of the stored gradients to its word: as eleven memset
    nodes it replayed, from the second replay of a sampler-driven graph on, with 69 or 138 wrong words
    in dL/d(embedder._B) (with `ba=None` too); it is one kernel now (capi.cpp zero_weight_grads)."""
    (a, _), (b, fused) = (_ba_schedule(pnr_mod, dev, fix, window, s) for s in ('eager', 'graph'))
    assert fused == (precision == 'f16x3')
    _assert_same_states(a, b, 'graph')
    assert int(b[-1][7][0]) == 5 and int(b[-1][8][0]) == 5


# ---- 7. it converges -------------------------------------------------------------------------------------

def test_ba_converges(pnr_mod, dev, fix, window):
    """The window rendered at the true poses, the two free poses perturbed as the fixture perturbs them,
    30 BA iterations at cam_lr 1e-3 (configs/nice_slam.yaml): the mean |camera tensor - true| over the
    free frames and the loss both end lower than they start."""
    from pnr.mapping import MapStep
    _, _, _, true = window
    sampler = _perturbed_sampler(pnr_mod, dev, fix, window, 400, seed=2)
    sampler.c2w[0] = window[0][0].to(dev)  # the fixed frame sits at its rendering pose
    ba = pnr_mod.BundleAdjust(sampler, 1e-3)
    cam = torch.from_numpy(fix['cam']).clone()
    cam[0] = true[0]
    ba.set_camera_tensors(cam)
    ms = MapStep(_renderer(pnr_mod), _decoder(pnr_mod, dev), ba=ba)
    ms.opt.use_device_step()
    err0 = (ba.camera_tensors()[1:].cpu() - true[1:]).abs().mean().item()
    losses = [float(ms(*sampler())) for _ in range(30)]
    err = (ba.camera_tensors()[1:].cpu() - true[1:]).abs().mean().item()
    print(f'loss {losses[0]:.4f} -> {losses[-1]:.4f} (ratio {losses[-1] / losses[0]:.3f}); '
          f'mean |cam - true| {err0:.3e} -> {err:.3e} (ratio {err / err0:.3f})')
    assert err < err0
    assert losses[-1] < losses[0]
    assert torch.equal(ba.camera_tensors()[0].cpu(), true[0])


# ---- 8. refusals -----------------------------------------------------------------------------------------

def test_ba_refusals(pnr_mod, dev, fix, window):
    from pnr.mapping import MapStep
    sampler = _perturbed_sampler(pnr_mod, dev, fix, window, 7)
    ba = pnr_mod.BundleAdjust(sampler, 1e-3)
    ddp = types.SimpleNamespace(world=2, shard_points=False)
    with pytest.raises(NotImplementedError, match='data parallel'):
        MapStep(_renderer(pnr_mod), _decoder(pnr_mod, dev), ba=ba, ddp=ddp)
    ms = MapStep(_renderer(pnr_mod), _decoder(pnr_mod, dev), ba=ba)
    batch = sampler()
    with pytest.raises(ValueError, match='last batch'):  # a batch that is not the sampler's
        ms(*[t[:-1] for t in batch[:5]])
