"""Bundle-adjustment gradients of the Mapper loss (tests/golden/ba_grads*.npz) -- test infrastructure.

A window of three 34x60 frames (room0 poses 0..2 of scene.npz rendered by the oracle with the trained
decoder; intrinsics scaled as tests/test_gpu_parity.py::_track_scene scales them, cx = 30 so that
pixel column 30 has a camera-frame direction whose x component is exactly zero), 23 fixed pixels per
frame, and three camera tensors perturbed off the scene poses by a few 1e-3 -- so the quaternions
are NOT unit and quad2rotation's 2 / sum q^2 term carries gradient.  The batch holds zero-depth
pixels, rays that leave the scene bound before the batch's far clamp, and the zero-component ray.

The Mapper loss with BA (src/Mapper.py:567-581, 623-655): rays from camera_from_tensor of each frame's
tensor, mapping_loss over render_batch_ray + regulation.  Its gradient w.r.t. the (3,7) camera tensors
and the 11 decoder tensors, evaluated by the oracle (oracle/ref_render.py) in float32 (`grad_f32/`)
and correctly rounded (`grad_cr/`, eval_points_cr: every GEMM summed in float64 and rounded per
layer), with `golden_vs_cr/<name>` = max|f32 - cr| / max|cr| as in grads_cr.npz.

The loss is only piecewise smooth (ReLU units, the L1 terms, the bound test, the sort of the sample
depths), and a 23-ray frame is small enough for one kink crossed by one sample to move a camera-gradient
element by several 1e-3 of its size -- more than the elementwise bound the GPU tests hold an
implementation to (rtol 1e-3).  A gradient that jumps when an input moves by one float32 ulp is no
yardstick: the device builds its rays from its own float32 pose table, which may differ from the
oracle's in the last bit.  So the pixel seed is the first one (from 11 up) at which the float32 camera
gradient moves by less than a quarter of that bound, elementwise, under eight +-1-ulp-sized (6e-8)
perturbations of the camera tensors (`stable`).  Measured over seeds 11..27 the worst such move ranges
from 0.2 to 141 bounds, and only seed 27 stays below a quarter.  (Seed 11 itself sits on a kink: ray
45's render gradient takes either of two values 0.0345 apart, depending on the last bit of its ray.)

Three files, each below the 1 MiB a committed file may have (one form of the decoder gradient is
892 KB of float32 on its own): ba_grads.npz holds the inputs, the losses, every ratio and the camera
gradient in both forms; ba_grads_dec_f32.npz / ba_grads_dec_cr.npz the 11 decoder tensors' gradients.

    python tests/golden/make_ba_grads.py     (CPU, ~1 min; no reference import)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
from conftest import load_golden, golden_params  # noqa: E402
from oracle import ref_render as ref  # noqa: E402

H, W, FX, FY, CX, CY = 34, 60, 30., 30., 30., 16.5
N_PER_FRAME = 23
PERTURB = [[0.003, -0.002, 0.001, 0.002, 0.004, -0.003, 0.002],
           [-0.002, 0.003, 0.002, -0.001, -0.003, 0.002, 0.004],
           [0.001, 0.002, -0.003, 0.003, 0.002, 0.004, -0.002]]


def window(bound):
    """(camera tensors (3,7), true tensors, depth (3,H,W), colour (3,H,W,3)): the frames rendered at the
    TRUE poses, every 7th row / 5th column depth zeroed; the tensors perturbed off them."""
    params = golden_params('trained')
    poses = torch.from_numpy(load_golden('scene.npz')['poses'][:3]).float()
    depth, color = [], []
    for c2w in poses:
        gd, _, gc = ref.render_img(params, c2w, bound, H, W, FX, FY, CX, CY)
        gd = gd.float().clone()
        gd[::7, ::5] = 0.
        depth.append(gd)
        color.append(gc.float())
    true = torch.stack([ref.tensor_from_camera(c2w) for c2w in poses]).float()
    cam = true + torch.tensor(PERTURB)
    return cam, true, torch.stack(depth), torch.stack(color)


def pixels(seed):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, H * W, size=(3, N_PER_FRAME)).astype(np.int64)
    idx[0, 0] = 0 * W + 0       # zero depth (row 0, column 0)
    idx[0, 1] = 7 * W + 5       # zero depth
    idx[2, 3] = 14 * W + 10     # zero depth
    idx[1, 0] = 12 * W + 30     # column 30 = cx: the camera-frame direction's x component is 0
    return torch.from_numpy(idx.reshape(-1))


def rays(cam, idx):
    F = cam.shape[0]
    pix = idx.reshape(F, -1)
    ro, rd = [], []
    for f in range(F):
        o, d = ref.rays_from_uv((pix[f] % W).float(), (pix[f] // W).float(), ref.camera_from_tensor(cam[f]),
                                FX, FY, CX, CY)
        ro.append(o.reshape(-1, 3))
        rd.append(d.reshape(-1, 3))
    return torch.cat(ro, 0), torch.cat(rd, 0)


def ba_loss(p, cam, idx, gt, gc, t_rand, bound, cr):
    ev = (lambda q: ref.eval_points_cr(p, q, bound)) if cr else None
    ro, rd = rays(cam, idx)
    d, v, c = ref.render_batch_ray(p, rd, ro, bound, gt_depth=gt, eval_fn=ev)
    sig = ref.regulation(p, rd, ro, gt, bound, t_rand=t_rand, eval_fn=ev)
    return ref.mapping_loss(d, c, gt, gc, sig)


def cam_grad(cam, idx, gt, gc, t_rand, bound):
    ct = cam.clone().requires_grad_(True)
    ba_loss(golden_params('trained'), ct, idx, gt, gc, t_rand, bound, False).backward()
    return ct.grad.numpy().copy()


def stable(cam, idx, gt, gc, t_rand, bound):
    """The float32 camera gradient is locally continuous here: eight perturbations of the tensors by
    +-6e-8 (one float32 ulp of their entries) move no element by more than a quarter of the elementwise
    bound of the GPU tests, 0.25 (1e-3 |g| + 1e-6 max|g|).  Returns (ok, worst move / bound)."""
    g = cam_grad(cam, idx, gt, gc, t_rand, bound)
    tol = 1e-3 * np.abs(g) + 1e-6 * np.abs(g).max()
    rng = np.random.RandomState(0)
    worst = 0.0
    for _ in range(8):
        sign = torch.from_numpy(rng.choice([-1.0, 1.0], size=tuple(cam.shape))).float()
        worst = max(worst, (np.abs(cam_grad(cam + 6e-8 * sign, idx, gt, gc, t_rand, bound) - g) / tol).max())
        if worst > 0.25:
            return False, worst
    return True, worst


def main():
    torch.set_num_threads(8)
    bound = torch.from_numpy(load_golden('scene.npz')['bound'])
    cam, true, depth, color = window(bound)
    f = torch.arange(3).repeat_interleave(N_PER_FRAME)
    t_rand = torch.rand((3 * N_PER_FRAME, 32), generator=torch.Generator().manual_seed(12))
    for seed in range(11, 40):
        idx = pixels(seed)
        gt = depth.reshape(3, -1)[f, idx].contiguous()
        gc = color.reshape(3, -1, 3)[f, idx].contiguous()
        ok, worst = stable(cam, idx, gt, gc, t_rand, bound)
        print(f'pixel seed {seed}: worst 1-ulp move / bound = {worst:.3f}', 'taken' if ok else 'on a kink')
        if ok:
            break
    else:
        raise SystemExit('no stable pixel seed')
    # what the batch must contain
    assert int((gt == 0).sum()) >= 3
    ro, rd = rays(cam, idx)
    _, far = ref.near_far(ro, rd, bound, 32, gt)
    clamp = float((gt * 1.2).max())
    n_exit = int((far.reshape(-1) < clamp).sum())
    assert n_exit >= 1, 'no ray leaves the scene bound before the far clamp'
    assert float((idx.reshape(3, -1)[1, 0] % W).float() - CX) == 0.0
    print(f'{int((gt == 0).sum())} zero-depth pixels, {n_exit} rays leave the bound before far = {clamp:.3f}')

    out = {'cam': cam.numpy(), 'cam_true': true.numpy(), 'idx': idx.numpy(), 'gt_depth': gt.numpy(),
           'gt_color': gc.numpy(), 't_rand': t_rand.numpy(), 'intrinsics': np.array([H, W, FX, FY, CX, CY]),
           'n_per_frame': np.array(N_PER_FRAME), 'pixel_seed': np.array(seed)}
    grads, dec = {}, {'f32': {}, 'cr': {}}
    for tag, cr in (('f32', False), ('cr', True)):
        p = {k: v.clone().requires_grad_(True) for k, v in golden_params('trained').items()}
        ct = cam.clone().requires_grad_(True)
        loss = ba_loss(p, ct, idx, gt, gc, t_rand, bound, cr)
        loss.backward()
        out[f'loss_{tag}'] = np.array(loss.item())
        grads[tag] = {'cam': ct.grad.numpy().copy(), **{k: t.grad.numpy().copy() for k, t in p.items()}}
        for k, g in grads[tag].items():
            (out if k == 'cam' else dec[tag])[f'grad_{tag}/{k}'] = g
    for k in grads['cr']:
        a, b = grads['f32'][k], grads['cr'][k]
        out[f'golden_vs_cr/{k}'] = np.array(np.abs(a - b).max() / np.abs(b).max())
        print(f'{k:24s} |f32 - cr| / max = {out[f"golden_vs_cr/{k}"]:.2e}')
    print('loss f32 / cr:', out['loss_f32'], out['loss_cr'])
    np.savez_compressed(os.path.join(HERE, 'ba_grads.npz'), **out)
    for tag in dec:
        np.savez_compressed(os.path.join(HERE, f'ba_grads_dec_{tag}.npz'), **dec[tag])


if __name__ == '__main__':
    main()
