"""One Mapper iteration on the HIP path (src/Mapper.py:335-694).

`MapStep` is the inner loop body of Mapper.optimize_map for the imap* decoder
(src/Mapper.py:507-662): render the sampled rays with gt depth (Renderer.render_batch_ray,
:623-624), L1 depth over gt>0 + w_color * L1 colour (:641-646), 0.0005 * |sigma| of the
regulation query (:650-655), backward, Adam step with lr = imap_decoders_lr (:540, :657-662).

The decoder parameters live in ONE flat float32 buffer (and so do their grads), so a data-
parallel caller reduces a single 891 KB buffer per step and Adam is one kernel
(pnr_adam_step).  With neural points the fc_c tensors and the point features
join the same buffer (features last, with their own learning rate: a second Adam launch over the
tail of the buffer), still one all-reduce per step -- or, with DataParallel(shard_points=True), a
reduce-scatter of the feature tail, Adam on the owned feature range and an all-gather.  `ddp`
(pnr.dist.DataParallel) adds the cross-GPU gradient all-reduce and the
global far clamp; without it the step is single-GPU.  The step is deterministic: every weight-
gradient GEMM stores per-workgroup partial tiles that one reduction adds in a fixed order (no float
atomics), so a replay or a rerun reproduces it bit for bit.  It is not the reference's float32
summation order (no GPU sum is); tests/test_gpu_precision.py holds it to the correctly-rounded
gradient.  The point-feature gradient (neural points) is summed exactly in int64 fixed point
(include/pnr.h, ABI 10), so it does not depend on scheduling either: a neural-point step reruns and
replays bit for bit too.

Bundle adjustment (mapping.BA, src/Mapper.py:460-500, 567-581, 675-692): `MapStep(..., ba=BundleAdjust(
sampler, cam_lr))` adds the camera tensors of the window's keyframes as a second parameter group.  The
map pass then also emits the ray gradients (one launch more), and ONE pnr_pose_step launch forms the
(F,7) camera-tensor gradient, takes the camera Adam step and rewrites the sampler's c2w table, so the
next iteration's rays come from the stepped poses.  Deterministic like the rest of the step.
"""
from __future__ import annotations

import torch

from . import _lib


class FlatParams:
    """Re-seat every parameter of `module` (and its .grad) as a view of one flat buffer."""

    def __init__(self, params):
        self.params = list(params)
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.data = torch.empty(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            k = p.numel()
            self.data[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.data[off:off + k].view_as(p)
            p.grad = self.grad[off:off + k].view_as(p)
            off += k
        self.numel = n

    def zero_grad(self):
        self.grad.zero_()


class Adam:
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8) over a FlatParams buffer, one launch per
    learning-rate segment.  `segments` = [(first word, words, lr)], default the whole buffer.
    `use_device_step()` switches the step number to a device counter (pnr_adam_multi_dev: every
    segment and the step advance in one launch), so a step captured in a graph replays with the right
    bias corrections."""

    def __init__(self, flat: FlatParams, lr: float, betas=(0.9, 0.999), eps=1e-8, on_update=None, segments=None,
                 half=None):
        """`half` (optional): {segment index: float16 device tensor of the segment's length} -- with the
        device step counter, the Adam launch also writes float16 of the updated values there (the
        gather's f16 feature copy, pnr_adam_multi_dev_h) and `wrote_half` is set after the step."""
        self.flat = flat
        self.half = dict(half or {})
        self.wrote_half = False
        self.on_update = on_update
        self.lr = lr
        self.segments = segments if segments is not None else [(0, flat.numel, lr)]
        self.b1, self.b2 = betas
        self.eps = eps
        # moments per segment, sized to it: a sharded feature tail holds only the owned range's m / v
        self.mv = [(torch.zeros(n, device=flat.data.device), torch.zeros(n, device=flat.data.device))
                   for _, n, _ in self.segments]
        self.step_count = 0
        self.step_dev = None  # int32 device counter of completed steps (graph mode)

    def use_device_step(self):
        """step_dev = int32 {completed steps, ticket 0} on the device (pnr_adam_multi_dev): every
        segment and the step advance in ONE launch per step."""
        if self.step_dev is None:
            import ctypes
            self.step_dev = torch.tensor([self.step_count, 0], dtype=torch.int32, device=self.flat.data.device)
            k = len(self.segments)
            self._seg_args = ((ctypes.c_int64 * k)(*[a for a, _, _ in self.segments]),
                              (ctypes.c_int64 * k)(*[n for _, n, _ in self.segments]),
                              (ctypes.c_void_p * k)(*[m.data_ptr() for m, _ in self.mv]),
                              (ctypes.c_void_p * k)(*[v.data_ptr() for _, v in self.mv]),
                              (ctypes.c_float * k)(*[lr for _, _, lr in self.segments]))
            self._half_arr = None
            if self.half:
                self._half_arr = (ctypes.c_void_p * k)(*[self.half[q].data_ptr() if q in self.half else None
                                                         for q in range(k)])

    def step(self):
        self.step_count += 1
        lib = _lib.load()
        f = self.flat
        st = _lib.stream_of(f.data.device)
        self.wrote_half = False
        if self.step_dev is not None:
            off, n, m, v, lr = self._seg_args
            if self._half_arr is not None:
                _lib.check(lib.pnr_adam_multi_dev_h(_lib.ptr(f.data), _lib.ptr(f.grad), len(self.segments), off, n, m,
                                                    v, lr, self.b1, self.b2, self.eps, self._half_arr,
                                                    _lib.ptr(self.step_dev), st), 'adam_multi_dev_h')
                self.wrote_half = True
            else:
                _lib.check(lib.pnr_adam_multi_dev(_lib.ptr(f.data), _lib.ptr(f.grad), len(self.segments), off, n, m,
                                                  v, lr, self.b1, self.b2, self.eps, _lib.ptr(self.step_dev), st),
                           'adam_multi_dev')
        else:
            for (a, n, lr), (m, v) in zip(self.segments, self.mv):
                _lib.check(lib.pnr_adam_step(_lib.ptr(f.data[a:]), _lib.ptr(f.grad[a:]), _lib.ptr(m),
                                             _lib.ptr(v), n, lr, self.b1, self.b2, self.eps, self.step_count,
                                             st), 'adam_step')
        if self.on_update is not None:  # weights changed behind autograd: drop the packed image
            self.on_update()


class BundleAdjust:
    """The camera-tensor parameter group of Mapper.optimize_map under mapping.BA (src/Mapper.py:460-500):
    one (qw, qx, qy, qz, tx, ty, tz) tensor per frame of a WindowSampler's window (get_tensor_from_camera
    of its poses), Adam moments for them, and the step itself (pnr_pose_step: pose gradient from the ray
    gradients, Adam with lr = mapping.BA_cam_lr on the frames that are not fixed, and their rows of the
    pose table rewritten from the stepped tensors -- one launch).

    `self.c2w` IS `sampler.c2w` (the same storage): the sampler's next batch is drawn from the stepped
    poses.  As in the reference, whose rays come from get_camera_from_tensor(camera_tensor) from the
    first iteration on (:567-581), the rows of the frames that are not fixed are rewritten from their
    tensors here.  `fixed`: frame indices that stay put, default the oldest frame (:464-465).
    `poses()` is the (F,4,4) est_c2w of the write-back (:675-690), `camera_tensors()` the (F,7) tensors;
    `g_cam` holds the last step's camera gradient (zero rows for the fixed frames)."""

    def __init__(self, sampler, cam_lr, fixed=(0,), betas=(0.9, 0.999), eps=1e-8):
        from .common import get_tensor_from_camera
        self.sampler = sampler
        self.c2w = sampler.c2w
        dev = self.c2w.device
        F = self.c2w.shape[0]
        self.fixed = tuple(sorted({int(f) % F for f in fixed}))
        self.fixed_mask = torch.zeros(F, dtype=torch.uint8)
        for f in self.fixed:
            self.fixed_mask[f] = 1
        self.fixed_mask = self.fixed_mask.to(dev)
        self.lr = float(cam_lr)
        self.b1, self.b2 = betas
        self.eps = eps
        self.cam = torch.empty((F, 7), dtype=torch.float32, device=dev)
        self.m = torch.zeros((F, 7), dtype=torch.float32, device=dev)
        self.v = torch.zeros((F, 7), dtype=torch.float32, device=dev)
        self.g_cam = torch.zeros((F, 7), dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)  # completed camera Adam steps
        self.ws = torch.zeros(_lib.load().pnr_pose_step_workspace_bytes(F, int(sampler.n)), dtype=torch.uint8,
                              device=dev)
        self.set_camera_tensors(torch.stack([get_tensor_from_camera(self.c2w[f].cpu()) for f in range(F)]))

    def set_camera_tensors(self, cam):
        """Take (F,7) camera tensors (any quaternion norm) and rewrite the pose-table rows of the frames
        that are not fixed from them (get_camera_from_tensor)."""
        from .common import get_camera_from_tensor
        self.cam.copy_(cam.detach().to(self.cam.device, torch.float32))
        free = [f for f in range(self.cam.shape[0]) if f not in self.fixed]
        if free:
            self.c2w[free, :3, :] = get_camera_from_tensor(self.cam[free])

    def camera_tensors(self):
        return self.cam.detach().clone()

    def poses(self):
        return self.c2w.detach().clone()

    def step(self, g_rays_o, g_rays_d, idx=None, adam=True):
        """pnr_pose_step on the ray gradients of the batch drawn from `idx` (default: the sampler's last
        batch).  adam=False: `g_cam` only."""
        idx = self.sampler.idx if idx is None else idx
        F, H, W = self.sampler.depth.shape
        npf = int(self.sampler.n)
        if idx is None or idx.numel() != F * npf or g_rays_o.shape[0] != F * npf or g_rays_d.shape[0] != F * npf:
            raise ValueError('pnr.BundleAdjust: the ray gradients do not belong to the window sampler\'s last batch '
                             f'({F} frames x {npf} pixels)')
        dev = self.cam.device
        _lib.require_cuda(g_rays_o, g_rays_d, idx, self.cam, self.c2w)
        fx, fy, cx, cy = [float(x) for x in self.sampler.cam]
        _lib.check(_lib.load().pnr_pose_step(
            _lib.ptr(g_rays_o), _lib.ptr(g_rays_d), _lib.ptr(idx), F, npf, H, W, fx, fy, cx, cy, _lib.ptr(self.cam),
            _lib.ptr(self.fixed_mask), _lib.ptr(self.m), _lib.ptr(self.v), self.lr, self.b1, self.b2, self.eps,
            _lib.ptr(self.step_dev), 1 if adam else 0, _lib.ptr(self.c2w), _lib.ptr(self.g_cam), _lib.ptr(self.ws),
            self.ws.numel(), _lib.stream_of(dev)), 'pose_step')


class MapStep:
    """One Mapper iteration.  Default (`fused=True`): the render and the regulation are ONE decoder
    pass (pnr.renderer.MapPass -> pnr_map_fwd / pnr_map_bwd): the regulation and coarse samples share
    one MLP launch, the importance samples take a second, pnr_map_loss forms both loss terms and their
    gradients in one launch, and one delta-chain / weight-gradient pass covers every sample.  (The MLP
    kernels hold every CU's registers and LDS, so two chains on two streams could only take turns,
    and the small ray kernels of one chain waited behind the other's MLP launches.)
    `fused=False` keeps the two-chain form: the regulation's forward, loss term and backward on a side
    stream with its own gradient buffer (`overlap` True / 'auto' up to OVERLAP_MAX_RAYS rays) or on the
    caller's stream (`overlap=False`), joined before the gradients are summed (render + regulation, a
    fixed order).  No path goes through autograd (MapStep.loss is the autograd drop-in form).
    `ba` (a BundleAdjust over the WindowSampler that draws the batches): every path also produces the
    ray gradients and ends with the pose step on the pixel indices of the batch just drawn -- two
    launches more on the fused paths (k_map_ray_grads, k_pose_step); the two-chain form pays one ray
    kernel per chain and their sum as well.  The fused reduce + Adam + scales tail stays eligible."""

    OVERLAP_MAX_RAYS = 32768
    # the fused path as one pnr_map_step call (ABI 13) rather than pnr_map_fwd + pnr_map_loss + pnr_map_bwd
    one_call = True
    # let the gradient reduction take the Adam step and form the next pack's scales (pnr_map_step_adam)
    # when the step qualifies (`_wants_tail`); `tail_fused` tells which path the last step took
    fuse_tail = True

    def __init__(self, renderer, decoder, lr=2e-4, w_color_loss=0.05, w_reg=0.0005, ddp=None, points=None,
                 feat_lr=None, overlap='auto', fused=True, ba=None):
        if ba is not None and ddp is not None:
            raise NotImplementedError('pnr.MapStep: bundle adjustment under data parallel is not built (the camera '
                                      'gradient would need its own all-reduce)')
        self.ba = ba
        self.renderer = renderer
        self.decoder = decoder
        self.points = points
        params = list(decoder.ordered_params())
        if points is not None:
            params += list(decoder.ordered_fc_params())
        n_dec = sum(p.numel() for p in params)
        if points is not None:
            params.append(points.feats)
        self.flat = FlatParams(params)
        # A cloud with a capacity (NeuralPoints.add_frame) steps every row of `feats`, live or not: the
        # feature gradient view is zeroed every step, a row that is not live is no sample's neighbour and
        # keeps a zero gradient, and Adam with g = m = v = 0 leaves it bit-identical.  One deviation from
        # a per-row optimiser: a row that becomes live later meets Adam's running step count (its bias
        # corrections), not a fresh one.
        segs = [(0, n_dec, lr)]
        self.n_dec = n_dec
        self.shard = points is not None and ddp is not None and getattr(ddp, 'shard_points', False)
        if points is not None:
            flr = lr if feat_lr is None else feat_lr
            if self.shard:  # Adam on this rank's owned feature range only (pnr.dist reduce_scatter_)
                a, b, _ = ddp.feature_shard(points.feats.numel())
                if b > a:
                    segs.append((n_dec + a, b - a, flr))
            else:
                segs.append((n_dec, points.feats.numel(), flr))
        # float16 features (C5): the captured step's Adam launch refreshes the gather's f16 copy itself
        # (the whole-table conversion was a pass of its own); the sharded update all-gathers after Adam
        half = None
        if points is not None and points.feat_dtype == 'float16' and not self.shard and len(segs) == 2:
            half = {1: points._feats_for_gather()}
        self.opt = Adam(self.flat, lr, on_update=self._invalidate, segments=segs, half=half)
        self.c = {} if points is None else {'points_' + getattr(decoder, 'name', ''): points}
        self.w_color = w_color_loss
        self.w_reg = w_reg
        self.ddp = ddp
        if overlap not in (True, False, 'auto'):
            raise ValueError(f'overlap must be True, False or "auto", not {overlap!r}')
        self.overlap = overlap
        self.fused = bool(fused)
        self.side = None   # the side stream and the regulation chain's gradient buffer (same layout
        self.grad2 = None  # as flat.grad) with its views: made on the first overlapped step
        self._views = {'main': self._split(self.flat.grad)}
        self.tail_fused = False  # the last step ran reduce + Adam + scales as one launch
        self._tail = None        # (AdamTail descriptor, its scales / hand-off area)

    def _loss_ws(self, chain):
        """The pnr_map_loss workspace of a chain's stream (zero-filled once; each call leaves it zero)."""
        ws = self.__dict__.setdefault('_lws', {})
        if chain not in ws:
            from .renderer import map_loss_workspace
            ws[chain] = map_loss_workspace(self.flat.data.device)
        return ws[chain]

    def _overlaps(self, n_rays):
        if self.overlap != 'auto':
            return bool(self.overlap)
        return n_rays <= self.OVERLAP_MAX_RAYS

    def _split(self, buf):
        """(11 decoder, 8 fc_c or None, features or None) views of a flat-gradient-shaped buffer."""
        views, off = [], 0
        for p in self.flat.params:
            views.append(buf[off:off + p.numel()].view_as(p))
            off += p.numel()
        if self.points is None:
            return views, None, None
        return views[:11], views[11:19], views[19]

    def _wants_tail(self):
        """The fused tail's conditions on this side of the C call (single GPU, decoder only, the f16x3
        precision, Adam on the device step counter); pnr_map_step_adam checks the rest."""
        return (self.fuse_tail and self.fused and self.one_call and self.ddp is None and self.points is None
                and self.renderer.precision == 'f16x3' and self.opt.step_dev is not None
                and len(self.opt.segments) == 1 and self.opt.segments[0][:2] == (0, self.flat.numel))

    def _tail_desc(self):
        """The pnr_adam_tail of this call: built from the optimiser as it stands now (segment 0's learning
        rate, the betas, eps, the buffers), so a later change of any of them reaches the fused tail as it
        reaches Adam.step; only the scales / hand-off area is kept from call to call."""
        o, f = self.opt, self.flat
        if self._tail is None:
            self._tail = (None, torch.zeros(_lib.load().pnr_step_tail_floats(), device=f.data.device))
        area = self._tail[1]
        m, v = o.mv[0]
        t = _lib.AdamTail(f.data.data_ptr(), f.grad.data_ptr(), m.data_ptr(), v.data_ptr(), f.numel,
                          o.segments[0][2], o.b1, o.b2, o.eps, o.step_dev.data_ptr(), area.data_ptr())
        self._tail = (t, area)
        return t

    def head_pack(self):
        """(tensor pointers, image, scales) for a caller that packs in its own launch, when the last step
        left fresh scales (PackedMLP.adopt); else None."""
        if not self._wants_tail():
            return None
        from .renderer import _decoder_params, _packer
        return _packer(self.decoder).adopt(_decoder_params(self.decoder))

    def _invalidate(self):
        self.decoder._packed.invalidate()
        if self.points is not None:
            self.decoder._packed_fc.invalidate()
            if self.opt.wrote_half:  # Adam wrote the f16 feature copy with the fp32 master
                self.points.mark_feats_fresh()
            else:
                self.points.invalidate_feats()  # the f16 feature copy, if any

    def _regulation_chain(self, views, rays_o, rays_d, gt_depth, t_rand, ray_grads=None):
        from .renderer import TrainPass, map_loss
        reg = TrainPass(self.renderer, self.c, self.decoder, 'regulation')
        (sigma,) = reg.forward(rays_o, rays_d, gt_depth, t_rand=t_rand)
        loss, _, _, g_s = map_loss(None, None, None, None, 0.0, sigma=sigma, w_reg=self.w_reg, ws=self._loss_ws('side'))
        reg.backward(views[0], g_fc=views[1], g_feats=views[2], g_sigma=g_s, ray_grads=ray_grads)
        return loss

    def __call__(self, rays_o, rays_d, gt_depth, gt_color, t_rand=None, far_clamp=None):
        """One Mapper iteration.  far_clamp (optional): the batch's max(1.2 gt) as a device scalar
        (e.g. from WindowSampler), else computed by the render pass (or all-reduced, data parallel)."""
        if self.ba is None:
            return self._iterate(rays_o, rays_d, gt_depth, gt_color, t_rand, far_clamp, None)
        # bundle adjustment: the pass also writes dL/drays_o, dL/drays_d; the pose step ends the iteration
        idx = self.ba.sampler.idx
        if idx is None or idx.numel() != rays_o.shape[0]:
            raise ValueError('pnr.MapStep: with `ba` the batch must be the window sampler\'s last batch (its pixel '
                             'indices give the pose gradient)')
        rg = torch.empty((2, rays_o.shape[0], 3), dtype=torch.float32, device=rays_o.device)
        loss = self._iterate(rays_o, rays_d, gt_depth, gt_color, t_rand, far_clamp, rg)
        self.ba.step(rg[0], rg[1])
        return loss

    def _iterate(self, rays_o, rays_d, gt_depth, gt_color, t_rand, far_clamp, rg):
        from .renderer import TrainPass, map_loss
        r = self.renderer
        dev = rays_o.device
        rays_o = rays_o.float().contiguous()
        rays_d = rays_d.float().contiguous()
        gt_depth = gt_depth.reshape(-1).float().contiguous()
        gt_color = gt_color.float().contiguous()
        if t_rand is None:
            t_rand = torch.rand((rays_o.shape[0], r.N_samples), device=dev)
        t_rand = t_rand.float().contiguous()
        if self.fused:  # the map pass stores the decoder / fc_c gradients (grads_overwrite): zero the rest
            if self.points is not None:
                self._views['main'][2].zero_()
        else:
            self.flat.zero_grad()
        if self.ddp is not None:
            far_clamp = self.ddp.global_far_clamp(gt_depth, far_clamp)
        ren = TrainPass(r, self.c, self.decoder, 'render')
        # the weight images, the point index and the f16 feature copy: built on this stream before the
        # chains fork (both read them)
        prec = _lib.precision_code(r.precision)
        ren.packer.image(ren.feat.params, prec=prec)
        if self.points is not None:
            ren.feat.fc_owner.image(ren.feat.fc, prec=prec)
            self.points.index()
            self.points._feats_for_gather()
        if self.fused:  # render + regulation as ONE decoder pass (pnr_map_fwd / pnr_map_bwd)
            from .renderer import MapPass
            mp = MapPass(r, self.c, self.decoder)
            views = self._views['main']
            if self.one_call:  # pnr_map_step: forward, loss and backward in one C call, fused tail
                tail = self._tail_desc() if self._wants_tail() else None
                loss = mp.step(rays_o, rays_d, gt_depth, gt_color, t_rand, self.w_color, self.w_reg,
                               self._loss_ws('main'), views[0], g_fc=views[1], g_feats=views[2],
                               far_clamp=far_clamp, overwrite=True, tail=tail, ray_grads=rg)
                self.tail_fused = mp.tail_fused
                if mp.tail_fused:  # Adam ran inside the reduction: the image is stale, its next scales are not
                    self.opt.step_count += 1
                    self.opt.wrote_half = False
                    mp.packer.scales_fresh(mp.feat.params, self._tail[1])
                    return loss
                return self._finish(loss)
            d, _, c, sigma = mp.forward(rays_o, rays_d, gt_depth, t_rand, far_clamp=far_clamp)
            loss, g_d, g_c, g_s = map_loss(gt_depth, d, gt_color, c, self.w_color, sigma=sigma, w_reg=self.w_reg,
                                           ws=self._loss_ws('main'))
            views = self._views['main']
            mp.backward(views[0], g_fc=views[1], g_feats=views[2], g_depth=g_d, g_rgb=g_c, g_sigma=g_s,
                        overwrite=True, ray_grads=rg)
            return self._finish(loss)
        main = torch.cuda.current_stream(dev)
        overlap = self._overlaps(rays_o.shape[0])
        if overlap and self.side is None:
            self.side = torch.cuda.Stream(dev)
            self.grad2 = torch.zeros_like(self.flat.grad)
            self._views['side'] = self._split(self.grad2)
        rg2 = None if rg is None else torch.empty_like(rg)  # the regulation chain's ray gradients
        if overlap:
            self.side.wait_stream(main)
            with torch.cuda.stream(self.side):
                self.grad2.zero_()
                l_reg = self._regulation_chain(self._views['side'], rays_o, rays_d, gt_depth, t_rand, rg2)
        d, _, c = ren.forward(rays_o, rays_d, gt_depth, far_clamp=far_clamp)
        l_ren, g_d, g_c, _ = map_loss(gt_depth, d, gt_color, c, self.w_color, ws=self._loss_ws('main'))
        views = self._views['main']
        ren.backward(views[0], g_fc=views[1], g_feats=views[2], g_depth=g_d, g_rgb=g_c, ray_grads=rg)
        if overlap:
            main.wait_stream(self.side)
            self.flat.grad.add_(self.grad2)  # render + regulation gradients, a fixed order
        else:
            l_reg = self._regulation_chain(views, rays_o, rays_d, gt_depth, t_rand, rg2)
        if rg is not None:
            rg.add_(rg2)
        return self._finish(l_ren + l_reg)

    def _finish(self, loss):
        """The gradient exchange (data parallel) and the Adam step."""
        self.tail_fused = False
        if self.ddp is not None and self.shard:
            self.ddp.allreduce_(self.flat.grad[:self.n_dec])
            self.ddp.reduce_scatter_(self.flat.grad[self.n_dec:])
        elif self.ddp is not None:
            self.ddp.allreduce_(self.flat.grad)
        self.opt.step()
        if self.shard:
            self.ddp.all_gather_(self.flat.data[self.n_dec:])
            self.points.invalidate_feats()
        return loss

    def loss(self, rays_o, rays_d, gt_depth, gt_color, t_rand=None, far_clamp=None, camera_tensors=None, idx=None):
        """The Mapper loss through the autograd Renderer API (src/Mapper.py:623-655): the drop-in form
        of what __call__ computes on its fused path.
        Bundle adjustment form (src/Mapper.py:567-581): with `camera_tensors` (F,7) and the batch's pixel
        indices `idx` (F * n, the layout of pnr_window_rays) the rays are built per frame from
        get_camera_from_tensor through pnr.tracking.rays_from_uv, so the loss reaches the camera tensors
        (rays_o / rays_d are ignored and may be None); the frames `ba` holds fixed are detached.  The
        image size and intrinsics are the window sampler's (ba) or else the renderer's."""
        r, dec = self.renderer, self.decoder
        if camera_tensors is not None:
            from .common import get_camera_from_tensor
            from .tracking import rays_from_uv
            if self.ba is not None:
                (_, H, W), (fx, fy, cx, cy) = self.ba.sampler.depth.shape, self.ba.sampler.cam
            else:
                H, W, fx, fy, cx, cy = r.H, r.W, r.fx, r.fy, r.cx, r.cy
            F = camera_tensors.shape[0]
            pix = idx.reshape(F, -1).clamp(0, H * W - 1)
            ro, rd = [], []
            for f in range(F):
                ct = camera_tensors[f]
                if self.ba is not None and f in self.ba.fixed:
                    ct = ct.detach()
                o, d = rays_from_uv((pix[f] % W).float(), torch.div(pix[f], W, rounding_mode='floor').float(),
                                    get_camera_from_tensor(ct), fx, fy, cx, cy)
                ro.append(o)
                rd.append(d)
            rays_o, rays_d = torch.cat(ro, 0), torch.cat(rd, 0)
        dev = rays_o.device
        d, _, c = r.render_batch_ray(self.c, dec, rays_d, rays_o, dev, 'color', gt_depth, far_clamp=far_clamp)
        m = gt_depth > 0
        loss = torch.where(m, torch.abs(gt_depth - d), torch.zeros_like(d)).sum()
        loss = loss + self.w_color * torch.abs(gt_color - c).sum()
        sigma = r.regulation(self.c, dec, rays_d, rays_o, gt_depth, dev, 'color', t_rand=t_rand)
        return loss + self.w_reg * torch.abs(sigma).sum()


class MapGraph:
    """A MapStep captured once in a HIP graph (torch.cuda.CUDAGraph) and replayed per iteration.

    The Mapper runs `mapping.iters` (60) iterations per keyframe on a fixed-size pixel batch
    (1,000 rays under configs/pointNeRF_slam.yaml); at that size a step is ~130 launches whose host
    overhead rivals the GPU time.  Replaying the captured step removes it.  The graph owns static
    input buffers (rays, gt depth / colour and the regulation jitter t_rand): each call copies the
    batch in, replays, and returns the loss tensor (overwritten by the next call).  Capture needs a
    fixed batch shape and Adam's device step counter (`Adam.use_device_step`).  A caller that
    produces its batch in place (into `inputs`: rays_o, rays_d, gt_depth, gt_color, t_rand) skips the
    five copies, ~25 us of launches at the 1,000-ray batch.  A data-parallel
    step (ddp) is captured with its collectives when the process group is RCCL ('nccl'): the far
    clamp is all-reduced and read on the device (far_mode 2), so the step has no host sync; gloo
    collectives cannot be captured.  `warmup` ordinary steps run first on the given batch (torch
    requires work on a side stream before a capture); they are real optimisation steps.

    `carry_scales` (default True): when the step's tail is fused (MapStep.tail_fused: reduce + Adam +
    weight scales in one launch) the captured iteration repacks the f16x3 weight images from the scales
    the PREVIOUS iteration's tail left on the device -- no max|W| pass of its own.  Such a graph is valid
    only while nothing but its own replays moves the decoder weights: after load_state_dict, an eager
    step through another optimiser path or a manual opt.step(), make a new MapGraph (its warm-up steps
    bring the scales up to date) instead of replaying this one; Python's "scales fresh" mark cannot
    reach inside a captured graph.  (An eager MapStep between replays is fine: its fused tail leaves the
    same area current, and an unfused one is exactly the case above.)  carry_scales=False captures the
    self-contained form instead: every replay recomputes the scales (the full f16x3 repack, two
    launches more).
    """

    def __init__(self, mstep: MapStep, rays_o=None, rays_d=None, gt_depth=None, gt_color=None, t_rand=None,
                 warmup=2, batch_fn=None, carry_scales=True):
        """`batch_fn` (optional): a callable producing (rays_o, rays_d, gt_depth, gt_color, t_rand) on
        the device -- e.g. a Mapper iteration's window sampling (WindowSampler) -- captured INTO the
        graph together with the step, so each replay draws a fresh batch (torch's CUDA RNG is
        capture-safe); then `__call__()` takes no arguments."""
        if mstep.ddp is not None and getattr(mstep.ddp, 'active', mstep.ddp.world > 1):
            import torch.distributed as dist
            if dist.get_backend(mstep.ddp.group) != 'nccl':
                raise NotImplementedError('pnr.MapGraph: only RCCL (nccl) collectives can be captured in a graph')
        self.mstep = mstep
        self.batch_fn = batch_fn
        if batch_fn is None:
            dev = rays_o.device
            self.inputs = [t.detach().clone() for t in (rays_o, rays_d, gt_depth, gt_color, t_rand)]
            body = lambda: mstep(*self.inputs)  # noqa: E731
        else:
            dev = batch_fn()[0].device
            self.inputs = None

            def body():
                # the window sampler and the stage-2-only repack as ONE launch when the last step left
                # fresh scales (pnr_window_sample_pack); any other batch_fn or state: separate calls
                grouped = carry_scales and isinstance(batch_fn, WindowSampler) and batch_fn.device_rng
                pack = mstep.head_pack() if grouped else None
                return mstep(*(batch_fn(pack=pack) if pack is not None else batch_fn()))
        # the descriptor's n_points and the index are captured by value: a grown cloud needs a new graph
        self.n_points = None if mstep.points is None else mstep.points.n_points
        mstep.opt.use_device_step()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                body()
        torch.cuda.current_stream(dev).wait_stream(side)
        # the captured step starts with the weight repack: in full, or (after a warm-up step whose tail
        # was fused) from the scales that step -- and then every replay -- leaves
        if not (mstep.tail_fused and carry_scales):
            mstep._invalidate()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = body()

    def __call__(self, rays_o=None, rays_d=None, gt_depth=None, gt_color=None, t_rand=None):
        """Copy the batch into the static inputs (a tensor that IS the static buffer -- the caller
        wrote its batch into `self.inputs` directly -- is not copied), replay, return the loss.  With a
        captured `batch_fn`, just replay."""
        if self.n_points is not None and self.mstep.points.n_points != self.n_points:
            raise RuntimeError(f'pnr.MapGraph: the cloud grew from {self.n_points} to {self.mstep.points.n_points} '
                               'points since the capture (NeuralPoints.add_frame): make a new MapGraph')
        if self.batch_fn is None:
            for dst, src in zip(self.inputs, (rays_o, rays_d, gt_depth, gt_color, t_rand)):
                if src.data_ptr() != dst.data_ptr():
                    dst.copy_(src, non_blocking=True)
        self.graph.replay()
        # the replay moved the weights through Adam's raw pointers (no _version bump) and repacked only
        # the f16x3 images: a later eager call must not reuse a cached image of any precision
        self.mstep.decoder._packed.invalidate()
        if self.mstep.points is not None:
            self.mstep.decoder._packed_fc.invalidate()
        return self.loss


def window_batch(frames, pixs_per_image, H, W, fx, fy, cx, cy, device, generator=None):
    """The per-iteration pixel batch of Mapper.optimize_map (src/Mapper.py:560-606): for every
    frame of the optimisation window, in window order, `pixs_per_image` uniform pixels of the whole
    image (the effective path for every frame index: SURVEY.md appendix item 7), concatenated.
    frames: iterable of (c2w (3x4 or 4x4), gt depth (H,W), gt colour (H,W,3)) device tensors.
    Returns rays_o, rays_d (N,3), gt depth (N,), gt colour (N,3) float32."""
    from .renderer import get_samples
    out = [get_samples(0, H, 0, W, pixs_per_image, H, W, fx, fy, cx, cy, c2w, d, c, device, generator)
           for c2w, d, c in frames]
    return tuple(torch.cat([o[k].float() for o in out], 0) for k in range(4))



def window_rays(idx, n_per_frame, c2w, depth, color, fx, fy, cx, cy):
    """pnr_window_rays: the window batch of `window_batch` in ONE launch, for given pixel indices.
    c2w (F,4,4) / (F,3,4), depth (F,H,W), color (F,H,W,3) device tensors; idx (F * n_per_frame,) int64
    pixels of the whole image (row-major), frame f's rays at [f n, (f+1) n).  Returns rays_o, rays_d
    (N,3), gt depth (N,), gt colour (N,3) float32 -- equal to window_batch's get_samples on the same
    pixel indices (tests/test_gpu_mapping.py)."""
    lib = _lib.load()
    dev = depth.device
    F, H, W = depth.shape
    if c2w.shape[-2] == 3:
        c2w = torch.cat([c2w, torch.tensor([0., 0., 0., 1.], device=dev).expand(F, 1, 4)], 1)
    c2w = c2w.to(device=dev, dtype=torch.float32).contiguous()
    depth = depth.float().contiguous()
    color = color.float().contiguous()
    idx = idx.to(device=dev, dtype=torch.int64).contiguous()
    n = idx.numel()
    _lib.require_cuda(depth, color, idx, c2w)
    ro = torch.empty((n, 3), device=dev)
    rd = torch.empty((n, 3), device=dev)
    gd = torch.empty(n, device=dev)
    gc = torch.empty((n, 3), device=dev)
    _lib.check(lib.pnr_window_rays(_lib.ptr(idx), n, int(n_per_frame), H, W, float(fx), float(fy), float(cx),
                                   float(cy), _lib.ptr(c2w), _lib.ptr(depth), _lib.ptr(color), _lib.ptr(ro),
                                   _lib.ptr(rd), _lib.ptr(gd), _lib.ptr(gc), _lib.stream_of(dev)), 'window_rays')
    return ro, rd, gd, gc


class WindowSampler:
    """A Mapper iteration's batch over a fixed keyframe window (src/Mapper.py:397, 553-606):
    `pixs_per_image` = mapping.pixels // len(window) uniform pixels per frame, their rays, gt depth
    and colour, and the regulation jitter t_rand (Renderer.py:293).
    frames: list of (c2w, gt depth (H,W), gt colour (H,W,3)) device tensors.

    device_rng=True (default): ONE pnr_window_sample launch draws the pixels and the jitter on the
    device (counter-based hash of `seed` and a device batch counter) and also returns the batch far
    clamp max(1.2 gt) as a device scalar -- a captured iteration (MapGraph(batch_fn=sampler)) then
    spends one launch on its batch.  device_rng=False: torch.randint / torch.rand (torch's Philox
    stream, `generator`) + one pnr_window_rays launch; far clamp None (computed by the render pass).
    __call__ returns (rays_o, rays_d, gt_depth, gt_color, t_rand, far_clamp)."""

    def __init__(self, frames, pixs_per_image, fx, fy, cx, cy, n_samples=32, generator=None, device_rng=True,
                 seed=0):
        self.c2w = torch.stack([f[0][:3] if f[0].shape[0] == 3 else f[0] for f in frames]).float()
        if self.c2w.shape[1] == 3:
            self.c2w = torch.cat([self.c2w, torch.tensor([0., 0., 0., 1.], device=self.c2w.device)
                                  .expand(len(frames), 1, 4)], 1)
        self.c2w = self.c2w.contiguous()
        self.depth = torch.stack([f[1].float() for f in frames]).contiguous()
        self.color = torch.stack([f[2].float() for f in frames]).contiguous()
        self.n = int(pixs_per_image)
        self.cam = (fx, fy, cx, cy)
        self.n_samples = n_samples
        self.generator = generator
        self.device_rng = device_rng
        self.seed = int(seed) & ((1 << 64) - 1)
        self.idx = None  # the last batch's pixel indices
        if device_rng:
            lib = _lib.load()
            dev = self.depth.device
            self.state = torch.zeros(lib.pnr_window_sample_state_bytes(), dtype=torch.uint8, device=dev)

    def __call__(self, pack=None):
        """`pack` (MapStep.head_pack()): also run the stage-2-only weight repack in the same launch."""
        F, H, W = self.depth.shape
        dev = self.depth.device
        N = F * self.n
        if not self.device_rng:
            idx = self.idx = torch.randint(H * W, (N,), device=dev, generator=self.generator)
            ro, rd, gd, gc = window_rays(idx, self.n, self.c2w, self.depth, self.color, *self.cam)
            t_rand = torch.rand((N, self.n_samples), device=dev, generator=self.generator)
            return ro, rd, gd, gc, t_rand, None
        lib = _lib.load()
        _lib.require_cuda(self.depth, self.color, self.c2w)
        ro = torch.empty((N, 3), device=dev)
        rd = torch.empty((N, 3), device=dev)
        gd = torch.empty(N, device=dev)
        gc = torch.empty((N, 3), device=dev)
        t_rand = torch.empty((N, self.n_samples), device=dev)
        self.idx = torch.empty(N, dtype=torch.int64, device=dev)
        far = torch.empty(1, device=dev)
        if pack is not None:
            arr, img, scales = pack
            _lib.check(lib.pnr_window_sample_pack(self.seed, _lib.ptr(self.state), N, self.n, H, W,
                                                  *[float(v) for v in self.cam], _lib.ptr(self.c2w),
                                                  _lib.ptr(self.depth), _lib.ptr(self.color), self.n_samples,
                                                  _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(gd), _lib.ptr(gc),
                                                  _lib.ptr(t_rand), _lib.ptr(self.idx), _lib.ptr(far), arr,
                                                  _lib.ptr(img), _lib.ptr(scales), _lib.stream_of(dev)),
                       'window_sample_pack')
            return ro, rd, gd, gc, t_rand, far
        _lib.check(lib.pnr_window_sample(self.seed, _lib.ptr(self.state), N, self.n, H, W,
                                         *[float(v) for v in self.cam], _lib.ptr(self.c2w), _lib.ptr(self.depth),
                                         _lib.ptr(self.color), self.n_samples, _lib.ptr(ro), _lib.ptr(rd),
                                         _lib.ptr(gd), _lib.ptr(gc), _lib.ptr(t_rand), _lib.ptr(self.idx),
                                         _lib.ptr(far), _lib.stream_of(dev)), 'window_sample')
        return ro, rd, gd, gc, t_rand, far
