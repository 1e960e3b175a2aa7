"""The Mapper step's fused tail and grouped head.

pnr_map_step_adam: the weight-gradient reduction also takes the Adam step and forms the next pack's
weight scales (k_reduce_adam_multi) -- one launch where k_part_reduce_multi, k_adam_multi and the
pack's scale stage were three; pnr_mlp_pack_scaled then runs the images' launch alone, and
pnr_window_sample_pack runs it inside the window sampler's launch.  Everything is bit for bit what the
separate launches give: loss, parameters, gradients, Adam moments, step counter, scales and images.
Trained fixture weights, S = 32, I = 12, f16x3, the device step counter.
"""
import types

import pytest
import torch

from conftest import golden_params, load_golden

gpu = pytest.mark.gpu

W16 = 225280  # floats of the 16-point-wave forward image, after the raw table (mlp16w.h)
RAW_INV, RAW_SCL = 1344, 1352  # raw-table words of the inverse scales / scales (mlp16.h)


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


def _renderer(pnr, precision='f16x3'):
    bound = torch.from_numpy(load_golden('scene.npz')['bound'])
    slam = types.SimpleNamespace(bound=bound, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5)
    r = pnr.Renderer(pnr.ROOM0_CFG, None, slam)
    r.precision = precision
    return r


def _decoder(pnr, dev, params=None):
    dec = pnr.get_model(pnr.ROOM0_CFG, nice=False)
    dec.load_state_dict({k: v.clone() for k, v in (params or golden_params('trained')).items()})
    return dec.to(dev)


def _batches(dev, n, k=5, seed=7):
    r = load_golden('render.npz')
    ro = torch.from_numpy(r['p2_gt/rays_o'])[:n].to(dev)
    rd = torch.from_numpy(r['p2_gt/rays_d'])[:n].to(dev)
    gt = torch.from_numpy(r['p2_gt/gt_depth'])[:n].to(dev)
    gen = torch.Generator().manual_seed(seed)
    return [(ro, rd, gt, torch.rand((n, 3), generator=gen).to(dev), torch.rand((n, 32), generator=gen).to(dev))
            for _ in range(k)]


def _mstep(pnr, dev, fuse_tail, precision='f16x3', params=None, **kw):
    from pnr.mapping import MapStep
    ms = MapStep(_renderer(pnr, precision), _decoder(pnr, dev, params), **kw)
    ms.fuse_tail = fuse_tail
    ms.opt.use_device_step()
    return ms


def _state(ms, loss):
    torch.cuda.synchronize()
    m, v = ms.opt.mv[0]
    return {'loss': loss.detach().clone(), 'params': ms.flat.data.clone(), 'grads': ms.flat.grad.clone(),
            'm': m.clone(), 'v': v.clone(), 'step2': ms.opt.step_dev.clone()}


def _assert_same(a, b, what):
    for k in a:
        if not torch.equal(a[k], b[k]):
            d = (a[k] != b[k]).reshape(-1).nonzero().flatten()
            i = int(d[0]) if d.numel() else -1
            raise AssertionError(f'{what}: {k} differs in {d.numel()} of {a[k].numel()} elements, first at {i}: '
                                 f'{a[k].reshape(-1)[i].item()!r} against {b[k].reshape(-1)[i].item()!r}')


def _raw0(lib):
    return lib.pnr_mlp_packed_floats() - W16 - 3072  # kOffRaw


def _full_pack(dec):
    """A fresh full pack (scale stage + images) of the decoder's current weights, as int32 words."""
    from pnr.packing import PackedMLP
    return PackedMLP().image([p.detach().clone() for p in dec.ordered_params()]).view(torch.int32)


def _assert_f16x3_regions(lib, img, ref):
    """Everything the f16x3 kernels read: the f16x3 forward and delta-chain images, the raw table (biases,
    Fourier B, inverse scales, scales, Wo) and the 16-point-wave image (tests/test_gpu_determinism.py)."""
    raw0 = _raw0(lib)
    lo = raw0 - (917504 + 901120) // 4
    for a, b in ((lo, raw0 + RAW_INV + 5), (raw0 + RAW_SCL, raw0 + RAW_SCL + 5), (raw0 + 2048, raw0 + 3072 + W16)):
        assert torch.equal(img[a:b], ref[a:b]), (a, b)


def _ref_scales(lib, ref):
    """[5 scl | 5 inv] as the pack's scale stage (pnr_mlp_pack2) wrote them into a full pack's raw table."""
    raw0 = _raw0(lib)
    return torch.cat([ref[raw0 + RAW_SCL:raw0 + RAW_SCL + 5], ref[raw0 + RAW_INV:raw0 + RAW_INV + 5]])


@gpu
@pytest.mark.parametrize('n', [8, 37])
def test_fused_step_equals_unfused(pnr_mod, dev, n):
    """Three consecutive steps each way from identical state, at ray counts ragged against the 32- and
    128-point tiles (few partial tiles: both chains of the reduction and its odd remainder): loss, flat
    parameters, gradients, m, v and the step counter bitwise equal after every step; the ten scale floats
    equal the pack's scale stage on the same weights; the stage-2-only pack equals a full pack."""
    from pnr import _lib
    lib = _lib.load()
    f16 = _lib.PRECISIONS['f16x3']
    batches = _batches(dev, n)
    fused, plain = _mstep(pnr_mod, dev, True), _mstep(pnr_mod, dev, False)
    for k, b in enumerate(batches[:3]):
        sf = _state(fused, fused(*b))
        sp = _state(plain, plain(*b))
        assert fused.tail_fused and not plain.tail_fused
        _assert_same(sf, sp, f'step {k}')
        assert int(sf['step2'][0]) == k + 1 and int(sf['step2'][1]) == 0
        ref = _full_pack(fused.decoder)
        scales = fused._tail[1][:10].clone().view(torch.int32)
        assert torch.equal(scales, _ref_scales(lib, ref)), (k, scales, _ref_scales(lib, ref))
        pk = fused.decoder._packed
        assert pk._scales is not None  # stale, scales fresh: the next f16x3-only pack is stage 2 alone
        img = pk.image(list(fused.decoder.ordered_params()), prec=f16).clone().view(torch.int32)
        torch.cuda.synchronize()
        assert pk._scales is None
        _assert_f16x3_regions(lib, img, ref)


@gpu
def test_adam_helper_matches_adam_multi(pnr_mod, dev):
    """k_adam_multi on a flat buffer against the fused kernel's update for the same gradient, bitwise,
    on crafted weights: Wo = 0 and W1 = 0 make every hidden weight gradient zero, so W1 stays all zero
    (its scale takes the e = 20 branch) and W3, whose largest |w| sits in its last element, is left
    where it was; dWo / dbo are non-zero.  Two steps (the second with non-zero moments)."""
    from pnr import _lib
    lib = _lib.load()
    from pnr.decoder import PARAM_ORDER
    crafted = {k: v.clone() for k, v in golden_params('trained').items()}
    crafted[PARAM_ORDER[9]].zero_()                # Wo
    crafted[PARAM_ORDER[3]].zero_()                # W1
    crafted[PARAM_ORDER[7]].view(-1)[-1] = 100.0   # W3: the maximum in the last element
    ms = _mstep(pnr_mod, dev, True, params=crafted)
    b = _batches(dev, 37)[0]
    m, v = ms.opt.mv[0]
    for k in range(2):
        p0, m0, v0, s0 = ms.flat.data.clone(), m.clone(), v.clone(), ms.opt.step_dev.clone()
        ms(*b)
        torch.cuda.synchronize()
        assert ms.tail_fused
        g = ms.flat.grad.clone()
        nz = int((g != 0).sum())
        assert 0 < nz <= 4 * 256 + 4 if k == 0 else nz > 0  # first step: dWo and dbo alone (Wo = 0 stops the chain)
        import ctypes
        n = ms.flat.numel
        _lib.check(lib.pnr_adam_multi_dev(_lib.ptr(p0), _lib.ptr(g), 1, (ctypes.c_int64 * 1)(0),
                                          (ctypes.c_int64 * 1)(n), (ctypes.c_void_p * 1)(m0.data_ptr()),
                                          (ctypes.c_void_p * 1)(v0.data_ptr()), (ctypes.c_float * 1)(ms.opt.lr),
                                          ms.opt.b1, ms.opt.b2, ms.opt.eps, _lib.ptr(s0), _lib.stream_of(dev)),
                   'adam_multi_dev')
        torch.cuda.synchronize()
        assert torch.equal(p0, ms.flat.data), k
        assert torch.equal(m0, m) and torch.equal(v0, v), k
        assert torch.equal(s0, ms.opt.step_dev), k
        ref = _full_pack(ms.decoder)
        got = ms._tail[1][:10].clone()
        assert torch.equal(got.view(torch.int32), _ref_scales(lib, ref)), (k, got)
        if k == 0:  # W1 still all zero: e = 20 (the second step moves it through the now non-zero Wo)
            assert float(got[1]) == 2.0 ** 20 and float(got[6]) == 2.0 ** -20
        assert float(got[3]) == 2.0 ** 7  # W3: max 100 -> floor(log2(16384 / 100)) = 7
        if k == 0:
            assert bool((ms.decoder.ordered_params()[3] == 0).all())


@gpu
def test_tail_requires_exact_cover(pnr_mod, dev):
    """pnr_map_step_adam steps only the elements its reduction owns, so it refuses (before any launch) a
    flat buffer that the eleven gradient tensors do not tile exactly."""
    ms = _mstep(pnr_mod, dev, True)
    good = ms._tail_desc

    def longer():
        t = good()
        t.n += 4
        return t
    ms._tail_desc = longer
    with pytest.raises(RuntimeError, match='bad argument'):
        ms(*_batches(dev, 8)[0])
    torch.cuda.synchronize()
    assert int(ms.opt.step_dev[0]) == 0


def _tiny_frames(dev, hw=(6, 8), frames=5, seed=3):
    gen = torch.Generator().manual_seed(seed)
    c2w = torch.from_numpy(load_golden('scene.npz')['poses'][0]).float()
    out = []
    for f in range(frames):
        p = c2w.clone()
        p[:3, 3] += 0.01 * f
        out.append((p.to(dev), (1.0 + 2.0 * torch.rand(hw, generator=gen)).to(dev),
                    torch.rand((*hw, 3), generator=gen).to(dev)))
    return out


def _sampler(dev, per, seed=5):
    from pnr.mapping import WindowSampler
    return WindowSampler(_tiny_frames(dev), per, 6.0, 6.0, 3.5, 2.5, n_samples=32, seed=seed)


@gpu
@pytest.mark.parametrize('source,carry', [('static', True), ('sampler', True), ('sampler', False)])
def test_fused_eager_equals_graph(pnr_mod, dev, source, carry):
    """Eager fused steps against a captured graph's replays over 3 steps (after 2 warm-up steps), bitwise;
    with a WindowSampler as batch_fn the graph's head is the grouped sampler + pack launch
    (carry_scales=False: the self-contained graph, whose every replay recomputes the scales)."""
    from pnr.mapping import MapGraph
    batches = _batches(dev, 37)
    runs = []
    for graph in (False, True):
        ms = _mstep(pnr_mod, dev, True)
        sampler = _sampler(dev, 8) if source == 'sampler' else None
        states = []
        if graph:
            mg = (MapGraph(ms, batch_fn=sampler, warmup=2, carry_scales=carry) if sampler
                  else MapGraph(ms, *batches[0], warmup=2))
            for b in batches[1:4]:
                states.append(_state(ms, mg() if sampler else mg(*b)))
        else:
            if sampler:
                sampler()  # MapGraph draws one batch to find the device
            for _ in range(2):
                ms(*(sampler() if sampler else batches[0]))
            for b in batches[1:4]:
                states.append(_state(ms, ms(*(sampler() if sampler else b))))
        assert ms.tail_fused
        runs.append(states)
    for k, (a, b) in enumerate(zip(*runs)):
        _assert_same(a, b, f'replay {k}')
    assert int(runs[1][-1]['step2'][0]) == 5


@gpu
@pytest.mark.parametrize('case', ['fp32', 'points'])
def test_fallback_paths(pnr_mod, dev, case):
    """fp32 precision and neural points take today's launches (tail_fused False) and give what a step
    with the fused tail switched off gives."""
    from oracle import ref_points as RP
    n = 37
    batches = _batches(dev, n)
    out = []
    for fuse in (True, False):
        if case == 'fp32':
            ms = _mstep(pnr_mod, dev, fuse, precision='fp32')
        else:
            from pnr.mapping import MapStep
            ro, rd, gt = batches[0][:3]
            gen = torch.Generator().manual_seed(4)
            surf = (ro + rd * gt[:, None]).cpu()
            xyz = (surf.repeat(4, 1) + 0.01 * torch.randn((4 * n, 3), generator=gen)).float()
            feats = torch.randn((xyz.shape[0], 32), generator=gen) * 0.5
            dec = pnr_mod.MLP(name='color', dim=3, c_dim=32, color=True, skips=[], n_blocks=4, hidden_size=256)
            dec.load_state_dict({k: v.clone() for k, v in RP.init_fc_c(golden_params('trained'), seed=1).items()})
            pts = pnr_mod.NeuralPoints(xyz.to(dev), feats.to(dev), mode='idw', radius=0.04, k=8).to(dev)
            ms = MapStep(_renderer(pnr_mod), dec.to(dev), points=pts, feat_lr=1e-2)
            ms.fuse_tail = fuse
            ms.opt.use_device_step()
        states = []
        for b in batches[:2]:
            states.append(_state(ms, ms(*b)))
            assert not ms.tail_fused
            assert ms.decoder._packed._scales is None
        out.append(states)
    for k, (a, b) in enumerate(zip(*out)):
        _assert_same(a, b, f'{case} step {k}')


def test_tail_selection_logic():
    """The Python side of the selection, no GPU needed: a data-parallel step (ddp set), neural points, the
    fp32 precision, the host step counter and the two-chain / three-call forms all keep the old path."""
    import pnr
    from pnr.mapping import MapStep

    def make(precision='f16x3', **kw):
        dec = pnr.get_model(pnr.ROOM0_CFG, nice=False)
        return MapStep(_renderer(pnr, precision), dec, **kw)

    ms = make()
    assert not ms._wants_tail()  # Adam on the host step counter
    ms.opt.step_dev = torch.zeros(2, dtype=torch.int32)
    assert ms._wants_tail()
    ms.fuse_tail = False
    assert not ms._wants_tail()
    ms.fuse_tail = True
    ms.one_call = False
    assert not ms._wants_tail()
    for kw in ({'ddp': types.SimpleNamespace(world=1, active=False, shard_points=False)}, {'fused': False},
               {'precision': 'fp32'}, {'precision': 'bf16x3'}):
        ms = make(**kw)
        ms.opt.step_dev = torch.zeros(2, dtype=torch.int32)
        assert not ms._wants_tail(), kw
    ms = make()
    ms.opt.step_dev = torch.zeros(2, dtype=torch.int32)
    ms.points = object()
    assert not ms._wants_tail()


def test_packer_mark_is_dropped():
    """PackedMLP's "stale, scales fresh" mark: set by scales_fresh, dropped by invalidate() and by a
    changed tensor (load_state_dict bumps the version), never taken without an image (no GPU needed)."""
    from pnr.packing import PackedFC, PackedMLP
    params = [torch.zeros(4) for _ in range(11)]
    scales = torch.zeros(10)
    pk = PackedMLP()
    pk.scales_fresh(params, scales)
    assert pk._scales is not None and pk._key is None
    assert pk.adopt(params) is None  # no image yet: pack in full
    pk._img = torch.zeros(1)
    assert pk._fresh(params, pk._key_of(params)) is scales
    params[3].add_(1.0)  # in-place change: another version
    assert pk._fresh(params, pk._key_of(params)) is None and pk.adopt(params) is None
    pk.scales_fresh(params, scales)
    got = pk.adopt(params)
    assert got is not None and got[1] is pk._img and got[2] is scales
    assert pk._scales is None and pk._key == pk._key_of(params) and not pk._cover_all
    pk.scales_fresh(params, scales)
    pk.invalidate()
    assert pk._scales is None
    fc = PackedFC()
    fc.scales_fresh(params, scales)  # the fc_c images have no scaled pack
    assert fc._scales is None


@gpu
@pytest.mark.parametrize('per', [3, 60])
def test_grouped_head_equals_separate_calls(pnr_mod, dev, per):
    """pnr_window_sample_pack against pnr_window_sample + pnr_mlp_pack_scaled on a 6 x 8 camera with 5
    frames, two consecutive draws: rays, gt depth and colour, t_rand, pixel indices, the far clamp and
    the sampler state bitwise equal (300 rays: two ray blocks, so the far-clamp ticket crosses blocks and
    must count the sampler's blocks alone), and the packed image equal to the separate pack's."""
    from pnr import _lib
    lib = _lib.load()
    dec = _decoder(pnr_mod, dev)
    params = [p.detach() for p in dec.ordered_params()]
    base = _full_pack(dec).view(torch.float32)
    scales = _ref_scales(lib, base.view(torch.int32)).view(torch.float32).contiguous()
    arr = _lib.PtrArray(*[t.data_ptr() for t in params])
    a, b = _sampler(dev, per), _sampler(dev, per)
    for draw in range(2):
        # (images start as garbage in the f16x3 regions: the pack has to write all of them)
        img_a, img_b = base.clone(), base.clone()
        raw0 = _raw0(lib)
        for img in (img_a, img_b):
            img[raw0 - (917504 + 901120) // 4:raw0].fill_(1.0)
            img[raw0 + 3072:].fill_(1.0)
            img[raw0 + RAW_INV:raw0 + RAW_SCL + 5].fill_(3.0)
        out_a = a()
        _lib.check(lib.pnr_mlp_pack_scaled(arr, _lib.ptr(img_a), _lib.ptr(scales), _lib.stream_of(dev)), 'pack')
        out_b = b(pack=(arr, img_b, scales))
        torch.cuda.synchronize()
        for x, y, what in zip(out_a, out_b, ('rays_o', 'rays_d', 'gt_depth', 'gt_color', 't_rand', 'far')):
            assert torch.equal(x, y), (draw, what)
        assert torch.equal(a.idx, b.idx) and torch.equal(a.state, b.state), draw
        assert int(a.state[:8].view(torch.int64)[0]) == draw + 1  # the batch counter advanced once
        assert torch.equal(img_a.view(torch.int32), img_b.view(torch.int32)), draw
        _assert_f16x3_regions(lib, img_b.view(torch.int32), base.view(torch.int32))
