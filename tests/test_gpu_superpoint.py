"""pnr.superpoint (csrc/conv.hip, csrc/keypoints.hip) against torch float64 on the CPU and a numpy restatement of
the keypoint rules.

Weights and biases are uniform in +-1/sqrt(9 Cin).  Convolution bound, elementwise: an fp32 chain of K + 1 terms
has |fl - exact| <= gamma_{K+1} sum |terms|; here 2 (K + 2) 2^-24 (|b| + conv2d(|x|, |w|)), K = kh kw Cin, the
factor 2 for the MFMA's internal order.  ReLU and max are 1-Lipschitz, so the bound passes through them (its
maximum over the pool window).  The kernel's tile is 2 rows x 32 columns x 64 channels: 17 x 33 is one pixel past
16 rows and 32 columns, 5 x 9 one past 4 rows, 40 x 72 several tiles each way, Cout = 65 ragged in channels."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NONE, RELU, POOL, SOFTMAX, L2NORM = range(5)
U = 2.0 ** -24
SPEC = dict(conv1a=(1, 64, 3), conv1b=(64, 64, 3), conv2a=(64, 64, 3), conv2b=(64, 64, 3), conv3a=(64, 128, 3),
            conv3b=(128, 128, 3), conv4a=(128, 128, 3), conv4b=(128, 128, 3), convPa=(128, 256, 3),
            convPb=(256, 65, 1), convDa=(128, 256, 3), convDb=(256, 256, 1))
LAYER_CASES = [(1, 64, 3, RELU, 8, 8), (1, 64, 3, RELU, 24, 40), (64, 64, 3, POOL, 8, 8), (64, 64, 3, POOL, 24, 40),
               (64, 64, 3, POOL, 40, 72), (64, 128, 3, RELU, 5, 9), (64, 128, 3, RELU, 17, 33),
               (128, 128, 3, POOL, 10, 18), (128, 256, 3, RELU, 2, 3), (128, 256, 3, RELU, 15, 17),
               (256, 65, 1, NONE, 2, 3), (256, 65, 1, NONE, 15, 17), (256, 256, 1, NONE, 15, 17)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def draw(gen, cin, cout, k):
    s = 1.0 / np.sqrt(9 * cin)
    return ((torch.rand((cout, cin, k, k), generator=gen) * 2 - 1) * s, (torch.rand(cout, generator=gen) * 2 - 1) * s)


@functools.lru_cache(maxsize=None)
def state_dict(bias=True):
    gen, sd = torch.Generator().manual_seed(0), {}
    for name, (cin, cout, k) in SPEC.items():
        sd[name + '.weight'], b = draw(gen, cin, cout, k)
        sd[name + '.bias'] = b if bias else torch.zeros_like(b)
    return sd


def conv64(x, e_in, w, b, epi):
    """float64 layer on x (1,C,H,W) and the propagated bound: E = conv(E_in, |w|) + the local chain bound"""
    w, b, pad = w.double(), b.double(), w.shape[2] // 2
    y = F.conv2d(x, w, b, padding=pad)
    local = 2 * (w[0].numel() + 2) * U * (b.abs()[None, :, None, None] + F.conv2d(x.abs() + e_in, w.abs(), padding=pad))
    e = F.conv2d(e_in, w.abs(), padding=pad) + local
    if epi in (RELU, POOL):
        y = F.relu(y)
    if epi == POOL:
        y, e = F.max_pool2d(y, 2), F.max_pool2d(e, 2)
    return y, e


@pytest.mark.parametrize('cin,cout,k,epi,H,W', LAYER_CASES)
def test_layer(dev, cin, cout, k, epi, H, W):
    from pnr import superpoint as sp
    gen = torch.Generator().manual_seed(H * W + cin)
    w, b = draw(gen, cin, cout, k)
    x = torch.rand((cin, H, W), generator=gen) * 2 - 1
    ref, bound = conv64(x[None].double(), torch.zeros(1, cin, H, W, dtype=torch.float64), w, b, epi)
    out = torch.full(ref.shape[1:], float('nan'), device=dev)
    sp.conv2d(x.to(dev), sp.pack_conv_weight(w).to(dev), b.to(dev), epi, out=out)
    err = (out.cpu().double() - ref[0]).abs()
    print('max err / bound', float((err / bound[0]).max()))
    assert (err <= bound[0]).all()


@pytest.mark.parametrize('H,W', [(2, 3), (15, 17)])
def test_head_epilogues(dev, H, W):
    from pnr import superpoint as sp
    gen = torch.Generator().manual_seed(H)
    x = (torch.rand((256, H, W), generator=gen) * 2 - 1).to(dev)
    for cout, epi in ((65, SOFTMAX), (256, L2NORM)):
        w, b = draw(gen, 256, cout, 1)
        wp, b = sp.pack_conv_weight(w).to(dev), b.to(dev)
        raw = sp.conv2d(x, wp, b, NONE).cpu()
        if epi == L2NORM:
            got = sp.conv2d(x, wp, b, L2NORM).cpu().double()
            ref = raw.double() / raw.double().norm(dim=0, keepdim=True)
            assert ((got - ref).abs() <= 2.0 ** -15 * ref.abs()).all()
            continue
        semi, heat = sp.conv2d(x, wp, b, SOFTMAX, heat=torch.full((8 * H, 8 * W), float('nan'), device=dev))
        assert semi.cpu().numpy().tobytes() == raw.numpy().tobytes()
        dense = np.exp(raw.double().numpy())
        dense = dense / (dense.sum(0) + .00001)
        ref = dense[:-1].transpose(1, 2, 0).reshape(H, W, 8, 8).transpose(0, 2, 1, 3).reshape(8 * H, 8 * W)
        assert (np.abs(heat.cpu().double().numpy() - ref) <= 2.0 ** -17 * ref).all()


@pytest.mark.parametrize('H,W', [(16, 24), (64, 88), (120, 136)])
def test_network(dev, H, W):
    import pnr
    sd = state_dict()
    img = torch.rand((H, W), generator=torch.Generator().manual_seed(H))
    acts = {'img': (img[None, None].double(), torch.zeros(1, 1, H, W, dtype=torch.float64))}
    for name, src, epi in pnr.superpoint.LAYERS:
        acts[name] = conv64(*acts[src], sd[name + '.weight'], sd[name + '.bias'], epi)
    semi, desc = pnr.SuperPointNet(sd, dev).forward(img.to(dev))
    assert semi.shape == (1, 65, H // 8, W // 8) and desc.shape == (1, 256, H // 8, W // 8)
    # E grows by sum |w| ~ sqrt(9 Cin) / 2 per layer and ends far above the values.  What catches a wrong
    # order, pool or head is the second line of each pair: a wiring fault moves the outputs by their own size,
    # rounding in twelve fp32 layers by (K + 2) 2^-24 <= 7e-5 of a layer's terms, so 1e-3 of the largest output
    ref, e = acts['convPb']
    err = (semi.cpu().double() - ref).abs()
    assert (err <= e).all()
    assert err.max() <= 1e-3 * ref.abs().max()
    raw, e = acts['convDb']
    nrm = raw.norm(dim=1, keepdim=True)
    err = (desc.cpu().double() - raw / nrm).abs()
    assert (err <= 2 * e / nrm).all()
    assert err.max() <= 1e-3 * (raw / nrm).abs().max()


def ref_keypoints(heat, thresh, d, border=4):
    """the rules of include/pnr.h pnr_superpoint_keypoints, sequentially"""
    H, W = heat.shape
    ys, xs = np.nonzero(heat >= np.float32(thresh))
    alive = np.zeros((H, W), bool)
    alive[ys, xs] = True
    kept = []
    for k in np.lexsort((ys * W + xs, -heat[ys, xs].astype(np.float64))):
        y, x = ys[k], xs[k]
        if alive[y, x]:
            alive[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1] = False
            if border <= x < W - border and border <= y < H - border:
                kept.append((x, y, heat[y, x]))
    return np.array(kept, np.float32).reshape(-1, 3).T


def crafted(H, W, d, thresh):
    rng = np.random.RandomState(H + d)
    h = rng.uniform(0, 0.03, (H, W)).astype(np.float32)
    h[5:9, 10:16] = 0.02                                         # bitwise-equal blocks: the tie rule
    h[10:12, 30:38] = 0.9
    h[14:23] = 0
    h[15, 20], h[15, 30] = np.float32(thresh), np.nextafter(np.float32(thresh), np.float32(0))
    n = len(h[17, 2::d])
    h[17, 2::d] = np.linspace(0.9, 0.5, n)                       # chains: every other one falls, across tiles
    h[19, 2::d + 1] = np.linspace(0.5, 0.9, len(h[19, 2::d + 1]))  # d + 1 apart: all stay; ascending rank
    h[21, 1::d] = np.linspace(0.2, 0.6, len(h[21, 1::d]))        # a chain decided from the far end
    for c in (3, 4, W - 5, W - 4):
        h[8 + c % 7, c] = 0.7 + 0.001 * c
        h[{3: 3, 4: 4, W - 5: H - 5, W - 4: H - 4}[c], 12 + (3 * c) % 17] = 0.8 + 0.001 * c
    return h


@pytest.mark.parametrize('H,W', [(24, 40), (40, 72)])
@pytest.mark.parametrize('d', [1, 4])
def test_keypoints_exact(dev, H, W, d):
    from pnr import superpoint as sp
    single = np.zeros((H, W), np.float32)
    single[9, 13] = 0.5
    for heat in (crafted(H, W, d, 0.015), np.zeros((H, W), np.float32), single):
        ref = ref_keypoints(heat, 0.015, d)
        pts = sp.keypoints(torch.from_numpy(heat).to(dev), 0.015, d).cpu().numpy()
        assert pts.dtype == np.float32 and pts.shape == ref.shape and pts.tobytes() == ref.tobytes()
    assert ref.shape == (3, 1)


def ref_sample(coarse, pts):
    """float64 bilinear sample at (x / 8 - 0.5, y / 8 - 0.5), zeros outside, renormalised"""
    C, Hc, Wc = coarse.shape
    padded = np.zeros((C, Hc + 2, Wc + 2))
    padded[:, 1:-1, 1:-1] = coarse
    out = np.zeros((C, pts.shape[1]))
    for k, (x, y) in enumerate(pts[:2].T.astype(np.float64)):
        ix, iy = x / 8 - 0.5, y / 8 - 0.5
        x0, y0 = int(np.floor(ix)), int(np.floor(iy))
        wx, wy = ix - x0, iy - y0
        p = padded[:, y0 + 1:y0 + 3, x0 + 1:x0 + 3]
        out[:, k] = (p[:, 0, 0] * (1 - wx) + p[:, 0, 1] * wx) * (1 - wy) + (p[:, 1, 0] * (1 - wx) + p[:, 1, 1] * wx) * wy
    return out / np.linalg.norm(out, axis=0)


def test_sample_descriptors(dev):
    from pnr import superpoint as sp
    rng = np.random.RandomState(5)
    coarse = rng.randn(256, 5, 9)
    coarse = (coarse / np.linalg.norm(coarse, axis=0)).astype(np.float32)
    xy = np.array([(0, 0), (3, 2), (1, 39), (71, 0), (71, 39), (4, 4), (12, 20), (68, 36), (2, 17), (33, 3)] +
                  [(rng.randint(72), rng.randint(40)) for _ in range(6)], np.float32)
    pts = np.ascontiguousarray(np.concatenate([xy.T, np.ones((1, 16), np.float32)]))
    got = sp.sample_descriptors(torch.from_numpy(coarse).to(dev), torch.from_numpy(pts).to(dev)).cpu().numpy()
    assert got.shape == (256, 16) and (np.abs(got - ref_sample(coarse.astype(np.float64), pts)) <= 2.0 ** -20).all()


def test_run_end_to_end(dev):
    import pnr
    H, W = 64, 88
    # zero biases: with them a random network's signal decays below the biases of the last layers, its
    # descriptor map is constant to 1e-7 and a keypoint's nearest neighbour is decided by rounding
    fe = pnr.SuperPointFrontend(state_dict(bias=False), nms_dist=4, conf_thresh=0.015, nn_thresh=0.7)
    img = torch.rand((H, W), generator=torch.Generator().manual_seed(7)).to(dev)
    pts, desc, heat = fe.run(img)
    for t in fe.workspaces(H, W):
        t.view(torch.uint8).fill_(0xFF)
    again = fe.run(img)
    for a, b in zip((pts, desc, heat), again):
        assert a.dtype == torch.float32 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    ref = ref_keypoints(heat.cpu().numpy(), 0.015, 4)
    assert ref.shape[1] > 8 and pts.cpu().numpy().tobytes() == ref.tobytes()
    coarse = fe.net.activations(H, W)['convDb'].cpu().numpy().astype(np.float64)
    assert (np.abs(desc.cpu().numpy() - ref_sample(coarse, ref)) <= 2.0 ** -20).all()
    i1, i2, score = pnr.match_two_way(desc, desc, fe.nn_thresh)
    n = torch.arange(pts.shape[1], device=dev)
    # a float32 unit vector's own fp32 dot is 1 to within tau = 2 D 2^-24 (test_gpu_match.py), and reaches the
    # clip only from above: score = sqrt(2 - 2 dot) is 0 there and at most sqrt(2 tau) otherwise
    print('self-match max score', float(score.max()), 'zeros', int((score == 0).sum()), 'of', len(score))
    assert torch.equal(i1, n) and torch.equal(i2, n) and (score <= np.sqrt(2 * 2 * 256 * U)).all()
    bgr = torch.stack([img, img, img], 2)
    assert fe.run(bgr)[0].shape[0] == 3
    with pytest.raises(ValueError):
        fe.run(img[:20])
    with pytest.raises(ValueError):
        fe.run(img.double())
    with pytest.raises(ValueError):
        pnr.SuperPointNet({k: v for k, v in state_dict().items() if k != 'conv3b.bias'}, dev)
    L = pnr.library()
    one = img.data_ptr()
    assert L.pnr_superpoint_workspace_bytes(20, 88) == 0 and L.pnr_superpoint_workspace_bytes(64, 88) == 64 + 12 * H * W
    assert L.pnr_conv2d_fwd(one, one, one, one, one, 32, 64, 8, 8, 3, 0, None) == -1
    assert L.pnr_superpoint_keypoints(one, 20, 88, 0.015, 4, 4, one, 1 << 30, None) == -1
    assert L.pnr_superpoint_keypoints(one, 64, 88, 0.015, 4, 4, one, 8, None) == -2
