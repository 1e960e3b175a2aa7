"""SuperPoint on the device (src/demo_superpoint.py:78-293, built by src/frame.py:271): the 12-convolution
network on this project's fp32-MFMA convolution (csrc/conv.hip), the softmax / depth-to-space heatmap and the
descriptor normalisation as its epilogues, threshold + greedy NMS + border cut and the bilinear descriptor
sample in csrc/keypoints.hip.  image -> keypoints -> descriptors -> pnr.match_two_way never leaves the device.

Everything is float32 and batch 1.  H and W are positive multiples of 8.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib

NONE, RELU, RELU_POOL2, SOFTMAX_HEATMAP, L2NORM = range(5)  # include/pnr.h pnr_conv_epilogue
CHANNELS_IN, CHANNELS_OUT = (1, 64, 128, 256), (64, 128, 256, 65)
BORDER = 4  # demo_superpoint.py:144 border_remove
# (name, input, epilogue) in launch order; 'x4' is conv4b's output, which feeds both heads
LAYERS = (('conv1a', 'img', RELU), ('conv1b', 'conv1a', RELU_POOL2), ('conv2a', 'conv1b', RELU),
          ('conv2b', 'conv2a', RELU_POOL2), ('conv3a', 'conv2b', RELU), ('conv3b', 'conv3a', RELU_POOL2),
          ('conv4a', 'conv3b', RELU), ('conv4b', 'conv4a', RELU), ('convPa', 'conv4b', RELU),
          ('convPb', 'convPa', SOFTMAX_HEATMAP), ('convDa', 'conv4b', RELU), ('convDb', 'convDa', L2NORM))


def _f32(t, what, dim=None):
    _lib.require_cuda(t)
    if t.dtype != torch.float32 or not t.is_contiguous() or (dim is not None and t.dim() != dim):
        raise ValueError(f'pnr.superpoint: {what} is a contiguous float32 tensor' + (f' of {dim} dims' if dim else ''))
    return t


def _size(H, W):
    if H <= 0 or W <= 0 or H % 8 or W % 8:
        raise ValueError(f'pnr.superpoint: H = {H}, W = {W} are not positive multiples of 8')


def pack_conv_weight(weight):
    """conv.weight (Cout, Cin, k, k) -> the kernel's [k*k][Cin][Cout padded to a multiple of 64] (host permute)."""
    cout, cin, kh, kw = weight.shape
    if kh != kw or kh not in (1, 3) or cin not in CHANNELS_IN or cout not in CHANNELS_OUT:
        raise ValueError(f'pnr.superpoint: no kernel for a convolution weight of shape {tuple(weight.shape)}')
    w = weight.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    return torch.nn.functional.pad(w, (0, -cout % 64)).contiguous()


def conv2d(x, w_packed, bias, epilogue=NONE, out=None, heat=None):
    """One layer (pnr_conv2d_fwd): x (Cin, H, W), w_packed from pack_conv_weight, bias (Cout,).  Returns out
    (Cout, H, W), or (Cout, H/2, W/2) for RELU_POOL2; SOFTMAX_HEATMAP returns (out, heat (8H, 8W))."""
    _f32(x, 'x', 3), _f32(w_packed, 'w_packed', 3), _f32(bias, 'bias', 1)
    cin, H, W = x.shape
    cout, k = bias.shape[0], {1: 1, 9: 3}.get(w_packed.shape[0])
    if k is None or w_packed.shape[1] != cin or w_packed.shape[2] != cout + (-cout % 64):
        raise ValueError('pnr.superpoint: w_packed does not fit x and bias')
    if cin not in CHANNELS_IN or cout not in CHANNELS_OUT or epilogue not in range(5):
        raise ValueError(f'pnr.superpoint: no kernel for Cin = {cin}, Cout = {cout}, epilogue {epilogue}')
    if epilogue == RELU_POOL2 and (H % 2 or W % 2):
        raise ValueError('pnr.superpoint: RELU_POOL2 needs even H and W')
    if (epilogue == SOFTMAX_HEATMAP and (cout, k) != (65, 1)) or (epilogue == L2NORM and (cout, k) != (256, 1)) or \
            (cin == 1 and (k != 3 or epilogue > RELU)):
        raise ValueError(f'pnr.superpoint: epilogue {epilogue} does not serve {cin}->{cout}, kernel {k}')
    shape = (cout, H // 2, W // 2) if epilogue == RELU_POOL2 else (cout, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if epilogue == SOFTMAX_HEATMAP and heat is None:
        heat = torch.empty((8 * H, 8 * W), dtype=torch.float32, device=x.device)
    if _f32(out, 'out').shape != shape or (heat is not None and _f32(heat, 'heat').shape != (8 * H, 8 * W)):
        raise ValueError('pnr.superpoint: out / heat have the wrong shape')
    _lib.check(_lib.load().pnr_conv2d_fwd(_lib.ptr(x), _lib.ptr(w_packed), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(heat),
                                          cin, cout, H, W, k, epilogue, _lib.stream_of(x.device)), 'conv2d_fwd')
    return (out, heat) if epilogue == SOFTMAX_HEATMAP else out


def keypoints(heat, conf_thresh=0.015, nms_dist=4, border=BORDER, workspace=None):
    """pts (3, N) float32 [x; y; conf] of a heatmap (H, W): threshold, greedy NMS under the total order
    (confidence descending, then row-major index ascending), border cut, in that order (pnr_superpoint_keypoints).
    One host read (the count); the sort of the packed keys is torch's."""
    H, W = _f32(heat, 'heat', 2).shape
    _size(H, W)
    if not conf_thresh > 0 or not 0 <= nms_dist <= 64:
        raise ValueError('pnr.superpoint: conf_thresh is positive and nms_dist in [0, 64]')
    lib = _lib.load()
    nbytes = lib.pnr_superpoint_workspace_bytes(H, W)
    if nbytes == 0:
        raise ValueError(f'pnr.superpoint: a {H} x {W} heatmap is out of range')
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=heat.device)
    if ws.numel() < nbytes or ws.device != heat.device:
        raise ValueError('pnr.superpoint: the workspace was made for another size or device')
    _lib.check(lib.pnr_superpoint_keypoints(_lib.ptr(heat), H, W, float(conf_thresh), int(nms_dist), int(border),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_of(heat.device)), 'superpoint_keypoints')
    n = int(ws[:4].view(torch.int32).item())
    keys = torch.sort(ws[64:64 + 8 * n].view(torch.int64), descending=True).values
    p = 0xFFFFFFFF - (keys & 0xFFFFFFFF)
    conf = (keys >> 32).to(torch.int32).view(torch.float32)
    return torch.stack([(p % W).float(), (p // W).float(), conf])


def sample_descriptors(coarse, pts):
    """desc (256, N): the unit-length bilinear sample of the normalised coarse map (256, Hc, Wc) at the
    keypoints pts (3, N) (pnr_superpoint_sample_desc) -- what pnr.match_two_way takes."""
    _f32(coarse, 'coarse', 3), _f32(pts, 'pts', 2)
    if coarse.shape[0] != 256 or pts.shape[0] != 3 or pts.device != coarse.device:
        raise ValueError('pnr.superpoint: coarse is (256, Hc, Wc) and pts (3, N) on one device')
    N = pts.shape[1]
    desc = torch.empty((256, N), dtype=torch.float32, device=coarse.device)
    _lib.check(_lib.load().pnr_superpoint_sample_desc(_lib.ptr(coarse), coarse.shape[1], coarse.shape[2], _lib.ptr(pts),
                                                      N, _lib.ptr(desc), _lib.stream_of(coarse.device)), 'sample_desc')
    return desc


class SuperPointNet(object):
    """The network of demo_superpoint.py:78-131 from its `state_dict` (convXY.weight / convXY.bias), twelve
    launches.  `forward(img)` takes a (H, W) or (1, 1, H, W) image and returns semi (1, 65, H/8, W/8) and the
    normalised desc (1, 256, H/8, W/8); `heat` then holds the (H, W) heatmap of that image.  Activations are
    allocated once per image size and reused: the returned tensors are views that the next call overwrites."""

    def __init__(self, state_dict, device='cuda:0'):
        self.device = torch.device(device)
        self.params = {}
        for name, _, _ in LAYERS:
            for part in ('weight', 'bias'):
                if f'{name}.{part}' not in state_dict:
                    raise ValueError(f'pnr.SuperPointNet: the state_dict has no {name}.{part}')
            w, b = state_dict[f'{name}.weight'], state_dict[f'{name}.bias']
            if b.dim() != 1 or w.dim() != 4 or b.shape[0] != w.shape[0]:
                raise ValueError(f'pnr.SuperPointNet: {name} has a malformed weight or bias')
            self.params[name] = (pack_conv_weight(w).to(self.device), w.shape[0],
                                 b.detach().to(torch.float32).contiguous().to(self.device))
        self._acts = {}
        self.heat = None

    def activations(self, H, W):
        """name -> output buffer of every layer, and 'heat', for an H x W image."""
        _size(H, W)
        if (H, W) not in self._acts:
            acts, shapes = {}, {'img': (H, W)}
            for name, src, epi in LAYERS:
                h, w = shapes[src]
                shapes[name] = (h // 2, w // 2) if epi == RELU_POOL2 else (h, w)
                acts[name] = torch.empty((self.params[name][1],) + shapes[name], dtype=torch.float32, device=self.device)
            acts['heat'] = torch.empty((H, W), dtype=torch.float32, device=self.device)
            self._acts[(H, W)] = acts
        return self._acts[(H, W)]

    def forward(self, img, on_layer=None):
        if img.dim() == 4 and img.shape[:2] == (1, 1):
            img = img[0, 0]
        H, W = _f32(img, 'img', 2).shape
        if img.device != self.device:
            raise ValueError('pnr.SuperPointNet: the image is on another device')
        acts = self.activations(H, W)
        for name, src, epi in LAYERS:
            x = img[None] if src == 'img' else acts[src]
            wp, _, b = self.params[name]
            if on_layer is not None:
                on_layer(name, True)
            conv2d(x, wp, b, epi, out=acts[name], heat=acts['heat'] if epi == SOFTMAX_HEATMAP else None)
            if on_layer is not None:
                on_layer(name, False)
        self.heat = acts['heat']
        return acts['convPb'][None], acts['convDb'][None]

    __call__ = forward


class SuperPointFrontend(object):
    """demo_superpoint.py:134-293 on the device.  `weights`: a state_dict or a path to one.  `run(img)` takes a
    float32 (H, W) grey image in [0, 1], or (H, W, 3) BGR (cv2's grey weights), on the device and returns
    pts (3, N) [x; y; conf], desc (256, N) unit descriptors and the (H, W) heatmap, all device tensors; with no
    keypoint it returns ((3, 0), (256, 0), heatmap) where the reference returns Nones."""

    def __init__(self, weights, nms_dist=4, conf_thresh=0.015, nn_thresh=0.7, device='cuda:0'):
        if isinstance(weights, (str, bytes)) or hasattr(weights, '__fspath__'):
            weights = torch.load(weights, map_location='cpu')
        self.net = SuperPointNet(weights, device)
        self.nms_dist, self.conf_thresh, self.nn_thresh = nms_dist, conf_thresh, nn_thresh
        self.cell, self.border_remove = 8, BORDER
        self._ws = {}

    def workspaces(self, H, W):
        """Every buffer a run at H x W reuses (their contents before a run do not matter)."""
        acts = self.net.activations(H, W)
        if (H, W) not in self._ws:
            self._ws[(H, W)] = torch.empty(_lib.load().pnr_superpoint_workspace_bytes(H, W), dtype=torch.uint8,
                                           device=self.net.device)
        return list(acts.values()) + [self._ws[(H, W)]]

    def run(self, img):
        _lib.require_cuda(img)
        if img.dtype != torch.float32:
            raise ValueError('pnr.SuperPointFrontend: the image is float32')
        if img.dim() == 3 and img.shape[2] == 3:
            img = (img * img.new_tensor([0.114, 0.587, 0.299])).sum(2)
        if img.dim() != 2:
            raise ValueError('pnr.SuperPointFrontend: the image is (H, W) grey or (H, W, 3) BGR')
        H, W = img.shape
        ws = self.workspaces(H, W)[-1]
        _, coarse = self.net.forward(img.contiguous())
        pts = keypoints(self.net.heat, self.conf_thresh, self.nms_dist, self.border_remove, workspace=ws)
        return pts, sample_descriptors(coarse[0], pts), self.net.heat.clone()
