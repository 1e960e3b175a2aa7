"""Device cache of the MFMA-ordered weight image (pnr_mlp_pack, csrc/mlp.hip:k_pack).

The image is a pure function of the 11 decoder tensors; it is rebuilt only when one of them
changed (data pointer or in-place version counter, e.g. after optimizer.step()).  One pack is a
~2 MB device-to-device permutation, negligible next to a render call.

A Mapper iteration repacks after every Adam step, on its critical path: a caller that runs only the
f16x3 kernels asks for their images alone (`image(params, prec=PNR_PREC_F16X3)`, pnr_mlp_pack2 ABI 14:
no fp32 / bf16 images, bit for bit the f16x3 parts of a full pack); a later call that needs every
precision repacks.

A Mapper step whose reduction also ran Adam (pnr_map_step_adam) has already formed the new weights'
scales: it leaves the image "stale, scales fresh" (`scales_fresh`), and the next f16x3-only repack of
the same tensors is the images' launch alone (pnr_mlp_pack_scaled) -- or none here at all, when the
caller packs inside a launch of its own (`adopt`: MapGraph's grouped head).  Any `invalidate()`, a
changed tensor or a request for every precision drops the mark and packs in full.
"""
from __future__ import annotations

import torch

from . import _lib


class PackedMLP:
    """Image of the 11 reference tensors (pnr_mlp_pack)."""
    _floats = 'pnr_mlp_packed_floats'
    _pack = 'pnr_mlp_pack2'
    _arr = 'PtrArray'
    _pack_scaled = 'pnr_mlp_pack_scaled'

    def __init__(self):
        self._key = None
        self._img = None
        self._cover_all = False  # the image holds every precision's parts (else the f16x3 ones only)
        self._scales = None      # (key, device floats [5 scl | 5 inv]) of the tensors' current values

    def invalidate(self):
        """Force a re-pack (weights were written in place outside autograd, e.g. pnr_adam_step)."""
        self._key = None
        self._cover_all = False
        self._scales = None

    @staticmethod
    def _key_of(params):
        return tuple((t.data_ptr(), t._version, t.device.index) for t in params)

    def scales_fresh(self, params, scales):
        """The image is stale but `scales` (device floats, [5 scl | 5 inv]) are those of `params` as they
        now stand (pnr_map_step_adam wrote both)."""
        self.invalidate()
        if self._pack_scaled is not None and all(t.dtype == torch.float32 and t.is_contiguous() for t in params):
            self._scales = (self._key_of(params), scales)

    def _fresh(self, params, key):
        """The fresh scales, if they belong to these tensors and an image of this device exists."""
        if self._scales is None or self._scales[0] != key or self._img is None \
                or self._img.device != params[0].device:
            return None
        return self._scales[1]

    def adopt(self, params):
        """For a caller that runs the stage-2-only pack inside a launch of its own (pnr_window_sample_pack):
        (tensor pointer array, image, scales) when the scales are fresh, and the image then counts as
        packed for the f16x3 kernels; None otherwise (pack through `image`)."""
        key = self._key_of(params)
        scales = self._fresh(params, key)
        if scales is None:
            return None
        arr = getattr(_lib, self._arr)(*[t.data_ptr() for t in params])
        self._key = key
        self._cover_all = False
        self._scales = None
        return arr, self._img, scales

    def image(self, params, prec=None) -> torch.Tensor:
        """The packed image of `params`; prec = PNR_PREC_F16X3 (int): only the f16x3 kernels will read it."""
        key = self._key_of(params)
        only = prec == _lib.PRECISIONS['f16x3']
        if self._img is not None and key == self._key and (self._cover_all or only):
            return self._img
        _lib.require_cuda(*params)
        lib = _lib.load()
        dev = params[0].device
        scales = self._fresh(params, key) if only else None
        self._scales = None
        if scales is not None:  # the scale stage ran with the step: the images' launch alone
            arr = getattr(_lib, self._arr)(*[t.data_ptr() for t in params])
            _lib.check(getattr(lib, self._pack_scaled)(arr, _lib.ptr(self._img), _lib.ptr(scales),
                                                       _lib.stream_of(dev)), self._pack_scaled)
            self._key = key
            self._cover_all = False
            return self._img
        if self._img is None or self._img.device != dev:
            self._img = torch.empty(getattr(lib, self._floats)(), device=dev, dtype=torch.float32)
        srcs = [t.detach().float().contiguous() for t in params]
        arr = getattr(_lib, self._arr)(*[t.data_ptr() for t in srcs])
        flags = _lib.PACK_F16X3_ONLY if only else 0
        _lib.check(getattr(lib, self._pack)(arr, _lib.ptr(self._img), flags, _lib.stream_of(dev)), self._pack)
        self._srcs = srcs  # keep converted copies alive until the pack kernel ran
        self._key = key
        self._cover_all = not only
        return self._img


class PackedFC(PackedMLP):
    """Image of the 8 fc_c tensors of MLP(c_dim=32) (pnr_fc_pack)."""
    _floats = 'pnr_fc_packed_floats'
    _pack = 'pnr_fc_pack2'
    _arr = 'FcPtrArray'
    _pack_scaled = None
