"""Box label encoders (ltr/models/lwl/label_encoder.py:58-216, ltr/models/rts/label_encoder.py:106-265) on gfx950 (box_enc.hip): the
box-to-mask initialisation of RTS (STAHelper.predict_mask -> STANet.forward) and of box-initialised LWL (lwl.py:53-65).

  forward(module, bb, feat, sz)    ResidualDS16FeatSWBox.forward              -> pt_box_enc_f32      (label_enc, sample_w or None)
                                   ResidualDS16FeatSWBoxCatMultiBlock.forward -> pt_box_cat_enc_f32  label_enc

The box is read on the device (the reference synchronises with the host once per box); the binary mask is rasterised inside the stem
(FeatSWBox: nothing of image size is stored) or evaluated by the resize kernel (Cat), and the 3x3 convolutions over the concatenation of
feature and mask encoding read their input channels from the two tensors: no `torch.cat`.  `covered(module, bb, feat, sz)` says whether a
call runs here; install(box_encoder=True) hands every other call to the reference.  use_gauss=True, training mode and calls that need a
gradient are not served.  The weights are packed once per module state (layout in include/pt_hot.h; bias and eval BatchNorm as
per-channel scale / shift folded in float64) and cached outside the module (_packs.py: the key, and when `refresh(module)` is needed).
"""
import ctypes

import torch

from . import _lib
from ._packs import (CPU_TENSOR, PackCache, _basic_block, _conv_block, bn_fold, conv_ok, dev_f32 as _dev_f32, layers_key, one as _one,
                     quiet as _quiet, tap_major, tensors as _tensors)
from .filter import _ptr, _stream, device_guarded, workspace

_PACKS = PackCache()
BOX, CAT = "ResidualDS16FeatSWBox", "ResidualDS16FeatSWBoxCatMultiBlock"
_REASON = ("box label encoder: eval mode, use_gauss=False, device fp32 feature, no grad, the structure of ResidualDS16FeatSWBox (bb 3-D) or "
           "ResidualDS16FeatSWBoxCatMultiBlock (bb 2-D), layer dims multiples of 16 up to 128 (trunk up to 64), feat_dim a multiple of 16 "
           "up to 1024")


class _Info:
    """What the recogniser found: kind (BOX / CAT), [(Conv2d, BatchNorm2d or None)] in module order, the dims the library takes,
    feat_dim, whether label_pred ends in a ReLU, whether the module has samp_w_pred."""

    def __init__(self, kind, layers, dims, feat_dim, final_relu, with_sw):
        self.kind, self.layers, self.dims, self.feat_dim, self.final_relu, self.with_sw = kind, layers, dims, feat_dim, final_relu, with_sw


def _head(seq):
    """((Conv2d, BatchNorm2d or None), has ReLU) of label_pred, a conv_block with or without its ReLU."""
    for relu in (True, False):
        hit = _conv_block(seq, 1, relu)
        if hit is not None:
            return hit, relu
    return None, False


def _recognise(module):
    """_Info if `module` has exactly the structure of one of the two classes with use_gauss=False, else None."""
    kind = type(module).__name__
    if kind not in (BOX, CAT) or getattr(module, "use_gauss", True) is not False or not hasattr(module, "label_pred"):
        return None
    head, final_relu = _head(module.label_pred)
    if head is None:
        return None
    if kind == CAT:
        res = getattr(module, "res", None)
        if not isinstance(res, torch.nn.Sequential) or len(res) < 1:
            return None
        blocks = [_basic_block(b, 1) for b in res]
        if any(b is None for b in blocks):
            return None
        widths = [b[0][0].out_channels for b in blocks]
        chain = all(b[0][0].in_channels == c for b, c in zip(blocks[1:], widths)) and head[0].in_channels == widths[-1]
        feat_dim = blocks[0][0][0].in_channels - 1
        if not chain or feat_dim < 1:
            return None
        return _Info(CAT, [l for b in blocks for l in b] + [head], tuple(widths) + (head[0].out_channels,), feat_dim, final_relu, False)
    if not all(hasattr(module, a) for a in ("conv_block", "pool", "res1", "res2", "res3", "use_sample_w")):
        return None
    pool = module.pool
    if type(pool) is not torch.nn.MaxPool2d or (_one(pool.kernel_size), _one(pool.stride), _one(pool.padding), _one(pool.dilation)) != (3, 2, 1, 1):
        return None
    if pool.ceil_mode or pool.return_indices:
        return None
    stem = _conv_block(module.conv_block, 2, True)
    b1, b2, b3 = _basic_block(module.res1, 2), _basic_block(module.res2, 2), _basic_block(module.res3, 1)
    if stem is None or b1 is None or b2 is None or b3 is None:
        return None
    with_sw = bool(module.use_sample_w)
    sw = getattr(module, "samp_w_pred", None)
    if with_sw and not conv_ok(sw, 3, 1, True):
        return None
    c0, c1, c2, c3, f = stem[0].out_channels, b1[0][0].out_channels, b2[0][0].out_channels, b3[0][0].out_channels, head[0].out_channels
    feat_dim = b3[0][0].in_channels - c2
    chain = (stem[0].in_channels == 1 and b1[0][0].in_channels == c0 and b2[0][0].in_channels == c1 and feat_dim >= 1
             and head[0].in_channels == c3 and (not with_sw or (sw.in_channels, sw.out_channels) == (c3, f)))
    if not chain:
        return None
    layers = [stem] + b1 + b2 + b3 + [head] + ([(sw, None)] if with_sw else [])
    return _Info(BOX, layers, (c0, c1, c2, c3, f), feat_dim, final_relu, with_sw)


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


def _pack_floats(info):
    L = _lib.lib()
    if info.kind == BOX:
        return L.pt_box_enc_pack_floats(*info.dims, info.feat_dim, int(info.with_sw))
    return L.pt_box_cat_enc_pack_floats(len(info.dims) - 1, _int_array(info.dims), info.feat_dim)


def _weights(conv, order=None, padded=True):
    """(Cout, 9 * ceil16(Cin)) tap-major weights, the input channels taken in `order` and padded with zeros to a multiple of 16 (the
    layers of k_bx_conv; the trunk's keep the mask label encoder's layout, `padded` False)."""
    o, i = conv.out_channels, conv.in_channels
    w = tap_major(conv).reshape(o, 9, i)
    if order is not None:
        w = w[:, :, torch.as_tensor(order, device=w.device)]
    pad = -i % 16 if padded else 0
    if pad:
        w = torch.cat([w, w.new_zeros(o, 9, pad)], 2)
    return w.reshape(o, -1)


def _group(layers, order=None, padded=True):
    """One fused layer of the pack from the convolutions that share an input: weights | scales | shifts."""
    s, b = zip(*[bn_fold(c, bn) for c, bn in layers])
    return [torch.cat([_weights(c, order, padded) for c, _ in layers]).reshape(-1), torch.cat(s).float(), torch.cat(b).float()]


def pack_weights(module):
    """The pt_box_enc_f32 / pt_box_cat_enc_f32 pack of a box label encoder (float32, on its device; include/pt_hot.h)."""
    info = _recognise(module)
    n = _pack_floats(info) if info is not None else 0
    if n == 0:
        raise NotImplementedError(_REASON)
    ly, parts = info.layers, []
    if info.kind == BOX:
        c2, fd = info.dims[2], info.feat_dim
        order = list(range(c2, c2 + fd)) + list(range(c2))             # the module concatenates [trunk | feat], the kernel reads [feat | trunk]
        for group in ([0], [1, 2], [3], [4, 5], [6]):
            parts += _group([ly[k] for k in group], padded=False)
        parts += _group([ly[7], ly[8]], order) + _group([ly[9]]) + _group(ly[10:])
    else:
        for b in range(len(info.dims) - 1):
            parts += _group([ly[3 * b], ly[3 * b + 1]]) + _group([ly[3 * b + 2]])
        parts += _group([ly[-1]])
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(module)


def packed_weights(module, info=None):
    info = _recognise(module) if info is None else info
    if info is None:
        return pack_weights(module)                            # raises
    return _PACKS.get(module, layers_key(info.layers), pack_weights)


def _image_size(sz):
    try:
        hw = [int(v) for v in (sz.tolist() if isinstance(sz, torch.Tensor) else list(sz))[-2:]]
    except (TypeError, ValueError):
        return None
    return tuple(hw) if len(hw) == 2 else None


def _call(module, bb, feat, sz):
    """(info, n, (H, W), (C, h, w)) of a call the kernels serve, else None."""
    info = _recognise(module)
    if info is None or not isinstance(bb, torch.Tensor) or not isinstance(feat, torch.Tensor):
        return None
    if bb.dim() != (3 if info.kind == BOX else 2) or bb.shape[-1] != 4 or bb.is_complex() or not bb.is_cuda or bb.numel() == 0:
        return None
    if not _dev_f32(feat) or feat.dim() < 4 or feat.device != bb.device or feat.numel() == 0:
        return None
    image = _image_size(sz)
    if image is None or not _quiet(module, _tensors(info.layers) + [feat], feat) or (torch.is_grad_enabled() and bb.requires_grad):
        return None
    n = bb.numel() // 4
    C, h, w = feat.shape[-3:]
    if feat.numel() != n * C * h * w or C != info.feat_dim:
        return None
    L = _lib.lib()
    if info.kind == BOX:
        need = L.pt_box_enc_ws_bytes(n, *image, h, w, *info.dims, info.feat_dim)
    else:
        need = L.pt_box_cat_enc_ws_bytes(n, *image, h, w, len(info.dims) - 1, _int_array(info.dims), info.feat_dim)
    return (info, n, image, (C, h, w)) if need > 0 else None


def covered(module, bb, feat, sz) -> bool:
    return _call(module, bb, feat, sz) is not None


def _feature_view(feat, n, C, h, w):
    """(tensor, image stride in floats): `feat` as n images of dense channel planes, copied only where its strides are not of that kind."""
    f = feat.reshape(n, C, h, w)                               # a view wherever the leading dimensions merge
    if f.stride()[1:] != (h * w, w, 1) or (n > 1 and f.stride(0) < C * h * w):
        f = f.contiguous()
    return f, (f.stride(0) if n > 1 else C * h * w)


@device_guarded
def forward(module, bb, feat, sz, checked=False):
    """reference: ResidualDS16FeatSWBox.forward -> (label_enc, sample_w or None), each (frames, seq, F, h, w);
    ResidualDS16FeatSWBoxCatMultiBlock.forward -> label_enc (N, 1, F, h, w)."""
    for t in (bb, feat):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError(CPU_TENSOR)
    if checked:                                                # the dispatcher has asked covered(): only the sizes are read again
        info, (H, W), n = _recognise(module), _image_size(sz), bb.numel() // 4
        C, h, w = feat.shape[-3:]
    else:
        call = _call(module, bb, feat, sz)
        if call is None:
            raise NotImplementedError(_REASON)
        info, n, (H, W), (C, h, w) = call
    pack = packed_weights(module, info)
    boxes = bb.detach().reshape(n, 4)
    if boxes.dtype != torch.float32:                           # int() of the reference acts on the value as it is stored
        boxes = (boxes.trunc() if boxes.is_floating_point() else boxes).to(torch.float32)
    boxes = boxes.contiguous()
    f, f_img = _feature_view(feat.detach(), n, C, h, w)
    F = info.dims[-1]
    L = _lib.lib()
    if info.kind == BOX:
        enc = torch.empty((bb.shape[0], bb.shape[1], F, h, w), dtype=torch.float32, device=f.device)
        sw = torch.empty_like(enc) if info.with_sw else None
        ws = workspace(L.pt_box_enc_ws_bytes(n, H, W, h, w, *info.dims, C), f.device)
        rc = L.pt_box_enc_f32(_ptr(boxes), _ptr(f), f_img, _ptr(pack), _ptr(enc), _ptr(sw) if info.with_sw else None, n, H, W, h, w,
                              *info.dims, C, int(info.final_relu), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "pt_box_enc_f32")
        return enc, sw
    dims = _int_array(info.dims)
    enc = torch.empty((n, 1, F, h, w), dtype=torch.float32, device=f.device)
    ws = workspace(L.pt_box_cat_enc_ws_bytes(n, H, W, h, w, len(info.dims) - 1, dims, C), f.device)
    rc = L.pt_box_cat_enc_f32(_ptr(boxes), _ptr(f), f_img, _ptr(pack), _ptr(enc), n, H, W, h, w, len(info.dims) - 1, dims, C,
                              int(info.final_relu), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_box_cat_enc_f32")
    return enc
