"""IoU modulation vectors (ltr/models/bbreg/atom_iou_net.py:138-170) on gfx950 (iou_mod.hip):

  get_modulation(module, feat, bb)    AtomIoUNet.get_modulation of a reference AtomIoUNet object      -> pt_iou_mod_f32

conv3_1r / conv4_1r computed only on the pixel window PrRoIPool reads under each box (the box is read on the device), both poolings,
fc3_1r and the two fc34 blocks in one call of four launches.  `covered(module, feat, bb)` says whether a call runs here;
install(iou_mod=True) hands every other call to the reference.  The weights are packed once per module state (tap-major weights, bias +
eval BatchNorm as per-channel scale / shift; layout in include/pt_hot.h) and cached outside the module (_packs.py: the key, and when
`refresh(module)` is needed).
"""
import ctypes

import torch

from . import _lib
from ._packs import CPU_TENSOR, PackCache, aligned as _aligned, bn_fold, bn_ok, conv_ok, layers_key, one as _one, tap_major, tensors as _tensors
from .filter import _ptr, _stream, device_guarded, workspace

BLOCKS = ("conv3_1r", "conv4_1r", "fc3_1r", "fc34_3r", "fc34_4r")
POOLS = (("prroi_pool3r", 3), ("prroi_pool4r", 1))
_PACKS = PackCache()
_WHAT = ("get_modulation: eval mode, device fp32, no grad, five Conv2d + BatchNorm2d + ReLU blocks (3x3 pad 1, 3x3 pad 1, 3x3 pad 0, 1x1, "
         "1x1), PrRoIPool 3x3 / 1x1, Cin % 64 == 0, A, B, D, P3, P4 % 16 == 0, H * W <= 4096, bb (n, 4) with n <= 32")


def _valid_conv_ok(conv, k):
    """An undilated, ungrouped k x k Conv2d of stride 1 WITHOUT padding, with a bias (fc3_1r; conv_ok serves the padded ones: a 1 x 1
    convolution's 'same' padding is 0)."""
    return (type(conv) is torch.nn.Conv2d and (_one(conv.kernel_size), _one(conv.stride), _one(conv.padding), _one(conv.dilation))
            == (k, 1, 0, 1) and conv.groups == 1 and conv.bias is not None)


def _blocks(module):
    """[(Conv2d, BatchNorm2d)] of the five blocks if every one has the structure of atom_iou_net.py:26-45 and the channels chain, else
    None."""
    out = []
    for name in BLOCKS:
        blk = getattr(module, name, None)
        if not isinstance(blk, torch.nn.Sequential) or len(blk) != 3:
            return None
        conv, bn, act = blk[0], blk[1], blk[2]
        ok = _valid_conv_ok(conv, 3) if name == "fc3_1r" else conv_ok(conv, 1 if name.startswith("fc34") else 3, 1, True)
        if not (ok and bn_ok(bn, conv.out_channels) and isinstance(act, torch.nn.ReLU)):
            return None
        out.append((conv, bn))
    c3, c4, fc3, f3, f4 = [c for c, _ in out]
    if fc3.in_channels != c3.out_channels or f3.in_channels != fc3.out_channels + c4.out_channels or f4.in_channels != f3.in_channels:
        return None
    return out


def _scales(module):
    """(s3, s4) of the two pooling objects if they pool 3 x 3 and 1 x 1, else None."""
    out = []
    for name, size in POOLS:
        pool = getattr(module, name, None)
        try:
            if (int(pool.pooled_height), int(pool.pooled_width)) != (size, size) or not float(pool.spatial_scale) > 0:
                return None
            out.append(float(pool.spatial_scale))
        except (AttributeError, TypeError, ValueError):
            return None
    return tuple(out)


def _channels(blocks):
    """(Cin3, A, B, Cin4, D, P3, P4)"""
    c3, c4, fc3, f3, f4 = [c for c, _ in blocks]
    return (c3.in_channels, c3.out_channels, fc3.out_channels, c4.in_channels, c4.out_channels, f3.out_channels, f4.out_channels)


def _maps(feat):
    if not isinstance(feat, (list, tuple)) or len(feat) != 2:
        return None
    if not all(isinstance(f, torch.Tensor) and f.dim() == 4 for f in feat):
        return None
    return list(feat)


def pack_weights(module):
    """The pt_iou_mod_f32 pack of an AtomIoUNet (float32, on its device; include/pt_hot.h)."""
    blocks = _blocks(module)
    n = _lib.lib().pt_iou_mod_pack_floats(*_channels(blocks)) if blocks is not None else 0
    if n == 0:
        raise NotImplementedError(_WHAT)
    parts = []
    for conv, bn in blocks:
        s, shift = bn_fold(conv, bn)
        parts += [tap_major(conv).reshape(-1), s.float(), shift.float()]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(module)


def packed_weights(module, blocks=None):
    blocks = _blocks(module) if blocks is None else blocks
    if blocks is None:
        return pack_weights(module)                            # raises
    return _PACKS.get(module, layers_key(blocks), pack_weights)


def covered(module, feat, bb) -> bool:
    blocks, maps, scales = _blocks(module), _maps(feat), _scales(module)
    if blocks is None or maps is None or scales is None or module.training or any(m.training for blk in blocks for m in blk):
        return False
    f3, f4 = maps
    if not all(f.is_cuda and f.dtype == torch.float32 for f in maps) or f3.device != f4.device:
        return False
    if not (isinstance(bb, torch.Tensor) and bb.dim() == 2 and bb.shape[1] == 4 and bb.dtype == torch.float32 and bb.device == f3.device):
        return False
    n = bb.shape[0]
    if f3.shape[0] != n or f4.shape[0] != n:
        return False
    tens = _tensors(blocks)
    if any(t.device != f3.device or t.dtype != torch.float32 for t in tens):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in tens + maps + [bb]):
        return False
    ch = _channels(blocks)
    if f3.shape[1] != ch[0] or f4.shape[1] != ch[3]:
        return False
    return _lib.lib().pt_iou_mod_ws_bytes(n, *ch, f3.shape[2], f3.shape[3], f4.shape[2], f4.shape[3]) > 0


def window(box, scale, H, W):
    """(x0, y0, x1, y1), inclusive, of the pixel window the kernels take for an xywh box on an H x W map, or None where it is empty
    (pt_iou_mod_window; host only)."""
    out = (ctypes.c_int * 4)()
    rc = _lib.lib().pt_iou_mod_window((ctypes.c_float * 4)(*[float(v) for v in box]), float(scale), int(H), int(W), out)
    if rc < 0:
        _lib.check(rc, "pt_iou_mod_window")
    return None if rc else tuple(out)


@device_guarded
def get_modulation(module, feat, bb, checked=False):
    """reference: AtomIoUNet.get_modulation -> (fc34_3_r (n, P3, 1, 1), fc34_4_r (n, P4, 1, 1))."""
    for f in list(_maps(feat) or []) + [bb]:
        if isinstance(f, torch.Tensor) and not f.is_cuda:
            raise RuntimeError(CPU_TENSOR)
    if not checked and not covered(module, feat, bb):
        raise NotImplementedError(_WHAT)
    blocks = _blocks(module)
    ch = _channels(blocks)
    s3, s4 = _scales(module)
    pack = packed_weights(module, blocks)
    f3, f4, boxes = _aligned(feat[0]), _aligned(feat[1]), _aligned(bb)      # a leading slice x[:n] is dense: taken as it is
    n, (H3, W3), (H4, W4) = boxes.shape[0], f3.shape[2:], f4.shape[2:]
    out3 = torch.empty((n, ch[5], 1, 1), dtype=torch.float32, device=f3.device)
    out4 = torch.empty((n, ch[6], 1, 1), dtype=torch.float32, device=f3.device)
    L = _lib.lib()
    ws = workspace(L.pt_iou_mod_ws_bytes(n, *ch, H3, W3, H4, W4), f3.device)
    rc = L.pt_iou_mod_f32(_ptr(f3), _ptr(f4), _ptr(boxes), _ptr(pack), _ptr(out3), _ptr(out4), n, *ch, H3, W3, H4, W4, s3, s4,
                          _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_iou_mod_f32")
    return out3, out4
