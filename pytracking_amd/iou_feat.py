"""IoU feature extraction (ltr/models/bbreg/atom_iou_net.py:172-179) on gfx950 (iou_feat.hip):

  get_iou_feat(module, feat2)    AtomIoUNet.get_iou_feat of a reference AtomIoUNet object      -> pt_iou_feat_f32

Both towers -- conv3_2t(conv3_1t(layer2)) and conv4_2t(conv4_1t(layer3)), each block Conv2d(3x3, pad 1, bias) -> BatchNorm2d (eval) ->
ReLU -- in one call.  `covered(module, feat2)` says whether a call runs here; install(iou_feat=True) hands every other call to the
reference.  The weights are packed once per module state (tap-major weights, bias + eval BatchNorm as per-channel scale / shift; layout
in include/pt_hot.h) and cached outside the module (_packs.py: the key, and when `refresh(module)` is needed).
"""
import torch

from . import _lib
from ._packs import CPU_TENSOR, PackCache, aligned as _aligned, bn_fold, bn_ok, conv_ok, layers_key, tap_major, tensors as _tensors
from .filter import _ptr, _stream, device_guarded, workspace

BLOCKS = ("conv3_1t", "conv3_2t", "conv4_1t", "conv4_2t")
_PACKS = PackCache()


def _blocks(module):
    """[(Conv2d, BatchNorm2d)] of the four blocks if every one has the structure of atom_iou_net.py:7-12, else None."""
    out = []
    for name in BLOCKS:
        blk = getattr(module, name, None)
        if not isinstance(blk, torch.nn.Sequential) or len(blk) != 3:
            return None
        conv, bn, act = blk[0], blk[1], blk[2]
        if not (conv_ok(conv, 3, 1, True) and bn_ok(bn, conv.out_channels) and isinstance(act, torch.nn.ReLU)):
            return None
        out.append((conv, bn))
    if out[1][0].in_channels != out[0][0].out_channels or out[3][0].in_channels != out[2][0].out_channels:
        return None
    return out


def _channels(blocks):
    return (blocks[0][0].in_channels, blocks[0][0].out_channels, blocks[1][0].out_channels,
            blocks[2][0].in_channels, blocks[2][0].out_channels, blocks[3][0].out_channels)


def _maps(feat2):
    """The two (n, C, H, W) maps of the reference's argument (5-D tensors reshaped as atom_iou_net.py:174), or None."""
    if not isinstance(feat2, (list, tuple)) or len(feat2) != 2:
        return None
    if not all(isinstance(f, torch.Tensor) and f.dim() in (4, 5) for f in feat2):
        return None
    return [f.reshape(-1, *f.shape[-3:]) if f.dim() == 5 else f for f in feat2]


def pack_weights(module):
    """The pt_iou_feat_f32 pack of an AtomIoUNet (float32, on its device; include/pt_hot.h)."""
    blocks = _blocks(module)
    n = _lib.lib().pt_iou_feat_pack_floats(*_channels(blocks)) if blocks is not None else 0
    if n == 0:
        raise NotImplementedError("get_iou_feat: four Conv2d(3x3, pad 1, bias) + BatchNorm2d + ReLU blocks, Cin % 64 == 0, "
                                  "Cmid % 16 == 0, Cout % 16 == 0")
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


def covered(module, feat2) -> bool:
    blocks = _blocks(module)
    maps = _maps(feat2)
    if blocks is None or maps is None or module.training or any(m.training for blk in blocks for m in blk):
        return False
    f3, f4 = maps
    if not all(f.is_cuda and f.dtype == torch.float32 for f in maps) or f3.device != f4.device or f3.shape[0] != f4.shape[0]:
        return False
    tens = _tensors(blocks)
    if any(t.device != f3.device or t.dtype != torch.float32 for t in tens):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in tens + list(feat2)):
        return False
    ch = _channels(blocks)
    if f3.shape[1] != ch[0] or f4.shape[1] != ch[3]:
        return False
    n = f3.shape[0]
    return _lib.lib().pt_iou_feat_ws_bytes(n, ch[0], ch[1], ch[2], f3.shape[2], f3.shape[3], ch[3], ch[4], ch[5], f4.shape[2],
                                           f4.shape[3]) > 0


@device_guarded
def get_iou_feat(module, feat2, checked=False):
    """reference: AtomIoUNet.get_iou_feat -> (c3_t (n, Cout3, H3, W3), c4_t (n, Cout4, H4, W4))."""
    maps = _maps(feat2)
    for f in (maps or []):
        if not f.is_cuda:
            raise RuntimeError(CPU_TENSOR)
    if not checked and not covered(module, feat2):
        raise NotImplementedError("get_iou_feat: eval mode, device fp32, no grad, Conv2d(3x3, pad 1, bias) + BatchNorm2d + ReLU blocks, "
                                  "Cin % 64 == 0, Cmid % 16 == 0, Cout % 16 == 0, H * W <= 4096, n <= 8")
    blocks = _blocks(module)
    ch = _channels(blocks)
    pack = packed_weights(module, blocks)
    f3, f4 = _aligned(maps[0]), _aligned(maps[1])
    n, (H3, W3), (H4, W4) = f3.shape[0], f3.shape[2:], f4.shape[2:]
    c3 = torch.empty((n, ch[2], H3, W3), dtype=torch.float32, device=f3.device)
    c4 = torch.empty((n, ch[5], H4, W4), dtype=torch.float32, device=f3.device)
    L = _lib.lib()
    ws = workspace(L.pt_iou_feat_ws_bytes(n, ch[0], ch[1], ch[2], H3, W3, ch[3], ch[4], ch[5], H4, W4), f3.device)
    rc = L.pt_iou_feat_f32(_ptr(f3), _ptr(f4), _ptr(pack), _ptr(c3), _ptr(c4), n, ch[0], ch[1], ch[2], H3, W3, ch[3], ch[4], ch[5],
                           H4, W4, _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_iou_feat_f32")
    return c3, c4
