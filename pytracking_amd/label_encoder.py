"""Mask label encoder (ltr/models/lwl/label_encoder.py:9-55, ltr/models/rts/label_encoder.py:9-55) on gfx950 (label_enc.hip):

  forward(module, label_mask, feature=None)    ResidualDS16SW.forward of a reference ResidualDS16SW object       -> pt_label_enc_f32

Stem (conv 1 -> C0 stride 2, ReLU, max-pool) in one launch with the convolution output kept on chip, the two BasicBlocks and both heads on
the fp32 MFMA: six launches.  `covered(module, label_mask, feature)` says whether a call runs here; install(label_encoder=True) hands every
other call to the reference.  The weights are packed once per module state (tap-major weights; bias and eval BatchNorm, where the module
has one, as per-channel scale / shift folded in float64; layout in include/pt_hot.h) and cached outside the module (_packs.py: the key,
and when `refresh(module)` is needed).  The structure recogniser and the packer are shared with the score encoder (rts_fusion.py).
"""
import torch

from . import _lib
from ._packs import CPU_TENSOR, PackCache, aligned as _aligned, dev_f32 as _dev_f32, ds16_channels as _channels, ds16_layers, ds16_pack, layers_key, quiet as _quiet, tensors as _tensors
from .filter import _ptr, _stream, device_guarded, workspace

_PACKS = PackCache()


def _layers(module):
    """[(Conv2d, BatchNorm2d or None)] in pack order if `module` has exactly the structure of ResidualDS16SW, else None."""
    return ds16_layers(module, "ResidualDS16SW", 2)


def pack_weights(module):
    """The pt_label_enc_f32 pack of a ResidualDS16SW (float32, on its device; include/pt_hot.h)."""
    return ds16_pack(_layers(module), "pt_label_enc_pack_floats", "label encoder: the structure of ResidualDS16SW")


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(module)


def packed_weights(module, layers=None):
    layers = _layers(module) if layers is None else layers
    if layers is None:
        return pack_weights(module)                            # raises
    return _PACKS.get(module, layers_key(layers), pack_weights)


def covered(module, label_mask, feature=None) -> bool:
    layers = _layers(module)
    if layers is None or not isinstance(label_mask, torch.Tensor) or label_mask.dim() != 4:
        return False
    if not _dev_f32(label_mask) or label_mask.numel() == 0:
        return False
    if not _quiet(module, _tensors(layers) + [label_mask], label_mask):
        return False
    n = label_mask.shape[0] * label_mask.shape[1]
    return _lib.lib().pt_label_enc_ws_bytes(n, label_mask.shape[2], label_mask.shape[3], *_channels(layers)) > 0


@device_guarded
def forward(module, label_mask, feature=None, checked=False):
    """reference: ResidualDS16SW.forward -> (label_enc, sample_w), each (frames, seq, F, h, w)."""
    if isinstance(label_mask, torch.Tensor) and not label_mask.is_cuda:
        raise RuntimeError(CPU_TENSOR)
    if not checked and not covered(module, label_mask, feature):
        raise NotImplementedError("label encoder: eval mode, device fp32 4-D mask, no grad, the structure of ResidualDS16SW, layer dims "
                                  "multiples of 16 up to 64")
    layers = _layers(module)
    ch = _channels(layers)
    pack = packed_weights(module, layers)
    frames, seq, H, W = label_mask.shape
    n = frames * seq
    m = _aligned(label_mask)
    h, w = H, W
    for _ in range(4):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    enc = torch.empty((frames, seq, ch[3], h, w), dtype=torch.float32, device=m.device)
    sw = torch.empty((frames, seq, ch[3], h, w), dtype=torch.float32, device=m.device)
    L = _lib.lib()
    ws = workspace(L.pt_label_enc_ws_bytes(n, H, W, *ch), m.device)
    rc = L.pt_label_enc_f32(_ptr(m), _ptr(pack), _ptr(enc), _ptr(sw), n, H, W, *ch, _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_label_enc_f32")
    return enc, sw
