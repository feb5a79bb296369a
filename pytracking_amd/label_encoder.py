"""Mask label encoder (ltr/models/lwl/label_encoder.py:9-55, ltr/models/rts/label_encoder.py:9-55) on gfx950 (label_enc.hip):

  forward(module, label_mask, feature=None)    ResidualDS16SW.forward of a reference ResidualDS16SW object       -> pt_label_enc_f32

Stem (conv 1 -> C0 stride 2, ReLU, max-pool) in one launch with the convolution output kept on chip, the two BasicBlocks and both heads on
the fp32 MFMA: six launches.  `covered(module, label_mask, feature)` says whether a call runs here; install(label_encoder=True) hands every
other call to the reference.  The weights are packed once per module state (tap-major weights; bias and eval BatchNorm, where the module
has one, as per-channel scale / shift folded in float64; layout in include/pt_hot.h) and cached outside the module like the IoU towers':
the key is every parameter's and buffer's (data_ptr, _version, shape) plus the BatchNorm eps values, so `load_state_dict` and in-place
updates are picked up; after a write through `.data` call `refresh(module)`.
"""
import weakref

import torch

from . import _lib
from .filter import _ptr, _stream, device_guarded, workspace

_PACKS = weakref.WeakKeyDictionary()


def _one(v):
    return v[0] if isinstance(v, (tuple, list)) and len(v) == 2 and v[0] == v[1] else v


def _conv_ok(conv, stride, bias):
    return (type(conv) is torch.nn.Conv2d and (_one(conv.kernel_size), _one(conv.stride), _one(conv.padding), _one(conv.dilation))
            == (3, stride, 1, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and (conv.bias is not None) == bias)


def _bn_ok(bn, channels):
    return (type(bn) is torch.nn.BatchNorm2d and bn.track_running_stats and bn.running_mean is not None and bn.running_var is not None
            and bn.affine and bn.num_features == channels)


def _conv_block(seq, stride, relu):
    """(Conv2d, BatchNorm2d or None) of a `conv_block(...)` Sequential (ltr/models/layers/blocks.py:4-20), else None."""
    if not isinstance(seq, torch.nn.Sequential) or len(seq) < 1 or not _conv_ok(seq[0], stride, True):
        return None
    rest = list(seq)[1:]
    bn = rest.pop(0) if rest and isinstance(rest[0], torch.nn.BatchNorm2d) else None
    if bn is not None and not _bn_ok(bn, seq[0].out_channels):
        return None
    if [type(m) for m in rest] != ([torch.nn.ReLU] if relu else []):
        return None
    return seq[0], bn


def _basic_block(blk):
    """[(Conv2d, BatchNorm2d or None)] x 3 -- conv1, downsample, conv2 -- of a BasicBlock(stride 2, downsample = biased 3x3 stride-2 conv)
    (ltr/models/backbone/resnet.py:15-53), else None."""
    need = ("conv1", "conv2", "downsample", "relu", "use_bn")
    if blk is None or type(blk).__name__ != "BasicBlock" or not all(hasattr(blk, a) for a in need):
        return None
    if not (_conv_ok(blk.conv1, 2, False) and _conv_ok(blk.conv2, 1, False) and _conv_ok(blk.downsample, 2, True)):
        return None
    if not isinstance(blk.relu, torch.nn.ReLU):
        return None
    c = blk.conv1.out_channels
    if (blk.conv2.in_channels, blk.conv2.out_channels, blk.downsample.in_channels, blk.downsample.out_channels) != (c, c, blk.conv1.in_channels, c):
        return None
    bn1, bn2 = (getattr(blk, "bn1", None), getattr(blk, "bn2", None)) if blk.use_bn else (None, None)
    if blk.use_bn and not (_bn_ok(bn1, c) and _bn_ok(bn2, c)):
        return None
    return [(blk.conv1, bn1), (blk.downsample, None), (blk.conv2, bn2)]


def _layers(module):
    """[(Conv2d, BatchNorm2d or None)] in pack order -- stem, res1.conv1, res1.downsample, res1.conv2, res2.conv1, res2.downsample,
    res2.conv2, label_pred, samp_w_pred -- if `module` has exactly the structure of ResidualDS16SW, else None."""
    if type(module).__name__ != "ResidualDS16SW" or not all(hasattr(module, a) for a in ("conv_block", "pool", "res1", "res2", "label_pred",
                                                                                         "samp_w_pred")):
        return None
    pool = module.pool
    if type(pool) is not torch.nn.MaxPool2d or (_one(pool.kernel_size), _one(pool.stride), _one(pool.padding), _one(pool.dilation)) != (3, 2, 1, 1):
        return None
    if pool.ceil_mode or pool.return_indices:
        return None
    stem, head = _conv_block(module.conv_block, 2, True), _conv_block(module.label_pred, 1, True)
    b1, b2 = _basic_block(module.res1), _basic_block(module.res2)
    if stem is None or head is None or b1 is None or b2 is None or not _conv_ok(module.samp_w_pred, 1, True):
        return None
    out = [stem] + b1 + b2 + [head, (module.samp_w_pred, None)]
    c0, c1, c2, f = _channels(out)
    chain = (stem[0].in_channels == 1 and b1[0][0].in_channels == c0 and b2[0][0].in_channels == c1 and head[0].in_channels == c2
             and module.samp_w_pred.in_channels == c2 and module.samp_w_pred.out_channels == f)
    return out if chain else None


def _channels(layers):
    return (layers[0][0].out_channels, layers[1][0].out_channels, layers[4][0].out_channels, layers[7][0].out_channels)


def _tensors(layers):
    out = []
    for conv, bn in layers:
        out += [conv.weight] + ([conv.bias] if conv.bias is not None else [])
        if bn is not None:
            out += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    return out


def _folded(conv, bn):
    """(tap-major weight, scale, shift) of one convolution, float32; the fold is done in float64."""
    o = conv.out_channels
    bias = conv.bias.detach().double() if conv.bias is not None else torch.zeros(o, dtype=torch.float64, device=conv.weight.device)
    if bn is None:
        s, shift = torch.ones_like(bias), bias
    else:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shift = (bias - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return conv.weight.detach().permute(0, 2, 3, 1).reshape(o, -1).float(), s.float(), shift.float()


def pack_weights(module):
    """The pt_label_enc_f32 pack of a ResidualDS16SW (float32, on its device; include/pt_hot.h)."""
    layers = _layers(module)
    n = _lib.lib().pt_label_enc_pack_floats(*_channels(layers)) if layers is not None else 0
    if n == 0:
        raise NotImplementedError("label encoder: the structure of ResidualDS16SW with layer dims that are multiples of 16 up to 64")
    parts = []
    for group in ([0], [1, 2], [3], [4, 5], [6], [7, 8]):              # a block's conv1 | downsample and the two heads are one layer each
        w, s, b = zip(*[_folded(*layers[k]) for k in group])
        parts += [torch.cat(w).reshape(-1), torch.cat(s), torch.cat(b)]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def _state_key(layers):
    return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in _tensors(layers)) + tuple(bn.eps for _, bn in layers if bn is not None)


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.pop(module, None)


def packed_weights(module, layers=None):
    layers = _layers(module) if layers is None else layers
    if layers is None:
        return pack_weights(module)                            # raises
    key = _state_key(layers)
    hit = _PACKS.get(module)
    if hit is not None and hit[0] == key:
        return hit[1]
    pack = pack_weights(module)
    _PACKS[module] = (key, pack)
    return pack


def covered(module, label_mask, feature=None) -> bool:
    layers = _layers(module)
    if layers is None or not isinstance(label_mask, torch.Tensor) or label_mask.dim() != 4:
        return False
    if module.training or any(m.training for m in module.modules()):
        return False
    if not (label_mask.is_cuda and label_mask.dtype == torch.float32) or label_mask.numel() == 0:
        return False
    tens = _tensors(layers)
    if any(t.device != label_mask.device or t.dtype != torch.float32 for t in tens):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in tens + [label_mask]):
        return False
    n = label_mask.shape[0] * label_mask.shape[1]
    return _lib.lib().pt_label_enc_ws_bytes(n, label_mask.shape[2], label_mask.shape[3], *_channels(layers)) > 0


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


@device_guarded
def forward(module, label_mask, feature=None, checked=False):
    """reference: ResidualDS16SW.forward -> (label_enc, sample_w), each (frames, seq, F, h, w)."""
    if isinstance(label_mask, torch.Tensor) and not label_mask.is_cuda:
        raise RuntimeError("pytracking_amd ops run on the MI355X only (got a CPU tensor)")
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
