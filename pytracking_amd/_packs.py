"""What the fused modules share on the host: the weight-pack cache, the eval-BatchNorm fold, the structural checks of the reference's
convolution blocks, the call checks, and the recogniser / packer of the two DS16 encoders (label_encoder.py, rts_fusion.py).

The pack cache.  A fused module packs the weights of a reference `nn.Module` once per module STATE and keeps the pack outside the module
(a WeakKeyDictionary: not in `state_dict`, `deepcopy` or pickles; the entry goes with the module).  The state is `state_key(tensors,
*extras)`: every given parameter's and buffer's (data_ptr, _version, shape) plus whatever else the pack depends on (the BatchNorm eps
values, a config entry).  `load_state_dict`, `.to()` and in-place updates through ordinary ops all change it.  A write through `.data`
that keeps the storage bumps no version counter: after one, call the module's `refresh(module)`.  Every fused module owns one `PackCache`
(the same reference object may be served by two of them) and keeps `refresh` / `packed_weights` as its public face.
"""
import weakref

import torch

from . import _lib

CPU_TENSOR = "pytracking_amd ops run on the MI355X only (got a CPU tensor)"


class PackCache:
    """module -> (state key, pack), weakly keyed."""

    def __init__(self):
        self._packs = weakref.WeakKeyDictionary()

    def get(self, module, key, make):
        """The pack of `module` in state `key`; `make(module)` builds it when the cache has none for that state."""
        hit = self._packs.get(module)
        if hit is not None and hit[0] == key:
            return hit[1]
        pack = make(module)
        self._packs[module] = (key, pack)
        return pack

    def drop(self, module):
        self._packs.pop(module, None)

    def __contains__(self, module):
        return module in self._packs

    def __len__(self):
        return len(self._packs)


def state_key(tensors, *extras):
    return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors) + tuple(extras)


def layers_key(layers):
    """The state key of [(conv, BatchNorm or None)]."""
    return state_key(tensors(layers), *[bn.eps for _, bn in layers if bn is not None])


# ---------------------------------------------------------------------------------------------------------------------------
# the fold

def bn_fold(conv, bn=None):
    """float64 (scale, shift) with bn(conv(x)) = conv_without_bias(x) * scale + shift for an eval-mode BatchNorm behind `conv`
    (scale 1, shift = the bias without one)."""
    bias = (conv.bias.detach().double() if conv.bias is not None
            else torch.zeros(conv.out_channels, dtype=torch.float64, device=conv.weight.device))
    if bn is None:
        return torch.ones_like(bias), bias
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, (bias - bn.running_mean.detach().double()) * s + bn.bias.detach().double()


def bn_fold_weights(conv, bn=None):
    """float64 (W, b) with the scale multiplied into the weights: bn(conv(x)) = conv_W(x) + b; b is None for a bias-free convolution
    without BatchNorm."""
    w = conv.weight.detach().double()
    if bn is None:
        return w, (conv.bias.detach().double() if conv.bias is not None else None)
    s, shift = bn_fold(conv, bn)
    return w * s.reshape(-1, *[1] * (w.dim() - 1)), shift


def tap_major(conv):
    """(Cout, KH * KW * Cin) float32 view of a Conv2d weight, input channels innermost."""
    return conv.weight.detach().permute(0, 2, 3, 1).reshape(conv.out_channels, -1).float()


# ---------------------------------------------------------------------------------------------------------------------------
# structure

def one(v):
    return v[0] if isinstance(v, (tuple, list)) and len(v) == 2 and v[0] == v[1] else v


def conv_ok(conv, k, stride, bias):
    """An undilated, ungrouped, zero-padded k x k Conv2d of that stride with 'same' padding, with / without a bias."""
    return (type(conv) is torch.nn.Conv2d and (one(conv.kernel_size), one(conv.stride), one(conv.padding), one(conv.dilation))
            == (k, stride, k // 2, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and (conv.bias is not None) == bias)


def bn_ok(bn, channels):
    return (type(bn) is torch.nn.BatchNorm2d and bn.track_running_stats and bn.running_mean is not None and bn.running_var is not None
            and bn.affine and bn.num_features == channels)


def tensors(layers):
    """Every parameter and buffer of [(conv, BatchNorm or None)], in order."""
    out = []
    for conv, bn in layers:
        bias = conv.bias
        out += [conv.weight] if bias is None else [conv.weight, bias]
        if bn is not None:
            out += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# calls

def dev_f32(t, dim=None):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and (dim is None or t.dim() == dim)


def no_grad_needed(*ts):
    return not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts))


def quiet(module, ts, like):
    """Eval mode, everything fp32 on the device of `like`, nothing that asks for a gradient."""
    if module.training or any(m.training for m in module.modules()):
        return False
    if any(t.device != like.device or t.dtype != torch.float32 for t in ts):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in ts))


def require_device(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError(CPU_TENSOR)


def aligned(t):
    """`t` dense and on a 16-byte boundary (a copy only where it is not)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


# ---------------------------------------------------------------------------------------------------------------------------
# ResidualDS16SW (stride 2) / ResidualDS16SW_Clf (stride 1): one network at two strides

def _conv_block(seq, stride, relu):
    """(Conv2d, BatchNorm2d or None) of a `conv_block(...)` Sequential (ltr/models/layers/blocks.py:4-20), else None."""
    if not isinstance(seq, torch.nn.Sequential) or len(seq) < 1 or not conv_ok(seq[0], 3, stride, True):
        return None
    rest = list(seq)[1:]
    bn = rest.pop(0) if rest and isinstance(rest[0], torch.nn.BatchNorm2d) else None
    if bn is not None and not bn_ok(bn, seq[0].out_channels):
        return None
    if [type(m) for m in rest] != ([torch.nn.ReLU] if relu else []):
        return None
    return seq[0], bn


def _basic_block(blk, stride):
    """[(Conv2d, BatchNorm2d or None)] x 3 -- conv1, downsample, conv2 -- of a BasicBlock(stride, downsample = biased 3x3 conv of that
    stride) (ltr/models/backbone/resnet.py:15-53), else None."""
    need = ("conv1", "conv2", "downsample", "relu", "use_bn")
    if blk is None or type(blk).__name__ != "BasicBlock" or not all(hasattr(blk, a) for a in need):
        return None
    if not (conv_ok(blk.conv1, 3, stride, False) and conv_ok(blk.conv2, 3, 1, False) and conv_ok(blk.downsample, 3, stride, True)):
        return None
    if not isinstance(blk.relu, torch.nn.ReLU):
        return None
    c = blk.conv1.out_channels
    if (blk.conv2.in_channels, blk.conv2.out_channels, blk.downsample.in_channels, blk.downsample.out_channels) != (c, c, blk.conv1.in_channels, c):
        return None
    bn1, bn2 = (getattr(blk, "bn1", None), getattr(blk, "bn2", None)) if blk.use_bn else (None, None)
    if blk.use_bn and not (bn_ok(bn1, c) and bn_ok(bn2, c)):
        return None
    return [(blk.conv1, bn1), (blk.downsample, None), (blk.conv2, bn2)]


def ds16_channels(layers):
    """(C0, C1, C2, F)."""
    return (layers[0][0].out_channels, layers[1][0].out_channels, layers[4][0].out_channels, layers[7][0].out_channels)


def ds16_layers(module, cls_name, stride):
    """[(Conv2d, BatchNorm2d or None)] in pack order -- stem, res1.conv1, res1.downsample, res1.conv2, res2.conv1, res2.downsample,
    res2.conv2, label_pred, samp_w_pred -- if `module` has exactly the structure of the class of that name at that stride, else None."""
    if type(module).__name__ != cls_name or not all(hasattr(module, a) for a in ("conv_block", "pool", "res1", "res2", "label_pred",
                                                                                 "samp_w_pred")):
        return None
    pool = module.pool
    if type(pool) is not torch.nn.MaxPool2d or (one(pool.kernel_size), one(pool.stride), one(pool.padding), one(pool.dilation)) != (3, stride, 1, 1):
        return None
    if pool.ceil_mode or pool.return_indices:
        return None
    stem, head = _conv_block(module.conv_block, stride, True), _conv_block(module.label_pred, 1, True)
    b1, b2 = _basic_block(module.res1, stride), _basic_block(module.res2, stride)
    if stem is None or head is None or b1 is None or b2 is None or not conv_ok(module.samp_w_pred, 3, 1, True):
        return None
    out = [stem] + b1 + b2 + [head, (module.samp_w_pred, None)]
    c0, c1, c2, f = ds16_channels(out)
    chain = (stem[0].in_channels == 1 and b1[0][0].in_channels == c0 and b2[0][0].in_channels == c1 and head[0].in_channels == c2
             and module.samp_w_pred.in_channels == c2 and module.samp_w_pred.out_channels == f)
    return out if chain else None


def ds16_pack(layers, export, what):
    """The pack of either encoder (float32, on the module's device; include/pt_hot.h); the library's `export`(C0, C1, C2, F) is the size
    of it, 0 for dims it does not serve."""
    n = getattr(_lib.lib(), export)(*ds16_channels(layers)) if layers is not None else 0
    if n == 0:
        raise NotImplementedError(f"{what} with layer dims that are multiples of 16 up to 64")
    parts = []
    for group in ([0], [1, 2], [3], [4, 5], [6], [7, 8]):              # a block's conv1 | downsample and the two heads are one layer each
        s, b = zip(*[bn_fold(*layers[k]) for k in group])
        parts += [torch.cat([tap_major(layers[k][0]) for k in group]).reshape(-1), torch.cat(s).float(), torch.cat(b).float()]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack
