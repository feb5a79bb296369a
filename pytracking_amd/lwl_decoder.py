"""LWL / RTS segmentation decoder (ltr/models/lwl/decoder.py:87-160, ltr/models/rts/decoder.py: the same code) on gfx950 (lwl_decoder.hip):

  forward(module, scores, features, image_size, output_layers=(), num_objects=None)
      LWTLDecoder.forward / RTSDecoder.forward of a reference decoder object                                      -> pt_lwl_decoder_f32

Every level (score resize, proj, TSE, RRB, CAB, RRB) and the Upsampler in one asynchronous call: 1x1 convolutions on the fp32 MFMA reading
NCHW, 3x3 convolutions on the banded tap-major correlation or the per-tap GEMM route with one epilogue kernel behind them, small kernels
for the means, the CAB gate, the resizes and the last one-channel convolution.  `covered(...)` says whether a call runs here;
install(decoder=True) hands every other call to the reference.  The weights are packed once per module state (tap-major 3x3 weights; bias
and eval BatchNorm as per-channel scale / shift folded in float64; layout in include/pt_hot.h) and cached outside the module (_packs.py:
the key, and when `refresh(module)` is needed).
"""
import ctypes
from collections import OrderedDict

import torch

from . import _lib, _packs
from .filter import _ptr, _stream, device_guarded, workspace

_PACKS = _packs.PackCache()
_OC = {"layer1": 1, "layer2": 2, "layer3": 2, "layer4": 4}                       # decoder.py:104
_ORDERS = (("layer4", "layer3", "layer2", "layer1"), ("layer3", "layer2", "layer1"))


def _conv_ok(conv, k, i, o, bias=True):
    return _packs.conv_ok(conv, k, 1, bias) and (conv.in_channels, conv.out_channels) == (i, o)


def _relu_ok(m):
    return (type(m) is torch.nn.LeakyReLU and m.negative_slope == 0.0) or type(m) is torch.nn.ReLU


def _seq(seq, kinds):
    """The modules of a Sequential whose members are, in order, of the given kinds ('c' convolution, 'r' ReLU, 'b' BatchNorm), else None."""
    if not isinstance(seq, torch.nn.Sequential) or len(seq) != len(kinds):
        return None
    for m, k in zip(seq, kinds):
        if (k == "r" and not _relu_ok(m)) or (k == "c" and type(m) is not torch.nn.Conv2d) or (k == "b" and type(m) is not torch.nn.BatchNorm2d):
            return None
    return list(seq)


def _rrb(m, oc):
    """[(conv1x1, None), (conv3x3, bn or None), (conv3x3 without bias, None)] of an RRB (decoder.py:57-69), else None."""
    if m is None or not hasattr(m, "conv1x1") or not hasattr(m, "bblock") or not _conv_ok(m.conv1x1, 1, oc, oc):
        return None
    b = _seq(m.bblock, "cbrc")
    bn = b[1] if b is not None else None
    if b is None:
        b = _seq(m.bblock, "crc")
    if b is None or not _conv_ok(b[0], 3, oc, oc) or not _conv_ok(b[-1], 3, oc, oc, bias=False) or (bn is not None and not _packs.bn_ok(bn, oc)):
        return None
    return [(m.conv1x1, None), (b[0], bn), (b[-1], None)]


def _structure(module):
    """None, or the decoder's description: dict(levels, fc, ic, mdim, use_bn, layers) with `layers` = [(Conv2d, BatchNorm2d or None)] in pack
    order (include/pt_hot.h) -- recognised by attributes and types, so LWTLDecoder and RTSDecoder are both accepted."""
    need = ("ft_channels", "TSE", "RRB1", "CAB", "RRB2", "proj", "project")
    if not isinstance(module, torch.nn.Module) or not all(hasattr(module, a) for a in need):
        return None
    if not all(isinstance(getattr(module, a), torch.nn.ModuleDict) for a in need[1:6]) or not hasattr(module.ft_channels, "items"):
        return None
    levels = tuple(module.ft_channels)
    up = module.project
    if levels not in _ORDERS or not all(hasattr(up, a) for a in ("conv1", "conv2")) or type(up.conv1) is not torch.nn.Conv2d:
        return None
    mdim = up.conv1.in_channels
    if mdim % 2 or not _conv_ok(up.conv1, 3, mdim, mdim // 2) or not _conv_ok(up.conv2, 3, mdim // 2, 1):
        return None
    layers, fcs, ic, use_bn, prev = [], [], None, None, None
    for k, L in enumerate(levels):
        oc = _OC[L] * mdim
        if any(L not in getattr(module, a) for a in need[1:5]) or (L in module.proj) != (k > 0):
            return None
        tse, cab = module.TSE[L], module.CAB[L]
        if not all(hasattr(tse, a) for a in ("reduce", "transform")) or not hasattr(cab, "convreluconv") or bool(getattr(cab, "deepest", None)) != (k == 0):
            return None
        red, tr, crc = _seq(tse.reduce, "crc"), _seq(tse.transform, "crcrcr"), _seq(cab.convreluconv, "crc")
        if red is None or tr is None or crc is None:
            return None
        fc = red[0].in_channels
        nc = tr[0].in_channels
        ic = nc - oc if ic is None else ic
        if nc - oc != ic or ic <= 0 or int(module.ft_channels[L]) != fc:
            return None
        if not (_conv_ok(red[0], 1, fc, oc) and _conv_ok(red[2], 1, oc, oc) and _conv_ok(tr[0], 3, nc, nc) and _conv_ok(tr[2], 3, nc, nc)
                and _conv_ok(tr[4], 3, nc, oc) and _conv_ok(crc[0], 1, 2 * oc, oc) and _conv_ok(crc[2], 1, oc, oc)):
            return None
        if k > 0:
            pj = _seq(module.proj[L], "cr")
            if pj is None or not _conv_ok(pj[0], 1, prev, oc):
                return None
            layers.append((pj[0], None))
        r1, r2 = _rrb(module.RRB1[L], oc), _rrb(module.RRB2[L], oc)
        if r1 is None or r2 is None:
            return None
        bns = [r1[1][1] is not None, r2[1][1] is not None]
        use_bn = bns[0] if use_bn is None else use_bn
        if bns != [use_bn, use_bn]:
            return None
        layers += [(red[0], None), (red[2], None), (tr[0], None), (tr[2], None), (tr[4], None)] + r1 + [(crc[0], None), (crc[2], None)] + r2
        fcs.append(fc)
        prev = oc
    layers += [(up.conv1, None), (up.conv2, None)]
    return dict(levels=levels, fc=tuple(fcs), ic=ic, mdim=mdim, use_bn=bool(use_bn), layers=layers)


def _ints(values):
    values = [int(v) for v in values]
    return (ctypes.c_int * len(values))(*values)


def _pack_floats(st):
    return _lib.lib().pt_lwl_decoder_pack_floats(len(st["levels"]), _ints(st["fc"]), st["ic"], st["mdim"], int(st["use_bn"]))


def pack_weights(module):
    """The pt_lwl_decoder_f32 pack of a decoder (float32, on its device; include/pt_hot.h)."""
    st = _structure(module)
    n = _pack_floats(st) if st is not None else 0
    if n == 0:
        raise NotImplementedError("decoder: the structure of LWTLDecoder with 3 or 4 levels, ic % 16 == 0, mdim % 32 == 0, fc % 16 == 0")
    parts = []
    last = st["layers"][-1][0]
    for conv, bn in st["layers"]:
        w = _packs.tap_major(conv).reshape(-1)                        # 1x1: (o, i); 3x3: tap-major (o, 9, i)
        if conv is last or conv.weight.shape[-1] == 1:                # then the bias
            parts += [w, conv.bias.detach().float().reshape(-1)]
        else:                                                         # then scale, shift
            parts += [w] + [v.float() for v in _packs.bn_fold(conv, bn)]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(module)


def packed_weights(module, st=None):
    st = _structure(module) if st is None else st
    if st is None:
        return pack_weights(module)                            # raises
    return _PACKS.get(module, _packs.layers_key(st["layers"]), pack_weights)


def _image_hw(image_size):
    return tuple(int(v) for v in image_size[-2:])


def _shapes(st, scores, features, image_size):
    """(n, hw list in level order, score hw, image hw) of a call, or None when the tensors do not fit the module."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 5 or scores.shape[2] != st["ic"] or scores.numel() == 0:
        return None
    n = scores.shape[0] * scores.shape[1]
    hw = []
    try:
        ihw = _image_hw(image_size)
        for L, fc in zip(st["levels"], st["fc"]):
            ft = features[L]
            if not isinstance(ft, torch.Tensor) or ft.dim() != 4 or ft.shape[0] != n or ft.shape[1] != fc or ft.numel() == 0:
                return None
            hw += [ft.shape[2], ft.shape[3]]
    except (KeyError, TypeError, IndexError, ValueError):
        return None
    if len(ihw) != 2:
        return None
    return n, hw, tuple(scores.shape[-2:]), ihw


def _ws_bytes(st, shp):
    n, hw, shw, ihw = shp
    return _lib.lib().pt_lwl_decoder_ws_bytes(n, len(st["levels"]), _ints(st["fc"]), _ints(hw), _ints(shw), _ints(ihw), st["ic"], st["mdim"])


def covered(module, scores, features, image_size, output_layers=(), num_objects=None) -> bool:
    st = _structure(module)
    if st is None or num_objects is not None:
        return False
    shp = _shapes(st, scores, features, image_size)
    if shp is None:
        return False
    acts = [scores] + [features[L] for L in st["levels"]]
    if not scores.is_cuda or not _packs.quiet(module, _packs.tensors(st["layers"]) + acts, scores):
        return False
    return _ws_bytes(st, shp) > 0


@device_guarded
def forward(module, scores, features, image_size, output_layers=(), num_objects=None, checked=False):
    """reference: LWTLDecoder.forward -> (mask (n, 1, H, W), OrderedDict of the '{L}_dec' maps named in `output_layers`)."""
    _packs.require_device(scores, *(features.values() if hasattr(features, "values") else []))
    if not checked and not covered(module, scores, features, image_size, output_layers, num_objects):
        raise NotImplementedError("decoder: eval mode, device fp32 5-D scores, one feature map per level with batch frames * sequences, no "
                                  "grad, num_objects=None, the structure of LWTLDecoder, ic % 16 == 0, mdim % 32 == 0, fc % 16 == 0, n <= 8")
    st = _structure(module)
    pack = packed_weights(module, st)
    n, hw, shw, ihw = _shapes(st, scores, features, image_size)
    levels = st["levels"]
    s = _packs.aligned(scores.reshape(n, *scores.shape[-3:]))
    feats = [_packs.aligned(features[L]) for L in levels]
    mask = torch.empty((n, 1) + ihw, dtype=torch.float32, device=s.device)
    outputs = OrderedDict()
    for k, L in enumerate(levels):
        if "{}_dec".format(L) in output_layers:
            outputs["{}_dec".format(L)] = torch.empty((n, _OC[L] * st["mdim"], hw[2 * k], hw[2 * k + 1]), dtype=torch.float32, device=s.device)
    vp = ctypes.c_void_p
    fptr = (vp * 4)(*[t.data_ptr() for t in feats])
    dptr = (vp * 4)(*[outputs["{}_dec".format(L)].data_ptr() if "{}_dec".format(L) in outputs else None for L in levels])
    lib = _lib.lib()
    ws = workspace(_ws_bytes(st, (n, hw, shw, ihw)), s.device)
    rc = lib.pt_lwl_decoder_f32(_ptr(s), fptr, _ptr(pack), _ptr(mask), dptr, n, len(levels), _ints(st["fc"]), _ints(hw), _ints(shw), _ints(ihw),
                                st["ic"], st["mdim"], _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_lwl_decoder_f32")
    return mask, outputs
