"""ResNet backbone forward (ltr/models/backbone/resnet.py:175-221, ltr/models/backbone/resnet_mrcnn.py:140-186) on gfx950
(include/pt_bbn.h, csrc_bbn/backbone.hip):

  forward(module, x, output_layers=None)    ResNet.forward of a reference ResNet object (either file)             -> pt_bbn_forward_f32

The 7x7 stem, the max-pool and every residual block up to the deepest requested layer as implicit GEMMs over tokens on the fp32 MFMA, each
eval BatchNorm folded in float64 into the (scale, shift) of its convolution's epilogue (`_packs.bn_fold`), the residual add and the ReLU in
that epilogue too.  Returns what the reference returns: an OrderedDict of the requested layers in network order; nothing behind the deepest
requested layer is computed.  `describe(module)` reads the network off the module's own attributes (`conv1`, `bn1`, `maxpool`,
`layer1..4`, per block `conv1..3`, `bn1..3`, `downsample`, every convolution's stride / padding / dilation): the two differences between
the files -- which convolution of a layer's first block carries the stride, and on which side of the pool `conv1` is tapped (the class's
module name says it) -- are two fields of the `pt_bbn_desc`, not a second path.  `covered(module, x, output_layers)` says whether a call
runs here; install(backbone=True) hands every other call to the reference.  The weights are packed once per module state and cached outside
the module (_packs.py: the key, and when `refresh(module)` is needed); the workspace is held per (device, stream).

Not covered, still the reference's: training mode, gradients, CPU / non-fp32 / non-contiguous input, dilated networks
(`dilation_factor != 1`), `BasicBlock(use_bn=False)`, the `fc` / 'default' outputs, `preprocess_image`, `resnet18_vggm`, the Swin backbones.
"""
import collections
import ctypes
import weakref

import torch

from . import _lib_bbn as _L
from ._packs import CPU_TENSOR, PackCache, bn_fold, bn_ok, layers_key, one, tap_major, tensors as _tensors
from .filter import device_guarded

OUTPUTS = _L.OUTPUTS
_PACKS = PackCache()
MRCNN_MODULE = "ltr.models.backbone.resnet_mrcnn"              # the class of this module taps `conv1` behind the pool

Net = collections.namedtuple("Net", "desc layers")             # pt_bbn_desc, [(Conv2d, BatchNorm2d)] in pack order


def _conv(conv, k, cin, cout):
    """The stride of a bias-free, undilated, ungrouped k x k Conv2d cin -> cout with padding k // 2, else None."""
    if type(conv) is not torch.nn.Conv2d or conv.bias is not None or conv.groups != 1 or conv.padding_mode != "zeros":
        return None
    if (one(conv.kernel_size), one(conv.padding), one(conv.dilation)) != (k, k // 2, 1) or (conv.in_channels, conv.out_channels) != (cin, cout):
        return None
    s = one(conv.stride)
    return s if s in (1, 2) else None


def _block(blk, kind, cin, planes):
    """(convolutions [(Conv2d, BatchNorm2d)] in pack order, stride, which convolution carries it) of one residual block, else None."""
    bottleneck = kind == "Bottleneck"
    names = ("conv1", "conv2", "conv3") if bottleneck else ("conv1", "conv2")
    if type(blk).__name__ != kind or not all(hasattr(blk, a) for a in names + ("relu", "downsample")):
        return None
    if not isinstance(blk.relu, torch.nn.ReLU) or (not bottleneck and not getattr(blk, "use_bn", False)):
        return None
    shapes = ((1, cin, planes), (3, planes, planes), (1, planes, 4 * planes)) if bottleneck else ((3, cin, planes), (3, planes, planes))
    cout, convs, strides = shapes[-1][2], [], []
    for name, (k, ci, co) in zip(names, shapes):
        conv, bn = getattr(blk, name), getattr(blk, "bn" + name[-1], None)
        s = _conv(conv, k, ci, co)
        if s is None or not bn_ok(bn, co):
            return None
        convs.append((conv, bn))
        strides.append(s)
    if strides[-1] != 1 or sum(s == 2 for s in strides) > 1:
        return None
    stride, which = (2, strides.index(2) + 1) if 2 in strides else (1, 0)
    ds = blk.downsample
    if (ds is not None) != (stride != 1 or cin != cout):
        return None
    if ds is not None:
        if type(ds) is not torch.nn.Sequential or len(ds) != 2 or _conv(ds[0], 1, cin, cout) != stride or not bn_ok(ds[1], cout):
            return None
        convs.append((ds[0], ds[1]))
    return convs, stride, which


def describe(module):
    """Net of a reference ResNet the kernels cover, else None."""
    if type(module).__name__ != "ResNet" or not all(hasattr(module, a) for a in ("conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3",
                                                                                  "layer4", "output_layers")):
        return None
    c0, pool = getattr(module.conv1, "out_channels", 0), module.maxpool
    if _conv(module.conv1, 7, 3, c0) != 2 or not bn_ok(module.bn1, c0) or not isinstance(module.relu, torch.nn.ReLU):
        return None
    if type(pool) is not torch.nn.MaxPool2d or (one(pool.kernel_size), one(pool.stride), one(pool.padding), one(pool.dilation)) != (3, 2, 1, 1):
        return None
    if pool.ceil_mode or pool.return_indices or c0 % 8 or not 8 <= c0 <= _L.PT_BBN_MAX_INPLANES:
        return None
    stages = [getattr(module, f"layer{i}") for i in range(1, 5)]
    if not all(type(s) is torch.nn.Sequential and 1 <= len(s) <= _L.PT_BBN_MAX_BLOCKS for s in stages):
        return None
    kind = type(stages[0][0]).__name__
    if kind not in ("BasicBlock", "Bottleneck"):
        return None
    exp = 4 if kind == "Bottleneck" else 1
    layers, strides, carriers, cin = [(module.conv1, module.bn1)], [], set(), c0
    for i, stage in enumerate(stages):
        for b, blk in enumerate(stage):
            got = _block(blk, kind, cin, c0 << i)
            if got is None or (b > 0 and got[1] != 1):
                return None
            if b == 0:
                strides.append(got[1])
                carriers.add(got[2])
            layers += got[0]
            cin = (c0 << i) * exp
    carriers.discard(0)
    if len(carriers) > 1 or (kind == "BasicBlock" and carriers - {1}):
        return None
    desc = _L.BbnDesc()
    desc.block = _L.PT_BBN_BOTTLENECK if kind == "Bottleneck" else _L.PT_BBN_BASIC
    desc.inplanes = c0
    desc.blocks[:], desc.stride[:] = [len(s) for s in stages], strides
    desc.stride_conv = carriers.pop() if carriers else (2 if kind == "Bottleneck" else 1)
    desc.conv1_after_pool = int(type(module).__module__ == MRCNN_MODULE or bool(getattr(module, "conv1_after_pool", False)))
    return Net(desc, layers)


_NETS = weakref.WeakKeyDictionary()


def _net(module):
    """describe(module), remembered per module for as long as its module tree -- the identity of every submodule -- stays what it was
    (describe walks 53 blocks of a ResNet-50: as long as the kernels take).  A convolution's stride or a block's `use_bn` rewritten in place
    is not seen: call `refresh(module)` after one."""
    key = tuple(map(id, module.modules()))
    hit = _NETS.get(module)
    if hit is None or hit[0] != key:
        hit = _NETS[module] = (key, describe(module))
    return hit[1]


def pack_weights(module, net=None):
    """The pt_bbn_forward_f32 pack of a ResNet (float32, on its device; layout in include/pt_bbn.h)."""
    net = describe(module) if net is None else net
    if net is None:
        raise NotImplementedError("backbone: the structure of ltr's ResNet (BasicBlock / Bottleneck, dilation 1, BatchNorm everywhere)")
    parts = []
    for i, (conv, bn) in enumerate(net.layers):
        if i == 0:                                                 # the stem: (Cout, c * 49 + ky * 7 + kx), zero behind 147
            w = torch.zeros(conv.out_channels, _L.PT_BBN_STEM_K, dtype=torch.float32, device=conv.weight.device)
            w[:, :147] = conv.weight.detach().reshape(conv.out_channels, 147).float()
        else:
            w = tap_major(conv)
        s, b = bn_fold(conv, bn)
        parts += [w.reshape(-1), s.float(), b.float()]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == _L.lib().pt_bbn_pack_floats(ctypes.byref(net.desc)), pack.numel()
    return pack


def refresh(module):
    """Drop the packed weights and the remembered structure of `module` (needed only after a write through `.data`, which bumps no
    version counter, or an in-place change of a submodule's own attributes)."""
    _PACKS.drop(module)
    _NETS.pop(module, None)


def packed_weights(module, net=None):
    net = _net(module) if net is None else net
    if net is None:
        return pack_weights(module)                                # raises
    return _PACKS.get(module, layers_key(net.layers), lambda m: pack_weights(m, net))


def _mask(module, output_layers):
    """The out_mask of a request (None: the module's own list), 0 for one the kernels do not serve (`fc`, 'default', unknown names, an
    empty list, a repeated name: the reference compares list lengths)."""
    names = module.output_layers if output_layers is None else output_layers
    if not isinstance(names, (list, tuple)) or not names or len(set(names)) != len(names) or any(n not in OUTPUTS for n in names):
        return 0
    return sum(1 << OUTPUTS.index(n) for n in names)


def why_not(module, x, output_layers=None):
    """None for a call that runs here, else the reason it does not: the module's side first (structure, mode, request), then the input."""
    net = _net(module)
    if net is None:
        return "structure outside ltr's ResNet at dilation 1 with BatchNorm everywhere"
    mask = _mask(module, output_layers)
    if not mask:
        return "outputs outside conv1 / layer1..4"
    if module.training or any(m.training for m in module.modules()):
        return "training mode"
    if torch.is_grad_enabled():
        return "gradients enabled"
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        return "input that is not (n, 3, H, W)"
    if not x.is_cuda:
        return "CPU input"
    if x.dtype != torch.float32 or not x.is_contiguous():
        return "input that is not contiguous fp32"
    if any(t.device != x.device or t.dtype != torch.float32 for t in _tensors(net.layers)):
        return "parameters on another device or not fp32"
    if _L.lib().pt_bbn_ws_bytes(ctypes.byref(net.desc), x.shape[0], x.shape[2], x.shape[3], mask) == 0:
        return "sizes outside include/pt_bbn.h"
    return None


def covered(module, x, output_layers=None) -> bool:
    return why_not(module, x, output_layers) is None


_WORKSPACES = {}


def _workspace(nbytes, device):
    """The (device, stream)'s workspace, grown when a call needs more -> its 256-byte aligned address."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes + 256:
        ws = _WORKSPACES[key] = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return (ws.data_ptr() + 255) // 256 * 256


def plan(module, x_shape, output_layers=None):
    """[pt_bbn_launch] of the call (host only)."""
    net = _net(module)
    mask = _mask(module, output_layers) if net is not None else 0
    if not mask:
        raise NotImplementedError("backbone: request outside include/pt_bbn.h")
    rows = (_L.BbnLaunch * _L.PT_BBN_MAX_LAUNCHES)()
    n = _L.lib().pt_bbn_plan(ctypes.byref(net.desc), x_shape[0], x_shape[2], x_shape[3], mask, rows)
    _L.check(min(n, 0), "pt_bbn_plan")
    return list(rows[:n])


@device_guarded
def forward(module, x, output_layers=None, checked=False):
    """reference: ResNet.forward -> OrderedDict {layer name: (n, C, h, w)} of the requested layers, in network order."""
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        raise RuntimeError(CPU_TENSOR)
    if not checked and not covered(module, x, output_layers):
        raise NotImplementedError("backbone: eval mode, no grad, contiguous device fp32 (n, 3, H, W) input, the structure of ltr's ResNet at "
                                  "dilation 1, outputs among conv1 / layer1..4, sizes within include/pt_bbn.h")
    net = _net(module)
    mask = _mask(module, output_layers)
    pack = packed_weights(module, net)
    n, _, H, W = x.shape
    lib, desc = _L.lib(), ctypes.byref(net.desc)
    rows = (_L.BbnLaunch * _L.PT_BBN_MAX_LAUNCHES)()
    count = lib.pt_bbn_plan(desc, n, H, W, mask, rows)
    _L.check(min(count, 0), "pt_bbn_plan")
    outs, ptrs = collections.OrderedDict(), (ctypes.c_void_p * _L.PT_BBN_OUT_COUNT)()
    for r in sorted((r for r in rows[:count] if r.out >= 0), key=lambda r: r.out):     # the launches that write an NCHW output
        outs[OUTPUTS[r.out]] = t = torch.empty((n, r.N, r.Hout, r.Wout), dtype=torch.float32, device=x.device)
        ptrs[r.out] = t.data_ptr()
    nbytes = lib.pt_bbn_ws_bytes(desc, n, H, W, mask)
    rc = lib.pt_bbn_forward_f32(desc, pack.data_ptr(), x.data_ptr(), n, H, W, mask, ptrs, _workspace(nbytes, x.device), nbytes,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _L.check(rc, "pt_bbn_forward_f32")
    return outs
