"""TEST INFRASTRUCTURE ONLY -- the ResNet backbone forward (include/pt_bbn.h) restated from its structure, in float64 or fp32 on the CPU,
and a stand-in `nn.Module` with the reference's attribute names so that the GPU tests run without the reference tree.

A network is a `spec`: kind ('Bottleneck' / 'BasicBlock'), blocks (4), inplanes, mrcnn (the stride of a layer's first bottleneck on its
first 1x1, a downsample wherever the channel count changes, `conv1` tapped behind the pool, no `fc`).  `keys(spec)` lists every
`state_dict` entry of the reference class with its shape and role; `restate(spec, params, x, outputs, dtype, defect)` is the forward.

Seeded defects (`defect=`), each of which must miss the float64 bound of at least one case (tests/test_backbone_cpu.py): see DEFECTS."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

OUTPUTS = ("conv1", "layer1", "layer2", "layer3", "layer4")
EPS = 1e-5
DEFECTS = ("no_eps", "stride_on_other_conv", "residual_after_relu", "no_final_relu", "conv1_wrong_side", "downsample_stride_ignored", "stem_pad2")


def expansion(spec):
    return 4 if spec["kind"] == "Bottleneck" else 1


def layer_stride(spec, L):
    return 1 if L == 1 else 2


def block_convs(spec, L, b, cin):
    """[(name, k, cin, cout, stride)] of block b of layer L (1-based) in module order, then the downsample or None."""
    planes, s = spec["inplanes"] << (L - 1), (layer_stride(spec, L) if b == 0 else 1)
    cout = planes * expansion(spec)
    if spec["kind"] == "Bottleneck":
        s1, s2 = (s, 1) if spec["mrcnn"] else (1, s)
        convs = [("conv1", 1, cin, planes, s1), ("conv2", 3, planes, planes, s2), ("conv3", 1, planes, cout, 1)]
    else:
        convs = [("conv1", 3, cin, planes, s), ("conv2", 3, planes, planes, 1)]
    has_ds = b == 0 and (cin != cout or (s != 1 and not spec["mrcnn"]))
    return convs, (("downsample.0", 1, cin, cout, s) if has_ds else None), cout


def keys(spec, num_classes=1000):
    """[(state_dict key, shape, role)] in the reference's order; role: ('conv', k, cout) | 'gamma' | 'gamma_last' | 'beta' | 'mean' | 'var' |
    'count' | 'fc_w' | 'fc_b'."""
    out = []

    def bn(prefix, c, last=False):
        out.extend([(prefix + ".weight", (c,), "gamma_last" if last else "gamma"), (prefix + ".bias", (c,), "beta"),
                    (prefix + ".running_mean", (c,), "mean"), (prefix + ".running_var", (c,), "var"), (prefix + ".num_batches_tracked", (), "count")])

    c0 = spec["inplanes"]
    out.append(("conv1.weight", (c0, 3, 7, 7), ("conv", 7, c0)))
    bn("bn1", c0)
    cin = c0
    for L in range(1, 5):
        for b in range(spec["blocks"][L - 1]):
            convs, ds, cout = block_convs(spec, L, b, cin)
            p = f"layer{L}.{b}."
            for i, (name, k, ci, co, _) in enumerate(convs):
                out.append((p + name + ".weight", (co, ci, k, k), ("conv", k, co)))
                bn(p + "bn" + name[-1], co, last=i == len(convs) - 1)
            if ds is not None:
                out.append((p + "downsample.0.weight", (cout, cin, 1, 1), ("conv", 1, cout)))
                bn(p + "downsample.1", cout)
            cin = cout
    if not spec["mrcnn"]:
        out += [("fc.weight", (num_classes, c0 * 8 * expansion(spec)), "fc_w"), ("fc.bias", (num_classes,), "fc_b")]
    return out


def restate(spec, params, x, outputs, dtype=np.float64, defect=None):
    """OrderedDict {layer: (n, C, h, w) tensor of `dtype`} of the requested layers, stopping behind the deepest one."""
    assert defect is None or defect in DEFECTS, defect
    td = torch.float64 if dtype == np.float64 else torch.float32
    P = {k: torch.as_tensor(np.asarray(v)).to(td) for k, v in params.items() if not k.endswith("num_batches_tracked")}
    x = torch.as_tensor(np.asarray(x)).to(td)
    eps = 0.0 if defect == "no_eps" else EPS

    def bn(t, p):
        s = P[p + ".weight"] / torch.sqrt(P[p + ".running_var"] + eps)
        return (t - P[p + ".running_mean"][None, :, None, None]) * s[None, :, None, None] + P[p + ".bias"][None, :, None, None]

    def conv(t, name, k, stride, pad=None):
        return F.conv2d(t, P[name + ".weight"], stride=stride, padding=k // 2 if pad is None else pad)

    outs, deepest = OrderedDict(), max(OUTPUTS.index(o) for o in outputs)
    after_pool = spec["mrcnn"] != (defect == "conv1_wrong_side")
    t = torch.relu(bn(conv(x, "conv1", 7, 2, pad=2 if defect == "stem_pad2" else 3), "bn1"))
    if "conv1" in outputs and not after_pool:
        outs["conv1"] = t
    if deepest == 0 and not after_pool:
        return outs
    t = F.max_pool2d(t, 3, 2, 1)
    if "conv1" in outputs and after_pool:
        outs["conv1"] = t
    cin = spec["inplanes"]
    for L in range(1, deepest + 1):
        for b in range(spec["blocks"][L - 1]):
            convs, ds, cout = block_convs(spec, L, b, cin)
            p = f"layer{L}.{b}."
            if defect == "stride_on_other_conv" and spec["kind"] == "Bottleneck":
                (n1, k1, a1, b1, s1), (n2, k2, a2, b2, s2) = convs[0], convs[1]
                convs = [(n1, k1, a1, b1, s2), (n2, k2, a2, b2, s1), convs[2]]
            u = t
            for i, (name, k, _, _, s) in enumerate(convs):
                u = bn(conv(u, p + name, k, s), p + "bn" + name[-1])
                if i < len(convs) - 1:
                    u = torch.relu(u)
            res = t
            if ds is not None:
                res = conv(t, p + "downsample.0", 1, 1 if defect == "downsample_stride_ignored" else ds[4])
                if defect == "downsample_stride_ignored":
                    res = res[:, :, :u.shape[2], :u.shape[3]]
                res = bn(res, p + "downsample.1")
            if defect == "residual_after_relu":
                t = torch.relu(u) + res
            elif defect == "no_final_relu":
                t = u + res
            else:
                t = torch.relu(u + res)
            cin = cout
        if OUTPUTS[L] in outputs:
            outs[OUTPUTS[L]] = t
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------
# the stand-in module: the reference's attribute names and class names, no forward of its own
# ---------------------------------------------------------------------------------------------------------------------------------
class BasicBlock(torch.nn.Module):
    def __init__(self, convs, ds):
        super().__init__()
        self.use_bn = True
        _fill(self, convs, ds)


class Bottleneck(torch.nn.Module):
    def __init__(self, convs, ds):
        super().__init__()
        _fill(self, convs, ds)


def _fill(blk, convs, ds):
    for i, (name, k, ci, co, s) in enumerate(convs):
        setattr(blk, name, torch.nn.Conv2d(ci, co, k, stride=s, padding=k // 2, bias=False))
        setattr(blk, "bn" + name[-1], torch.nn.BatchNorm2d(co))
        if i == 0:
            blk.relu = torch.nn.ReLU(inplace=True)
    blk.downsample = None if ds is None else torch.nn.Sequential(torch.nn.Conv2d(ds[2], ds[3], 1, stride=ds[4], bias=False),
                                                                 torch.nn.BatchNorm2d(ds[3]))


class ResNet(torch.nn.Module):
    """Stand-in for ltr.models.backbone.resnet.ResNet / resnet_mrcnn.ResNet: same attributes, same `state_dict` keys."""

    def __init__(self, spec, output_layers):
        super().__init__()
        c0 = spec["inplanes"]
        self.output_layers = list(output_layers)
        self.conv1_after_pool = bool(spec["mrcnn"])                 # what the reference class's module says (pytracking_amd/backbone.py)
        self.conv1 = torch.nn.Conv2d(3, c0, 7, stride=2, padding=3, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(c0)
        self.relu = torch.nn.ReLU(inplace=True)
        self.maxpool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        cls, cin = (Bottleneck if spec["kind"] == "Bottleneck" else BasicBlock), c0
        for L in range(1, 5):
            blocks = []
            for b in range(spec["blocks"][L - 1]):
                convs, ds, cin_next = block_convs(spec, L, b, cin)
                blocks.append(cls(convs, ds))
                cin = cin_next
            setattr(self, f"layer{L}", torch.nn.Sequential(*blocks))
        if not spec["mrcnn"]:
            self.avgpool = torch.nn.AdaptiveAvgPool2d((1, 1))
            self.fc = torch.nn.Linear(c0 * 8 * expansion(spec), 1000)

    def forward(self, x, output_layers=None):
        raise RuntimeError("the stand-in has no forward: pytracking_amd.backbone.forward(module, x) is the subject")


def standin(spec, params, output_layers, device="cpu"):
    """The stand-in with `params` loaded strictly, in eval mode."""
    m = ResNet(spec, output_layers)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in params.items()}, strict=True)
    return m.to(device).eval()
