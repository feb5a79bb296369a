"""TEST INFRASTRUCTURE ONLY -- the case table of the ResNet backbone forward (include/pt_bbn.h): the smallest shapes at which the kernels can
still go wrong, one case per (kernel, tile, K-split) route the plan can pick, and the deployed shapes.

A case is a network spec (tests/backbone_np.py), an input shape, the requested outputs and a seed.  The parameters do not fit a fixture
(ResNet-50 to layer3 is 34 MB), so `params(case)` draws every `state_dict` entry from a seeded numpy generator: convolutions He-normal as
the constructor draws them (std sqrt(2 / (k k Cout))), BatchNorm gamma from U(0.5, 1.5) except the last BatchNorm of every block, U(0.1,
0.4) (with the constructor's gamma = 1 the activations reach 1.5e2 at layer3 of ResNet-50 and 9e4 in ResNet-101), beta and running mean
from N(0, 0.1^2), running variance from U(0.5, 1.5).

tools/make_golden_backbone.py writes what the UNMODIFIED reference classes made of a case on the CPU: tests/golden/backbone_<case>.npz, or,
where that would pass 1 MB, one file per output, backbone_<case>__<layer>.npz.  Per output <o>:
    <o>_f64, <o>_f32   the float64 run and the fp32 run (8 threads), flat, at `subset(case, o, numel)`: the whole map up to 65 536
                       elements, else 65 536 fixed pseudo-random flat positions
    <o>_shape          the map's shape
    <o>_ref_err        max |fp32 - float64| over the whole map          <o>_max   max |float64| over the whole map
    <o>_sum, <o>_abssum   sum and absolute sum of the whole float64 map
numpy only at import."""
import glob
import os
from collections import OrderedDict

import numpy as np

import backbone_np as RN

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUBSET = 65536
ALL = list(RN.OUTPUTS)


def net(kind, blocks, inplanes, mrcnn=False):
    return dict(kind=kind, blocks=list(blocks), inplanes=inplanes, mrcnn=mrcnn)


def case(spec, shape, outputs, seed, deployed=False):
    return dict(spec=spec, shape=tuple(shape), outputs=list(outputs), seed=seed, deployed=deployed)


BOTT1 = [1, 1, 1, 1]
CASES = OrderedDict([
    ("bott_tiny", case(net("Bottleneck", BOTT1, 16), (1, 3, 32, 32), ALL, 1)),
    # maps 17x24, 9x12, 5x6, 3x3, 2x2: every level odd, stride-2 sizes (x - 1) / 2 + 1, tiles that cross the image boundary
    ("bott_odd_n2", case(net("Bottleneck", [1, 2, 1, 1], 16), (2, 3, 33, 47), ALL, 2)),
    # layer4 is a 1x1 map: the 3x3 convolution of its second block sees nothing but halo
    ("bott_n5_to_1x1", case(net("Bottleneck", [1, 1, 1, 2], 16), (5, 3, 19, 21), ALL, 3)),
    # Cin and Cout no multiples of 32 or 64: the K tail and the N tail
    ("bott_c24", case(net("Bottleneck", BOTT1, 24), (1, 3, 32, 40), ALL, 4)),
    ("bott_c8", case(net("Bottleneck", BOTT1, 8), (2, 3, 32, 32), ALL, 5)),
    # no layer4 launch, no intermediate returned
    ("bott_c64_l23", case(net("Bottleneck", BOTT1, 64), (1, 3, 40, 56), ["layer2", "layer3"], 6)),
    # conv1 alone: before the pool in resnet.py, behind it in resnet_mrcnn.py; the call returns behind the stem
    ("conv1_only", case(net("Bottleneck", BOTT1, 16), (2, 3, 33, 47), ["conv1"], 7)),
    ("conv1_only_mrcnn", case(net("Bottleneck", BOTT1, 16, mrcnn=True), (2, 3, 33, 47), ["conv1"], 7)),
    ("basic_tiny", case(net("BasicBlock", [2, 2, 2, 2], 16), (2, 3, 33, 47), ALL, 8)),
    ("basic_r18_64", case(net("BasicBlock", [2, 2, 2, 2], 64), (1, 3, 64, 64), ALL, 9)),
    ("mrcnn_tiny", case(net("Bottleneck", BOTT1, 16, mrcnn=True), (2, 3, 33, 47), ["conv1", "layer1", "layer2", "layer3"], 10)),
    # routes the cases above do not reach (tests/test_backbone_cpu.py checks the table against a sweep of the plan)
    ("route_t128", case(net("Bottleneck", BOTT1, 64), (1, 3, 364, 364), ["layer1"], 11)),       # 64 -> 256 at 91x91: 65 x 4 tiles of 128
    ("route_t64", case(net("Bottleneck", BOTT1, 16), (4, 3, 256, 256), ["layer1"], 12)),        # M = 16384, one column tile
    # the deployed shapes
    ("r50_288", case(net("Bottleneck", [3, 4, 6, 3], 64), (1, 3, 288, 288), ["layer2", "layer3"], 20, deployed=True)),
    ("r50_288_n3", case(net("Bottleneck", [3, 4, 6, 3], 64), (3, 3, 288, 288), ["layer2", "layer3"], 21, deployed=True)),
    ("r18_288", case(net("BasicBlock", [2, 2, 2, 2], 64), (1, 3, 288, 288), ["layer2", "layer3"], 22, deployed=True)),
])
SMALL = [k for k, c in CASES.items() if not c["deployed"]]
DEPLOYED = [k for k, c in CASES.items() if c["deployed"]]


def params(name):
    """OrderedDict {state_dict key: numpy array} of the case, every key of the reference class, float32 (the counters int64)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 + c["seed"])
    out = OrderedDict()
    for key, shape, role in RN.keys(c["spec"]):
        if isinstance(role, tuple):
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (role[1] * role[1] * role[2]))
        elif role in ("gamma", "var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif role == "gamma_last":
            v = rng.uniform(0.1, 0.4, shape)
        elif role in ("beta", "mean"):
            v = rng.standard_normal(shape) * 0.1
        elif role == "count":
            out[key] = np.zeros((), np.int64)
            continue
        else:                                                       # the classifier no covered output reads
            v = rng.standard_normal(shape) * 0.01 if role == "fc_w" else np.zeros(shape)
        out[key] = v.astype(np.float32)
    return out


def image(name):
    c = CASES[name]
    return np.random.default_rng(2000 + c["seed"]).standard_normal(c["shape"]).astype(np.float32)


def subset(name, output, numel):
    """The fixed flat positions a deployed case stores of `output` (sorted)."""
    rng = np.random.default_rng(3000 + 10 * CASES[name]["seed"] + RN.OUTPUTS.index(output))
    return np.sort(rng.permutation(numel)[:SUBSET]) if numel > SUBSET else np.arange(numel)


def golden_files(name):
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, f"backbone_{name}.npz")) + glob.glob(os.path.join(GOLDEN_DIR, f"backbone_{name}__*.npz")))


_GOLDEN = {}


def golden(name):
    if name not in _GOLDEN:
        g = {}
        for f in golden_files(name):
            g.update(np.load(f))
        assert g, f"no golden of {name}: run tools/make_golden_backbone.py"
        _GOLDEN[name] = g
    return _GOLDEN[name]


def at_subset(name, output, full):
    """What the golden of `output` is compared with: the map, flat, at the stored positions."""
    full = np.asarray(full)
    return full.reshape(-1)[subset(name, output, full.size)]
