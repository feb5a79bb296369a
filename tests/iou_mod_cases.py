"""Shared by tests/test_iou_mod_cpu.py and tests/test_gpu_iou_mod.py: the golden cases (synth.IOU_MOD_CASES) with their seeded state and
inputs, and a plain-torch module with the five reference-branch blocks and the two pooling objects of AtomIoUNet (atom_iou_net.py:7-12,
26, 31, 34, 36, 41, 44-45) for the tests that must not read the reference tree.  Test infrastructure only.

  case      n   maps                         what it exercises
  one       1   Cin 64, both maps 1 x 1      every tap but the centre is padding
  edges     6   9 x 11 and 5 x 6             a box inside, over the top-left edge, wholly outside, of zero width, the whole map, in one pixel
  tiles     2   20 x 19 and 10 x 9           a stride-8 window 17 columns wide (straddles a 16-position tile); bins wider than 6 pixels
  batch     32  6 x 6 and 3 x 3              the same map in every image, a different box per image; n at its limit
  chan      3   7 x 5 and 4 x 3              Cin3 128, Cin4 192, A 48, B 32, D 80, P3 16, P4 48: the concatenation order
  dimp50 / prdimp50 / atom18                 the deployed sizes with the boxes of the first-frame augmentations"""
import os

import numpy as np
import torch

from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ("one", "edges", "tiles", "batch", "chan")
DEPLOYED = ("dimp50", "prdimp50", "atom18")
CASES = SMALL + DEPLOYED
S3, S4 = 1.0 / 8, 1.0 / 16
# The weakest seeded defect of tests/test_iou_mod_cpu.py (s4 used for level 3) lies 2.03e6 x max(ref_fp32_err, 2^-23 max|want|) from the
# reference's float64 output on its best case (`chan`), the other five between 2.6e6 and 7.7e6 x: every one is structural.
# f64_bound.raised_factor(worst measured, F_MAX) may never exceed this.
F_MAX = 2.0e6
_CACHE = {}


def conv(cin, cout, kernel_size=3, padding=1, dilation=1):
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, kernel_size=kernel_size, stride=1, padding=padding, dilation=dilation, bias=True),
                               torch.nn.BatchNorm2d(cout), torch.nn.ReLU(inplace=True))


class Pool(torch.nn.Module):
    """What get_modulation reads of a PrRoIPool2D: the pooled size and the scale (`pool`: the callable that pools, for device runs)."""

    def __init__(self, size, scale, pool=None):
        super().__init__()
        self.pooled_height, self.pooled_width, self.spatial_scale, self.pool = size, size, scale, pool

    def forward(self, features, rois):
        return self.pool(features, rois, self.pooled_height, self.pooled_width, self.spatial_scale)


class ModNet(torch.nn.Module):
    """The five blocks and two pooling objects get_modulation reads, under the reference's attribute names."""

    def __init__(self, cin3, cin4, dims, pool=None):
        super().__init__()
        A, B, D, P3, P4 = dims
        self.conv3_1r, self.conv4_1r = conv(cin3, A), conv(cin4, D)
        self.fc3_1r = conv(A, B, padding=0)
        self.fc34_3r, self.fc34_4r = conv(B + D, P3, kernel_size=1, padding=0), conv(B + D, P4, kernel_size=1, padding=0)
        self.prroi_pool3r, self.prroi_pool4r = Pool(3, S3, pool), Pool(1, S4, pool)

    def get_modulation(self, feat, bb):     # atom_iou_net.py:138-170, for comparisons on the device
        c3, c4 = self.conv3_1r(feat[0]), self.conv4_1r(feat[1])
        roi = torch.cat((torch.arange(bb.shape[0], dtype=torch.float32, device=bb.device).reshape(-1, 1), bb[:, 0:2], bb[:, 0:2] + bb[:, 2:4]), 1)
        cat = torch.cat((self.fc3_1r(self.prroi_pool3r(c3, roi)), self.prroi_pool4r(c4, roi)), 1)
        return self.fc34_3r(cat), self.fc34_4r(cat)


def case(name):
    """(golden dict, n, (Cin3, H3, W3), (Cin4, H4, W4), dims, state dict (numpy), (feat3, feat4, bb) (numpy)), generated once per session."""
    if name not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, f"iou_mod_{name}.npz")))
        n, l3, l4, dims = synth.IOU_MOD_CASES[name]
        assert (int(g["n"]), tuple(int(v) for v in g["level3"]), tuple(int(v) for v in g["level4"]), tuple(int(v) for v in g["dims"])) == (n, l3, l4, dims)
        sd = synth.iou_mod_state(int(g["state_seed"]), l3[0], l4[0], *dims)
        f3, f4, bb = synth.iou_mod_inputs(int(g["input_seed"]), name)
        assert np.array_equal(bb, g["boxes"])
        for a in (f3, f4, bb):
            a.setflags(write=False)
        _CACHE[name] = (g, n, l3, l4, dims, sd, (f3, f4, bb))
    return _CACHE[name]


def state_tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def module(name, device="cpu", pool=None):
    _, _, l3, l4, dims, sd, _ = case(name)
    net = ModNet(l3[0], l4[0], dims, pool)
    net.load_state_dict(state_tensors(sd))
    return net.to(device).eval()


def want(g):
    """{output: the reference's float64 run}"""
    return {"out3": g["out3_f64"], "out4": g["out4_f64"]}
