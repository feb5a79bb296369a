"""Shared by tests/test_iou_feat_cpu.py and tests/test_gpu_iou_feat.py: the golden cases (synth.IOU_FEAT_CASES) with their seeded state and
inputs, and a plain-torch module with the four test-branch blocks of AtomIoUNet (atom_iou_net.py:7-12, 27-29, 37-39) for the tests that
must not read the reference tree.  Test infrastructure only."""
import os

import numpy as np
import torch

from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ("a", "b", "c", "d", "wide")
DEPLOYED = ("dimp50", "prdimp50", "atom18")
CASES = SMALL + DEPLOYED
_CACHE = {}


def conv(cin, cout, dilation=1):
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=dilation, dilation=dilation, bias=True),
                               torch.nn.BatchNorm2d(cout), torch.nn.ReLU(inplace=True))


class Towers(torch.nn.Module):
    """The four blocks get_iou_feat reads, under the reference's attribute names."""

    def __init__(self, t3, t4):
        super().__init__()
        self.conv3_1t, self.conv3_2t = conv(t3[0], t3[1]), conv(t3[1], t3[2])
        self.conv4_1t, self.conv4_2t = conv(t4[0], t4[1]), conv(t4[1], t4[2])

    def get_iou_feat(self, feat2):          # atom_iou_net.py:172-179, for comparisons on the device
        feat2 = [f.reshape(-1, *f.shape[-3:]) if f.dim() == 5 else f for f in feat2]
        return self.conv3_2t(self.conv3_1t(feat2[0])), self.conv4_2t(self.conv4_1t(feat2[1]))


def case(name):
    """(golden dict, n, tower3, tower4, state dict (numpy), (feat3, feat4) (numpy)), generated once per session."""
    if name not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, f"iou_feat_{name}.npz")))
        n, t3, t4 = synth.IOU_FEAT_CASES[name]
        assert (int(g["n"]), tuple(int(v) for v in g["tower3"]), tuple(int(v) for v in g["tower4"])) == (n, t3, t4)
        sd = synth.iou_feat_state(int(g["state_seed"]), t3[0], t4[0], t3[1], t3[2], t4[1], t4[2])
        feats = synth.iou_feat_inputs(int(g["input_seed"]), n, t3[0], t3[3], t3[4], t4[0], t4[3], t4[4])
        _CACHE[name] = (g, n, t3, t4, sd, feats)
    return _CACHE[name]


def state_tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def module(name, device="cpu"):
    _, _, t3, t4, sd, _ = case(name)
    net = Towers(t3, t4)
    net.load_state_dict(state_tensors(sd))
    return net.to(device).eval()


def against_golden(g, c3, c4):
    """Largest |output - golden| over both towers (full maps, or the golden's fixed sample of a deployed case)."""
    errs = []
    for tag, c in (("3", c3), ("4", c4)):
        c = np.asarray(c)
        got = c.reshape(-1)[g["idx" + tag]] if "idx" + tag in g else c
        assert got.shape == g["c" + tag].shape, (got.shape, g["c" + tag].shape)
        errs.append(float(np.abs(got - g["c" + tag]).max()))
    return max(errs)
