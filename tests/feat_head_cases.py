"""Shared by tests/test_feat_head_cpu.py, tests/test_gpu_feat_head.py, tools/make_golden_feat_head.py and tools/bench_feat_head.py: the
cases of the LWL / RTS feature heads (synth.FEAT_HEAD_CASES) with their seeded inputs and weights, the plain-torch stand-in of the head --
`F.conv2d(stride, padding=1)` followed by the expression of InstanceL2Norm (ltr/models/layers/normalization.py:15-18) -- for the tests that
must not read the reference tree, and its float64 anchor: for a case the stand-in runs once in float64 on the CPU (`want`) and once in
fp32 on the CPU with f64_bound.THREADS threads; `ref_err` is the largest |fp32 - float64|, what fp32 arithmetic costs on this very case in
an order of summation nobody tuned.  A device output is held to the bound of tests/f64_bound.py, FACTOR x ref_err of `want`;
tests/test_feat_head_cpu.py fails if it is raised until a head with 10-bit weights or with a shifted tap origin passes.  Test
infrastructure only."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import f64_bound
from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tuple(synth.FEAT_HEAD_CASES)
SCALE, EPS = synth.FEAT_HEAD_SCALE, 1e-5
SEED = 2300                                   # case k: inputs and weights from SEED + k
X_STORED_MAX = 4096                           # a golden stores its input up to this many values; larger ones are regenerated from the seed
FACTOR = f64_bound.FACTOR
_CACHE = {}


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def problem(name):
    """(x, weight) of a small case as CPU tensors."""
    x, w = synth.feat_head_problem(SEED + CASES.index(name), *synth.FEAT_HEAD_CASES[name])
    return torch.from_numpy(x), torch.from_numpy(w)


def standin(x, w, stride, scale=SCALE, eps=EPS, origin=-1):
    """The head in plain torch, in the dtype of its arguments.  origin: tap (ky, kx) of output (y, x) reads input
    (stride*y + ky + origin, ...); -1 is the head, 0 the shifted mutant of the sensitivity test."""
    with torch.no_grad():
        y = F.conv2d(x, w, stride=stride, padding=1) if origin == -1 else F.conv2d(F.pad(x, (0, 2, 0, 2)), w, stride=stride)
        return y * (scale * ((y.shape[1] * y.shape[2] * y.shape[3]) / (
            torch.sum((y * y).view(y.shape[0], 1, 1, -1), dim=3, keepdim=True) + eps)).sqrt())


def anchor(key, x, w, stride, scale=SCALE, eps=EPS):
    """Anchor of the stand-in on the CPU tensors (x, w), computed once per session under `key`; `want` is the one output's array."""
    def run(dtype):
        return OrderedDict(y=standin(x, w, stride, scale, eps) if dtype == np.float32 else standin(x.double(), w.double(), stride, scale, eps))
    a = f64_bound.anchor(("feat_head", key), run, threads=f64_bound.THREADS)
    return a._replace(want=a.want["y"])


def small(name, stride=2):
    """(x, w, Anchor) of a small case."""
    x, w = problem(name)
    return x, w, anchor(("small", name, stride), x, w, stride)


def deployed(n, stride, seed):
    """(x, w, Anchor) of the deployed head, 1024 x 30 x 52 -> 512, on n images from a synth seed."""
    _, Cin, Cout, H, W = synth.FEAT_HEAD_DEPLOYED
    key = ("deployed", n, stride, seed)
    if key not in _CACHE:
        x, w = synth.feat_head_problem(seed, n, Cin, Cout, H, W)
        x, w = torch.from_numpy(x), torch.from_numpy(w)
        _CACHE[key] = (x, w, anchor(key + ("anchor",), x, w, stride))
    return _CACHE[key]


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"feat_head_{name}.npz")))
