"""Shared by tests/test_feat_head_cpu.py, tests/test_gpu_feat_head.py, tools/make_golden_feat_head.py and tools/bench_feat_head.py: the
cases of the LWL / RTS feature heads (synth.FEAT_HEAD_CASES) with their seeded inputs and weights, the plain-torch stand-in of the head --
`F.conv2d(stride, padding=1)` followed by the expression of InstanceL2Norm (ltr/models/layers/normalization.py:15-18) -- for the tests that
must not read the reference tree, and its float64 anchor: for a case the stand-in runs once in float64 on the CPU (`want`) and once in
fp32 on the CPU with fused_f64.THREADS threads; `ref_err` is the largest |fp32 - float64|, what fp32 arithmetic costs on this very case in
an order of summation nobody tuned.  A device output is held to FACTOR x ref_err of `want`.  FACTOR starts from fused_f64.FACTOR;
tests/test_feat_head_cpu.py fails if it is raised until a head with 10-bit weights or with a shifted tap origin passes.  Test
infrastructure only."""
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import fused_f64 as F64
from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tuple(synth.FEAT_HEAD_CASES)
SCALE, EPS = synth.FEAT_HEAD_SCALE, 1e-5
SEED = 2300                                   # case k: inputs and weights from SEED + k
X_STORED_MAX = 4096                           # a golden stores its input up to this many values; larger ones are regenerated from the seed
FACTOR = F64.FACTOR
Anchor = namedtuple("Anchor", "want ref_err")  # float64 numpy (read-only), float
_CACHE = {}


def bound(ref_err):
    return FACTOR * ref_err


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
    """Anchor of the stand-in on the CPU tensors (x, w), computed once per session under `key`."""
    if key not in _CACHE:
        want = standin(x.double(), w.double(), stride, scale, eps)
        threads = torch.get_num_threads()
        try:
            torch.set_num_threads(F64.THREADS)
            f32 = standin(x, w, stride, scale, eps)
        finally:
            torch.set_num_threads(threads)
        err = float((f32.double() - want).abs().max())
        want = want.numpy()
        want.setflags(write=False)
        _CACHE[key] = Anchor(want, err)
    return _CACHE[key]


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


def max_err(want, got):
    return float(np.abs(got.detach().double().cpu().numpy().reshape(want.shape) - want).max())


def report(tag, err, ref_err):
    """The line every test prints before it asserts."""
    return f"\n{tag}: max |out - float64| {err:.3e} ({err / ref_err:.2f}x)  ref_err {ref_err:.3e}, bound {bound(ref_err):.3e}"
