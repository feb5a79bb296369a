"""The float64 anchor of the three fused modules -- IoU feature extraction (iou_feat.hip), the mask label encoder (label_enc.hip) and the
LWL / RTS segmentation decoder (lwl_decoder.hip) -- shared by tests/test_fused_bounds_cpu.py, tests/test_fused_edge_cases_cpu.py and
tests/test_gpu_fused_f64.py.  For a module instance and its inputs the plain-torch stand-in (tests/iou_feat_cases.py,
tests/label_enc_cases.py, tests/lwl_decoder_cases.py) runs once in float64 on the CPU (`want`, per output tensor) and once in fp32 on the
CPU; `ref_err` is the largest |fp32 - float64| over all outputs of the case: what fp32 arithmetic costs on this very case in an order of
summation nobody tuned.  A device output is held to bound(ref_err) = FACTOR * ref_err of `want`, as tests/test_gpu_kys.py holds the cost
volume to 4 x its golden's ref_fp32_err.  The anchor, FACTOR and the bound are those of tests/f64_bound.py; tests/test_fused_bounds_cpu.py
fails if FACTOR is raised until a doubled BatchNorm eps or a convolution with 10-bit weights passes.  Reads nothing outside the repository.  Test infrastructure
only."""
import copy
from collections import OrderedDict

import numpy as np
import torch

import f64_bound
import iou_feat_cases as IC
import label_enc_cases as LC
import lwl_decoder_cases as DC
from f64_bound import FACTOR, THREADS, bound, errors, report  # noqa: F401  (tests/f64_bound.py's, re-exported to the users of this module)

KINDS = ("iou_feat", "label_enc", "lwl_decoder")
SMALL = {"iou_feat": IC.SMALL, "label_enc": tuple(c for c in LC.CASES if c != "deployed"),
         "lwl_decoder": tuple(c for c in DC.CASES if c != "deployed")}
DEPLOYED = {"iou_feat": IC.DEPLOYED, "label_enc": ("deployed",), "lwl_decoder": ("deployed",)}


def convert(args, device=None, dtype=None):
    """The arguments of a case with every floating tensor moved to `device` / `dtype`; sizes and names as they are."""
    if isinstance(args, torch.Tensor):
        return args.to(device=device, dtype=dtype if args.is_floating_point() else None)
    if isinstance(args, dict):
        return type(args)((k, convert(v, device, dtype)) for k, v in args.items())
    if isinstance(args, (list, tuple)) and any(isinstance(v, (torch.Tensor, dict)) for v in args):
        return type(args)(convert(v, device, dtype) for v in args)
    return args


def standin(kind, net, args):
    """One call of the stand-in `net` -> OrderedDict {output name: tensor}.  args: iou_feat dict(feats=(f3, f4)); label_enc dict(masks=
    (n, 1, H, W)); lwl_decoder dict(scores=(n, 1, ic, h, w), feats={layer: map}, image=(H, W), names=['{L}_dec', ...])."""
    with torch.no_grad():
        if kind == "iou_feat":
            c3, c4 = net.get_iou_feat(list(args["feats"]))
            return OrderedDict((("c3", c3), ("c4", c4)))
        if kind == "label_enc":
            enc, sw = net(args["masks"])
            return OrderedDict((("label_enc", enc), ("sample_w", sw)))
        mask, outs = net(args["scores"], args["feats"], args["image"], args["names"])
        return OrderedDict([(q, outs[q]) for q in args["names"]] + [("mask", mask)])


def anchor(kind, key, net, args):
    """Anchor of the fp32 CPU stand-in `net` on the CPU arguments `args`, computed once per session under (kind, key)."""
    def run(dtype):
        if dtype == np.float32:
            return standin(kind, net, args)
        return standin(kind, copy.deepcopy(net).double(), convert(args, dtype=torch.float64))
    return f64_bound.anchor(("fused", kind, key), run, threads=THREADS)


def committed_case(kind, name):
    """(stand-in module on the CPU, CPU arguments, the golden's ref_fp32_err) of a committed case of synth.*_CASES."""
    if kind == "iou_feat":
        g, _, _, _, _, (f3, f4) = IC.case(name)
        return IC.module(name), dict(feats=(torch.from_numpy(f3), torch.from_numpy(f4))), float(g["ref_fp32_err"])
    if kind == "label_enc":
        g, masks = LC.case(name)[0], LC.case(name)[7]
        return LC.module(name), dict(masks=torch.from_numpy(masks)[:, None]), float(g["ref_fp32_err"])
    g, c, _, _, _ = DC.case(name)
    s, feats = DC.inputs(name)
    return DC.module(name), dict(scores=s, feats=feats, image=tuple(c["image"]), names=DC.level_names(c)), float(g["ref_fp32_err"])


def committed(kind, name):
    net, args, _ = committed_case(kind, name)
    return anchor(kind, ("committed", name), net, args)
