"""The three fused modules on the MI355X against float64: IoU feature extraction (iou_feat.hip), the mask label encoder (label_enc.hip) and
the LWL / RTS segmentation decoder (lwl_decoder.hip), each through its public mirror, on every committed case of synth.*_CASES (the
deployed sizes in full) and every edge case of tests/fused_edge_cases.py.  Every output tensor -- for the decoder the mask AND every
'{L}_dec' level, which places a failure at a level -- is held to bound(ref_err) = FACTOR x the fp32 CPU stand-in's own distance from
float64 on that case (tests/fused_f64.py), where the golden tests allow a flat 1e-4.  Edge cases repeat bit for bit, and every sample of
the n = 8 and n = 33 cases equals the same sample run alone: bit for bit where every sum runs in the same order either way
(fused_edge_cases.routes_coincide), within the bound where the plan follows n.

Every test prints per output the measured max |gpu - float64| and its ratio to ref_err before it asserts (run with -s)."""
import copy

import pytest
import torch

import fused_edge_cases as EC
import fused_f64 as F64
from pytracking_amd import _lib, iou_feat as IF, label_encoder as LE, lwl_decoder as LD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMMITTED = [(kind, name) for kind in F64.KINDS for name in F64.SMALL[kind] + F64.DEPLOYED[kind]]
EDGE = [(kind, name) for kind in F64.KINDS for name in EC.CASES[kind]]
_RUNS = {}


def fused(kind, net, args):
    """One call of the fused module through its public mirror -> {output name: device tensor}, named as fused_f64.standin names them."""
    with torch.no_grad():
        if kind == "iou_feat":
            assert IF.covered(net, list(args["feats"]))
            return dict(zip(("c3", "c4"), IF.get_iou_feat(net, list(args["feats"]))))
        if kind == "label_enc":
            assert LE.covered(net, args["masks"])
            return dict(zip(("label_enc", "sample_w"), LE.forward(net, args["masks"])))
        assert LD.covered(net, args["scores"], args["feats"], args["image"], args["names"])
        mask, outs = LD.forward(net, args["scores"], args["feats"], args["image"], args["names"])
        assert list(outs) == list(args["names"])
        return dict(outs, mask=mask)


def _run(source, kind, name):
    """(anchor, module on the device, device arguments, outputs of one fused call), once per session."""
    key = (source, kind, name)
    if key not in _RUNS:
        if source == "committed":
            (net, args, _), anchor = F64.committed_case(kind, name), F64.committed(kind, name)
        else:
            (net, args), anchor = EC.case(kind, name), EC.anchor(kind, name)
        net, args = copy.deepcopy(net).to(DEV), F64.convert(args, device=DEV)            # the CPU module stays what the anchor ran
        out = fused(kind, net, args)
        torch.cuda.synchronize()
        _RUNS[key] = (anchor, net, args, out)
    return _RUNS[key]


def _within_bound(source, kind, name):
    anchor, _, _, out = _run(source, kind, name)
    assert set(out) == set(anchor.want) and all(tuple(out[q].shape) == anchor.want[q].shape for q in out)
    errs = F64.errors(anchor.want, out)
    print(F64.report(f"{kind}_{name} ({source})", errs, anchor.ref_err))
    assert all(e <= F64.bound(anchor.ref_err) for e in errs.values()), errs


@pytest.mark.parametrize("kind,name", COMMITTED)
def test_committed_case_within_the_float64_bound(kind, name):
    _within_bound("committed", kind, name)


@pytest.mark.parametrize("kind,name", EDGE)
def test_edge_case_within_the_float64_bound(kind, name):
    _within_bound("edge", kind, name)


@pytest.mark.parametrize("kind,name", EDGE)
def test_edge_case_repeats_bit_for_bit(kind, name):
    _, net, args, out = _run("edge", kind, name)
    again = fused(kind, net, args)
    assert all(torch.equal(out[q], again[q]) for q in out)


@pytest.mark.parametrize("kind,name", EC.PER_SAMPLE)
def test_every_sample_equals_the_same_sample_alone(kind, name):
    """Distinct samples, each run again with n = 1: an error in a per-image stride or in the grid's z index shows here even where repeated
    inputs would hide it."""
    anchor, net, args, out = _run("edge", kind, name)
    same_bits = EC.routes_coincide(_lib.lib(), kind, name)
    worst, differing = 0.0, []
    for k in range(EC.samples(kind, name)):
        alone = fused(kind, net, EC.sample(kind, args, k))
        for q in out:
            a, b = alone[q].reshape(out[q][k:k + 1].shape), out[q][k:k + 1]
            worst = max(worst, float((a.double() - b.double()).abs().max()))
            if not torch.equal(a, b):
                differing.append((k, q))
    print(f"\n{kind}_{name}: max |sample in the batch - sample alone| = {worst:.3e} ({worst / anchor.ref_err:.2f} x ref_err), "
          + ("the same plans: equal bits required" if same_bits else f"plans follow n: bound {F64.bound(anchor.ref_err):.3e}"))
    if same_bits:
        assert not differing, differing
    else:
        assert worst <= F64.bound(anchor.ref_err)
