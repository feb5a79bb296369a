"""IoU feature extraction on the MI355X (iou_feat.hip through pytracking_amd.iou_feat): every case of synth.IOU_FEAT_CASES against the golden
of the unmodified reference's fp32 CPU run (tools/make_golden_iou_feat.py) within the project's 1e-4 absolute -- the reference's own
distance from float64 is recorded in each golden and is at most 2.3e-6 -- 5-D inputs, bit-identical repeats, graph capture, the weight
cache, install(iou_feat=True) on the bundle's AtomIoUNet, and the refined boxes downstream of the fused features.

Every test prints its measured maximum error before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import iou_feat_cases as IC
from f64_bound import dev, needs_bundle
from oracle import ref_harness
from pytracking_amd import iou_feat as IF, iou_refine as IR, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4


def _run(name, net=None):
    g, n, t3, t4, sd, (f3, f4) = IC.case(name)
    net = IC.module(name, DEV) if net is None else net
    with torch.no_grad():
        feats = [dev(f3), dev(f4)]
        assert IF.covered(net, feats)
        c3, c4 = IF.get_iou_feat(net, feats)
    return g, net, feats, c3, c4


@pytest.mark.parametrize("name", IC.CASES)
def test_matches_reference_golden(name):
    g, net, feats, c3, c4 = _run(name)
    n, t3, t4 = synth.IOU_FEAT_CASES[name]
    assert c3.shape == (n, t3[2], t3[3], t3[4]) and c4.shape == (n, t4[2], t4[3], t4[4])
    err = IC.against_golden(g, c3.cpu().numpy(), c4.cpu().numpy())
    print(f"\niou_feat_{name}: max |gpu - reference fp32| = {err:.3e} (bound {ATOL:.0e}, ref_fp32_err {float(g['ref_fp32_err']):.3e})")
    assert err <= ATOL
    with torch.no_grad():
        d3, d4 = IF.get_iou_feat(net, feats)
    assert torch.equal(c3, d3) and torch.equal(c4, d4)                 # two calls are bit-identical


def test_five_dimensional_input():
    g, net, feats, c3, c4 = _run("b")
    with torch.no_grad():
        five = [f.reshape(1, *f.shape) for f in feats]                  # (images, sequences, C, H, W) as atom_iou_net.py:174 takes it
        assert IF.covered(net, five)
        e3, e4 = IF.get_iou_feat(net, five)
        mixed = IF.get_iou_feat(net, [feats[0].reshape(2, 1, *feats[0].shape[1:]), feats[1]])
    assert e3.shape == c3.shape and torch.equal(e3, c3) and torch.equal(e4, c4)
    assert torch.equal(mixed[0], c3) and torch.equal(mixed[1], c4)


@pytest.mark.parametrize("name", ["c", "dimp50"])
def test_graph_capture_replays_the_eager_bits(name):
    g, net, feats, c3, c4 = _run(name)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            IF.get_iou_feat(net, feats)                                 # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            k3, k4 = IF.get_iou_feat(net, feats)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(k3, c3) and torch.equal(k4, c4)


def test_cache_follows_load_state_dict_and_in_place_updates():
    g, n, t3, t4, sd, (f3, f4) = IC.case("c")
    net = IC.module("c", DEV)
    feats = [dev(f3), dev(f4)]
    other = synth.iou_feat_state(int(g["state_seed"]) + 50, t3[0], t4[0], t3[1], t3[2], t4[1], t4[2])
    with torch.no_grad():
        first = IF.get_iou_feat(net, feats)
        net.load_state_dict(IC.state_tensors(other))
        fresh = IC.Towers(t3, t4)
        fresh.load_state_dict(IC.state_tensors(other))
        want = IF.get_iou_feat(fresh.to(DEV).eval(), feats)
        got = IF.get_iou_feat(net, feats)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], first[0])
        net.conv3_2t[1].running_var.mul_(1.7)                           # in place
        net.conv4_1t[1].running_var.add_(0.3)
        changed = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        fresh2 = IC.Towers(t3, t4)
        fresh2.load_state_dict(changed)
        want2 = IF.get_iou_feat(fresh2.to(DEV).eval(), feats)
        got2 = IF.get_iou_feat(net, feats)
        stock = net.get_iou_feat(feats)                                 # the same module in stock PyTorch on the device
    assert torch.equal(got2[0], want2[0]) and torch.equal(got2[1], want2[1]) and not torch.equal(got2[0], got[0])
    err = max(float((got2[0] - stock[0]).abs().max()), float((got2[1] - stock[1]).abs().max()))
    print(f"\nafter the in-place change: max |fused - stock on device| = {err:.3e}")
    assert err <= 2 * ATOL                                              # both sides within 1e-4 of the exact value


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(iou_feat=True)
    try:
        yield amd
    finally:
        amd.uninstall()


def _bundle_net(seed=1234):
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    g, n, t3, t4, sd, (f3, f4) = IC.case("dimp50")
    net = AtomIoUNet(input_dim=(t3[0], t4[0]), pred_input_dim=(t3[2], t4[2]), pred_inter_dim=(256, 256))
    state = IC.state_tensors(sd)
    state.update({k: torch.from_numpy(v.copy()) for k, v in synth.iou_net_params(seed).items()})
    net.load_state_dict(state, strict=False)
    return g, net.to(DEV).eval(), [dev(f3), dev(f4)]


@needs_bundle
def test_install_dispatches_the_bundles_module(amd):
    g, net, feats = _bundle_net()
    amd.stats.clear()
    with torch.no_grad():
        c3, c4 = net.get_iou_feat(feats)
    assert amd.stats["AtomIoUNet.get_iou_feat.fast"] == 1 and amd.stats["AtomIoUNet.get_iou_feat.reference"] == 0
    err = IC.against_golden(g, c3.cpu().numpy(), c4.cpu().numpy())
    print(f"\ninstall(iou_feat=True), DiMP-50: max |gpu - reference fp32| = {err:.3e}")
    assert err <= ATOL
    net.train()
    with torch.no_grad():
        net.get_iou_feat([f[:, :, :4, :4] for f in feats])             # training mode: the reference branch (batch statistics)
    assert amd.stats["AtomIoUNet.get_iou_feat.fast"] == 1 and amd.stats["AtomIoUNet.get_iou_feat.reference"] == 1


@needs_bundle
def test_refined_boxes_downstream_agree_with_the_stock_features(amd):
    """The fused features and the stock module's features (same device) through the same refinement: refined boxes within the allowance
    tests/trackers_on_device.py gives refined boxes, 1e-4 + 1e-6 x the largest coordinate."""
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    g, net, feats = _bundle_net()
    _, _, mod3, mod4, boxes = synth.iou_inputs(77)
    with torch.no_grad():
        fused = net.get_iou_feat(feats)
        stock = amd.original(AtomIoUNet, "get_iou_feat")(net, feats)
        out = [IR.refine_boxes(net, (dev(mod3), dev(mod4)), f, torch.from_numpy(boxes.copy()), 5, 1.0, 1.0, False) for f in (fused, stock)]
    (bf, jf), (bs, js) = [(b.cpu().numpy(), j.cpu().numpy()) for b, j in out]
    tol = 1e-4 + 1e-6 * float(np.abs(bs).max())
    db, dj = float(np.abs(bf - bs).max()), float(np.abs(jf - js).max())
    print(f"\nrefined boxes: max |fused - stock| = {db:.3e} px (allowance {tol:.3e}), IoU {dj:.3e}; moved {float(np.abs(bs - boxes).max()):.2f} px")
    assert float(np.abs(bs - boxes).max()) > 1e-2                       # the refinement moved the proposals
    assert db <= tol
