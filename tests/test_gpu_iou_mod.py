"""IoU modulation vectors on the MI355X (iou_mod.hip through pytracking_amd.iou_mod): every case of synth.IOU_MOD_CASES against the goldens
of the unmodified reference's CPU run (tools/make_golden_iou_mod.py) -- within f64_bound's FACTOR x max(ref_fp32_err, 2^-23 max|want|) of
its float64 outputs and within a flat 1e-4 of its fp32 outputs --, bit-identical repeats, graph capture, nothing outside the window's
footprint feeding the result, nothing read from the workspace before it is written, and install(iou_mod=True) on the bundle's AtomIoUNet.

The CPU does no convolution here: the goldens carry the float64 outputs.  Every test prints its measured error before it asserts (run
with -s); the rows go to profiles/iou_mod_f64.txt when IOU_MOD_F64_OUT names it.  Worst measured ratio on the MI355X: 1.12 x (`edges`), so FACTOR stays 4."""
import ctypes

import numpy as np
import pytest
import torch

import f64_bound
import iou_mod_cases as IC
from f64_bound import dev, needs_bundle
from oracle import ref_harness
from pytracking_amd import _lib, iou_mod as IM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
WORST_MEASURED = 1.12         # `edges` out3, profiles/iou_mod_f64.txt; above FACTOR / 2 the factor would be raised_factor's
FACTOR = f64_bound.raised_factor(WORST_MEASURED, IC.F_MAX)
TABLE = f64_bound.Table("IOU_MOD_F64_OUT", "IoU modulation vectors (iou_mod.hip) on the MI355X against the reference's float64 run: max |out - float64|, the "
                        "reference's own fp32 distance (ref_err), the floor 2^-23 max|want|, and err / max(ref_err, floor)")


def _inputs(name):
    g, n, l3, l4, dims, sd, (f3, f4, bb) = IC.case(name)
    return g, [dev(f3), dev(f4)], dev(bb)


def _run(name, net=None):
    g, feats, bb = _inputs(name)
    net = IC.module(name, DEV) if net is None else net
    with torch.no_grad():
        assert IM.covered(net, feats, bb)
        o3, o4 = IM.get_modulation(net, feats, bb)
    return g, net, feats, bb, o3, o4


@pytest.mark.parametrize("name", IC.CASES)
def test_matches_reference_golden(name):
    g, net, feats, bb, o3, o4 = _run(name)
    n, dims = int(g["n"]), [int(v) for v in g["dims"]]
    assert o3.shape == (n, dims[3], 1, 1) and o4.shape == (n, dims[4], 1, 1)
    got = {"out3": o3.reshape(n, -1), "out4": o4.reshape(n, -1)}
    f64_bound.held("iou_mod " + name, got, IC.want(g), float(g["ref_fp32_err"]), factor=FACTOR, floor=f64_bound.ulp_of_max, table=TABLE)
    flat = max(float(np.abs(got[q].cpu().numpy() - g[q]).max()) for q in got)
    print(f"iou_mod_{name}: max |gpu - reference fp32| = {flat:.3e} (bound {ATOL:.0e})")
    assert flat <= ATOL
    with torch.no_grad():
        d3, d4 = IM.get_modulation(net, feats, bb)
    assert torch.equal(o3, d3) and torch.equal(o4, d4)                 # two calls are bit-identical


def test_leading_slice_of_a_larger_batch():
    """The trackers pass x[:n] of the augmented batch: dense, taken as it is, and the result is that of the n images alone."""
    g, net, feats, bb, o3, o4 = _run("edges")
    with torch.no_grad():
        big = [torch.cat([f, f.flip(0)]) for f in feats]
        sl = [b[:f.shape[0]] for b, f in zip(big, feats)]
        assert all(s.data_ptr() == b.data_ptr() and s.is_contiguous() for s, b in zip(sl, big)) and IM.covered(net, sl, bb)
        e3, e4 = IM.get_modulation(net, sl, bb)
        assert not IM.covered(net, big, bb)                             # maps whose batch is not n
    assert torch.equal(e3, o3) and torch.equal(e4, o4)


@pytest.mark.parametrize("name", ["tiles", "dimp50"])
def test_graph_capture_replays_the_eager_bits(name):
    g, net, feats, bb, o3, o4 = _run(name)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            IM.get_modulation(net, feats, bb)                           # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            k3, k4 = IM.get_modulation(net, feats, bb)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(k3, o3) and torch.equal(k4, o4)


def test_nothing_outside_the_windows_footprint_feeds_the_result():
    """`edges` with every map value outside (window + one halo ring) of its image at 1e30: the same bits as the clean input."""
    g, net, feats, bb, o3, o4 = _run("edges")
    boxes = bb.cpu().numpy()
    dirty = []
    for f, s in zip(feats, (IC.S3, IC.S4)):
        f = f.clone()
        H, W = f.shape[2:]
        for i, b in enumerate(boxes):
            keep = torch.zeros((H, W), dtype=torch.bool, device=f.device)
            win = IM.window(b, s, H, W)
            if win is not None:
                x0, y0, x1, y1 = win
                keep[max(y0 - 1, 0):y1 + 2, max(x0 - 1, 0):x1 + 2] = True
            f[i, :, ~keep] = 1e30
        dirty.append(f)
    assert float(dirty[0].max()) > 9e29 and float(dirty[1].max()) > 9e29 and IM.window(boxes[2], IC.S3, *feats[0].shape[2:]) is None
    with torch.no_grad():
        d3, d4 = IM.get_modulation(net, dirty, bb)
    assert torch.equal(d3, o3) and torch.equal(d4, o4)


def test_raw_call_with_a_poisoned_workspace_gives_the_same_bits():
    """Nothing is read from the workspace before this call wrote it: NaN everywhere in it beforehand changes no bit."""
    g, net, feats, bb, o3, o4 = _run("edges")
    n, dims = int(g["n"]), [int(v) for v in g["dims"]]
    ch = IM._channels(IM._blocks(net))
    sizes = [n, *ch, *feats[0].shape[2:], *feats[1].shape[2:]]
    L = _lib.lib()
    need = L.pt_iou_mod_ws_bytes(*sizes)
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    p3, p4 = torch.empty_like(o3), torch.empty_like(o4)
    pack = IM.packed_weights(net)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.pt_iou_mod_f32(ptr(feats[0]), ptr(feats[1]), ptr(bb), ptr(pack), ptr(p3), ptr(p4), *sizes, IC.S3, IC.S4, ptr(ws), need,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and ws.data_ptr() % 256 == 0
    assert torch.equal(p3, o3) and torch.equal(p4, o4)
    assert bool(torch.isnan(ws).any())                                  # the maps are written only inside the windows


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(iou_mod=True)
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
def test_install_dispatches_the_bundles_module(amd):
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    g, n, l3, l4, dims, sd, _ = IC.case("atom18")
    _, feats, bb = _inputs("atom18")
    net = AtomIoUNet(input_dim=(l3[0], l4[0]), pred_input_dim=(dims[3], dims[4]))
    net.load_state_dict(IC.state_tensors(sd), strict=False)
    net = net.to(DEV).eval()
    amd.stats.clear()
    with torch.no_grad():
        o3, o4 = net.get_modulation(feats, bb)
        d3, d4 = IM.get_modulation(net, feats, bb)
    assert amd.stats["AtomIoUNet.get_modulation.fast"] == 1 and amd.stats["AtomIoUNet.get_modulation.reference"] == 0
    assert torch.equal(o3, d3) and torch.equal(o4, d4)
    got = {"out3": o3.reshape(n, -1), "out4": o4.reshape(n, -1)}
    f64_bound.held("install(iou_mod=True) atom18", got, IC.want(g), float(g["ref_fp32_err"]), factor=FACTOR, floor=f64_bound.ulp_of_max)
    net.train()
    with torch.no_grad():
        net.get_modulation([f[:2, :, :4, :4] for f in feats], bb[:2])  # training mode: the reference branch (batch statistics)
    assert amd.stats["AtomIoUNet.get_modulation.fast"] == 1 and amd.stats["AtomIoUNet.get_modulation.reference"] == 1
