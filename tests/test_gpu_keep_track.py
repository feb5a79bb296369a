"""KeepTrack target-candidate matching on the MI355X (tcm.hip through pytracking_amd.candidate_matching) against the unmodified
reference's goldens (tools/make_golden_keep_track.py): peaks bit-exact, descriptors within 1e-4, the matcher's log_assignment within
1e-4 with exact matches; install() takes the fast branch on device and hands the uncovered cases to the reference; a captured graph
replays bit-equal to the eager call; an in-place weight update takes effect on the next call."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_harness
from pytracking_amd import candidate_matching as CM, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="reference bundle missing")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
PEAKS = ["tcm_peaks_23", "tcm_peaks_31", "tcm_peaks_noise", "tcm_peaks_boundary"]
DESC = ["tcm_desc_fast_p1", "tcm_desc_fast_p7", "tcm_desc_fast_p40", "tcm_desc_default_p1", "tcm_desc_default_p7",
        "tcm_desc_default_p40"]
MATCH = ["tcm_match_1x2", "tcm_match_2x1", "tcm_match_3x5", "tcm_match_8x8", "tcm_match_17x31", "tcm_match_64x64",
         "tcm_match_skip_gnn", "tcm_match_it50"]


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _extractor(seed):
    ref_harness.install()
    from ltr.models.target_candidate_matching.target_candidate_matching import DescriptorExtractor
    ext = DescriptorExtractor(1024, 256, 4)
    w, b = synth.tcm_desc_conv(seed + 1)
    ext.conv.weight.data.copy_(torch.from_numpy(w))
    ext.conv.bias.data.copy_(torch.from_numpy(b))
    return ext.to(DEV).eval()


def _superglue(g):
    ref_harness.install()
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    skip = bool(g["skip_gnn"])
    sg = SuperGlue({'skip_gnn': skip, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': int(g["iters"]),
                    'output_normalization': 'sinkhorn'})
    sg.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.tcm_superglue_state(int(g["seed"]), 4, skip).items()})
    return sg.to(DEV).eval()


def _data(g, dev=DEV):
    d = {k: torch.from_numpy(g[k].copy()).to(dev) for k in ("descriptors0", "descriptors1", "img_coords0", "img_coords1", "scores0",
                                                            "scores1")}
    d["image_size0"] = d["image_size1"] = torch.Size(tuple(int(v) for v in g["image_shape"]))
    return d


@pytest.mark.parametrize("name", PEAKS)
def test_peaks_bit_exact(name):
    g = _load(name)
    c, v = CM.find_local_maxima(torch.from_numpy(g["scores"]).to(DEV), float(g["th"]), int(g["ks"]))
    assert c.dtype == torch.int64 and v.dtype == torch.float32 and c.shape == (len(g["coords"]), 2)
    np.testing.assert_array_equal(c.cpu().numpy(), g["coords"])
    np.testing.assert_array_equal(v.cpu().numpy(), g["values"])


def test_peaks_batch_and_plateau():
    ref_harness.install()                      # the 4-D form returns the reference's TensorList
    g = _load("tcm_peaks_batch")
    cs, vs = CM.find_local_maxima(torch.from_numpy(g["scores"]).to(DEV), float(g["th"]), int(g["ks"]))
    assert type(cs).__name__ == "TensorList" and len(cs) == len(g["counts"])
    off = 0
    for c, v, n in zip(cs, vs, g["counts"]):
        np.testing.assert_array_equal(c.cpu().numpy(), g["coords"][off:off + n])
        np.testing.assert_array_equal(v.cpu().numpy(), g["values"][off:off + n])
        off += n
    g = _load("tcm_peaks_plateau")
    c, v = CM.find_local_maxima(torch.from_numpy(g["scores"]).to(DEV), float(g["th"]), int(g["ks"]))
    assert sorted(map(tuple, c.cpu().numpy())) == sorted(map(tuple, g["coords"]))
    assert np.all(np.diff(v.cpu().numpy()) <= 0)


@pytest.mark.parametrize("name", DESC)
def test_descriptors_match_golden(name):
    g = _load(name)
    ext = _extractor(int(g["seed"]))
    x = torch.from_numpy(synth.tcm_layer3(int(g["seed"]), 1, 1024, int(g["H"]), int(g["W"]))).to(DEV)
    coords = torch.from_numpy(g["coords"]).to(DEV)
    with torch.no_grad():
        out = CM.get_descriptors(ext, x, coords)
        again = CM.get_descriptors(ext, x, coords)
    assert out.shape == g["desc"].shape
    np.testing.assert_allclose(out.cpu().numpy(), g["desc"], atol=1e-4, rtol=0)
    assert torch.equal(out, again)


@pytest.mark.parametrize("name", MATCH)
def test_matcher_matches_golden(name):
    g = _load(name)
    sg = _superglue(g)
    with torch.no_grad():
        pred = CM.match(sg, _data(g))
        again = CM.match(sg, _data(g))
    M, N = int(g["M"]), int(g["N"])
    assert pred["log_assignment"].shape == (1, M + 1, N + 1)
    assert pred["matches0"].dtype == torch.int64 and pred["matches0"].shape == (1, M) and pred["matches1"].shape == (1, N)
    assert pred["match_scores0"].dtype == torch.float32 and pred["bin_score"] is sg.bin_score
    np.testing.assert_allclose(pred["log_assignment"][0].cpu().numpy(), g["log_assignment"], atol=1e-4, rtol=0)
    np.testing.assert_array_equal(pred["matches0"][0].cpu().numpy(), g["matches0"])
    np.testing.assert_array_equal(pred["matches1"][0].cpu().numpy(), g["matches1"])
    np.testing.assert_allclose(pred["match_scores0"][0].cpu().numpy(), g["match_scores0"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(pred["match_scores1"][0].cpu().numpy(), g["match_scores1"], atol=1e-5, rtol=0)
    for k in ("log_assignment", "matches0", "matches1", "match_scores0", "match_scores1"):
        assert torch.equal(pred[k], again[k]), k


def test_install_fast_branch_and_fallbacks():
    ref_harness.install()
    from pytracking_amd import install as amd
    import ltr.data.processing_utils as prutils
    amd.install()
    try:
        g = _load("tcm_match_8x8")
        sg = _superglue(g)
        amd.stats.clear()
        with torch.no_grad():
            pred = sg(_data(g))
        assert amd.stats["SuperGlue._forward.fast"] == 1 and amd.stats["SuperGlue._forward.reference"] == 0
        np.testing.assert_allclose(pred["log_assignment"][0].cpu().numpy(), g["log_assignment"], atol=1e-4, rtol=0)
        # grad-enabled parameters, training mode, CPU tensors, more than 64 candidates: the reference
        amd.stats.clear()
        sg(_data(g))
        sg.train()
        with torch.no_grad():
            sg(_data(g))
        sg.eval()
        with torch.no_grad():
            sg.cpu()(_data(g, "cpu"))
            sg.to(DEV)
            big = synth.tcm_match_inputs(5, 65, 3)
            d = {k: torch.from_numpy(v).to(DEV) for k, v in big.items()}
            d["image_size0"] = d["image_size1"] = torch.Size((480, 640))
            sg(d)
        assert amd.stats["SuperGlue._forward.reference"] == 4 and amd.stats["SuperGlue._forward.fast"] == 0
        # peaks and descriptors through the rebound names
        gp = _load("tcm_peaks_23")
        amd.stats.clear()
        c, v = prutils.find_local_maxima(torch.from_numpy(gp["scores"]).to(DEV), ks=5, th=float(gp["th"]))
        np.testing.assert_array_equal(c.cpu().numpy(), gp["coords"])
        gd = _load("tcm_desc_fast_p7")
        ext = _extractor(int(gd["seed"]))
        x = torch.from_numpy(synth.tcm_layer3(int(gd["seed"]), 1, 1024, 22, 22)).to(DEV)
        with torch.no_grad():
            out = ext.get_descriptors(x, torch.from_numpy(gd["coords"]).to(DEV))
        np.testing.assert_allclose(out.cpu().numpy(), gd["desc"], atol=1e-4, rtol=0)
        assert amd.stats["find_local_maxima.fast"] == 1 and amd.stats["DescriptorExtractor.get_descriptors.fast"] == 1
        assert amd.stats["find_local_maxima.reference"] == 0 and amd.stats["DescriptorExtractor.get_descriptors.reference"] == 0
    finally:
        amd.uninstall()


def test_graph_replay_bit_equal_and_inplace_update():
    g = _load("tcm_match_17x31")
    sg = _superglue(g)
    data = _data(g)
    gd = _load("tcm_desc_fast_p40")
    ext = _extractor(int(gd["seed"]))
    x = torch.from_numpy(synth.tcm_layer3(int(gd["seed"]), 1, 1024, 22, 22)).to(DEV)
    coords = torch.from_numpy(gd["coords"]).to(DEV)
    with torch.no_grad():
        eager = CM.match(sg, data)
        eager_d = CM.get_descriptors(ext, x, coords)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            CM.match(sg, data)
            CM.get_descriptors(ext, x, coords)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = CM.match(sg, data)
            cap_d = CM.get_descriptors(ext, x, coords)
        graph.replay()
        torch.cuda.synchronize()
    for k in ("log_assignment", "matches0", "matches1", "match_scores0", "match_scores1"):
        assert torch.equal(cap[k], eager[k]), k
    assert torch.equal(cap_d, eager_d)
    # bin_score is read at call time; an in-place update of a weight through an ordinary op takes effect on the next call
    with torch.no_grad():
        sg.bin_score.add_(0.5)
        la_bin = CM.match(sg, data)["log_assignment"]
        sg.gnn.layers[0].update.mlp[1].running_mean.mul_(2.0)
        la_bn = CM.match(sg, data)["log_assignment"]
        sg.gnn.layers[0].update.mlp[1].running_mean.div_(2.0)
        sg.bin_score.sub_(0.5)
        back = CM.match(sg, data)["log_assignment"]
    assert (la_bin - eager["log_assignment"]).abs().max() > 1e-3
    assert (la_bn - la_bin).abs().max() > 1e-4
    torch.testing.assert_close(back, eager["log_assignment"], atol=1e-6, rtol=0)
