"""KeepTrack target-candidate matching (pytracking_amd.candidate_matching, tcm.hip) without a GPU: the goldens of the unmodified
reference (tools/make_golden_keep_track.py) agree with the float64 restatement (tests/tcm_np.py), the weight pack folds the eval
BatchNorms exactly as the module computes, the C ABI refuses bad arguments before any launch, install() binds and uninstall()
restores the new names, and KeepTrack's localisation / box refinement methods are DiMP's in code."""
import ast
import ctypes
import inspect
import os
import textwrap

import numpy as np
import pytest
import torch

import tcm_np
from oracle import ref_harness
from pytracking_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PEAKS = ["tcm_peaks_23", "tcm_peaks_31", "tcm_peaks_noise", "tcm_peaks_boundary"]
DESC = ["tcm_desc_fast_p1", "tcm_desc_fast_p7", "tcm_desc_fast_p40", "tcm_desc_default_p1", "tcm_desc_default_p7",
        "tcm_desc_default_p40"]
MATCH = ["tcm_match_1x2", "tcm_match_2x1", "tcm_match_3x5", "tcm_match_8x8", "tcm_match_17x31", "tcm_match_64x64",
         "tcm_match_skip_gnn", "tcm_match_it50"]
needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _match_data(g):
    shape = tuple(int(v) for v in g["image_shape"])
    d = {k: g[k] for k in ("descriptors0", "descriptors1", "img_coords0", "img_coords1", "scores0", "scores1")}
    d["image_size0"] = d["image_size1"] = shape
    return d


def test_golden_files_are_small():
    for name in PEAKS + ["tcm_peaks_plateau", "tcm_peaks_batch"] + DESC + MATCH:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 256 << 10, name


@pytest.mark.parametrize("name", PEAKS)
def test_numpy_peaks_match_golden(name):
    g = _load(name)
    c, v = tcm_np.find_local_maxima(g["scores"], float(g["th"]), int(g["ks"]))
    np.testing.assert_array_equal(c, g["coords"])
    np.testing.assert_array_equal(v.astype(np.float32), g["values"])


def test_numpy_peaks_boundary_and_plateau():
    g = _load("tcm_peaks_boundary")
    assert [tuple(r) for r in g["coords"]] == [(18, 5), (10, 10)]         # float32(th) itself is not > th; the next float is
    g = _load("tcm_peaks_plateau")
    c, v = tcm_np.find_local_maxima(g["scores"], float(g["th"]), int(g["ks"]))
    assert sorted(map(tuple, c)) == sorted(map(tuple, g["coords"]))      # the order of ties is not pinned by the reference
    assert {(11, 7), (11, 8), (12, 7), (12, 8)} <= set(map(tuple, c))
    g = _load("tcm_peaks_batch")
    off = 0
    for b, n in enumerate(g["counts"]):
        c, v = tcm_np.find_local_maxima(g["scores"][b, 0], float(g["th"]), int(g["ks"]))
        np.testing.assert_array_equal(c, g["coords"][off:off + n])
        off += n


@pytest.mark.parametrize("name", DESC)
def test_numpy_descriptors_match_golden(name):
    g = _load(name)
    x = synth.tcm_layer3(int(g["seed"]), 1, 1024, int(g["H"]), int(g["W"]))
    w, b = synth.tcm_desc_conv(int(g["seed"]) + 1)
    out = tcm_np.get_descriptors(x, w, b, g["coords"][None])
    np.testing.assert_allclose(out, g["desc"], atol=2e-5 * np.abs(g["desc"]).max(), rtol=0)
    H, W = int(g["H"]), int(g["W"])
    if len(g["coords"]) > 1:       # first / last row and column of the (H+1) x (W+1) output map: the zero padding is exercised
        assert {(0, 0), (H, W)} <= set(map(tuple, g["coords"]))


@pytest.mark.parametrize("name", MATCH)
def test_numpy_matcher_matches_golden(name):
    g = _load(name)
    sd = synth.tcm_superglue_state(int(g["seed"]), 4, bool(g["skip_gnn"]))
    layers = [] if g["skip_gnn"] else ["self", "cross"] * 2
    Z, m0, m1, ms0, ms1 = tcm_np.match(sd, layers, int(g["iters"]), _match_data(g))
    np.testing.assert_allclose(Z, g["log_assignment"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(ms0, g["match_scores0"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(ms1, g["match_scores1"], atol=1e-5, rtol=0)
    assert min(float(g["margin_rows"]), float(g["margin_cols"]), float(g["margin_thr"])) > 1e-3, name   # well-conditioned
    np.testing.assert_array_equal(m0, g["matches0"])
    np.testing.assert_array_equal(m1, g["matches1"])


def test_numpy_matcher_pins_the_quirks():
    """Each of the head interleave, the (y, x) / (w, h) normalisation and the dustbin moves the answer: a restatement without it
    misses the golden."""
    g = _load("tcm_match_8x8")
    sd = synth.tcm_superglue_state(int(g["seed"]))
    d = _match_data(g)
    d_swapped = dict(d, img_coords0=d["img_coords0"][:, ::-1].copy(), img_coords1=d["img_coords1"][:, ::-1].copy())
    Z, *_ = tcm_np.match(sd, ["self", "cross"] * 2, 10, d_swapped)
    assert np.abs(Z - g["log_assignment"]).max() > 1e-2
    sd_bin = dict(sd, bin_score=np.array(float(sd["bin_score"]) + 0.5, np.float32))
    Z, *_ = tcm_np.match(sd_bin, ["self", "cross"] * 2, 10, d)
    assert np.abs(Z - g["log_assignment"]).max() > 1e-2


@pytest.fixture(scope="module")
def L():
    if _lib.needs_build():
        _lib.build_library()
    return _lib.lib()


def test_abi_argument_checks_do_not_launch(L):
    n = None
    one = ctypes.c_void_p(256)
    assert L.pt_tcm_peaks_f32(n, 1, 23, 23, 5, 0.1, one, one, one, n) == _lib.PT_ERR_NULL
    assert L.pt_tcm_peaks_f32(one, 1, 23, 23, 4, 0.1, one, one, one, n) == _lib.PT_ERR_UNSUPPORTED     # even ks
    assert L.pt_tcm_peaks_f32(one, 1, 23, 23, 0, 0.1, one, one, one, n) == _lib.PT_ERR_SHAPE
    assert L.pt_tcm_peaks_f32(one, 1, 65, 23, 5, 0.1, one, one, one, n) == _lib.PT_ERR_UNSUPPORTED     # map above 64x64
    ws = L.pt_tcm_desc_ws_bytes(1, 8, 1024, 256)
    assert ws == 64 * 8 * 256 * 4
    assert L.pt_tcm_desc_f32(one, n, one, one, 1, 1024, 22, 22, 8, 256, one, one, ws, n) == _lib.PT_ERR_NULL
    assert L.pt_tcm_desc_f32(one, one, one, one, 1, 1000, 22, 22, 8, 256, one, one, ws, n) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_tcm_desc_f32(one, one, one, one, 1, 1024, 22, 22, 8, 256, one, one, ws - 4, n) == _lib.PT_ERR_WORKSPACE
    nf = L.pt_tcm_match_weight_floats(4)
    assert nf == 109376 + 4 * 657152 + 65792

    def prm(M=8, N=8, layers=4, skip=0):
        return _lib.TcmMatchParams(M, N, layers, 0b1010, skip, 10, 0.2, (ctypes.c_float * 2)(320, 240), 448.0,
                                   (ctypes.c_float * 2)(320, 240), 448.0, nf)

    def call(p, w=one):
        return L.pt_tcm_match_f32(ctypes.byref(p), w, *([one] * 12), one, 1 << 30, n)

    assert call(prm(), w=n) == _lib.PT_ERR_NULL
    assert call(prm(M=65)) == _lib.PT_ERR_UNSUPPORTED
    assert call(prm(N=0)) == _lib.PT_ERR_SHAPE
    assert call(prm(layers=33)) == _lib.PT_ERR_UNSUPPORTED
    assert call(prm(layers=-1)) == _lib.PT_ERR_SHAPE
    assert call(prm(layers=5)) == _lib.PT_ERR_SHAPE                    # pack smaller than five layers need
    p = prm()
    assert L.pt_tcm_match_f32(ctypes.byref(p), one, *([one] * 12), one, L.pt_tcm_match_ws_bytes(ctypes.byref(p)) - 4, n) == \
        _lib.PT_ERR_WORKSPACE


@needs_ref
def test_pack_folds_batchnorm_like_the_module(L):
    ref_harness.install()
    from pytracking_amd import candidate_matching as CM
    g = _load("tcm_match_3x5")
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    sg = SuperGlue({'skip_gnn': False, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': 10,
                    'output_normalization': 'sinkhorn'})
    sg.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.tcm_superglue_state(int(g["seed"])).items()})
    sg.eval()
    pack = CM.pack_weights(sg).double()
    x = torch.randn(3, 7, dtype=torch.float64)
    with torch.no_grad():
        ref = sg.kenc.encoder.double()(x[None])[0]
    dims, off, h = [3, 32, 64, 128, 256, 256], 0, x
    for k in range(5):
        O, I = dims[k + 1], dims[k]
        w = pack[off:off + O * I].view(O, I)
        b = pack[off + O * I:off + O * I + O]
        off += O * I + O
        h = w @ h + b[:, None]
        if k < 4:
            h = h.clamp_min(0)
    torch.testing.assert_close(h, ref, atol=1e-5, rtol=1e-5)
    sg.float()
    # the pack is cached on the module state: an in-place update through an ordinary op makes a new pack
    p1 = CM.packed_weights(sg)
    assert CM.packed_weights(sg) is p1
    with torch.no_grad():
        sg.final_proj.bias.add_(1.0)
    p2 = CM.packed_weights(sg)
    assert p2 is not p1 and float((p2[-256:] - p1[-256:]).mean()) == pytest.approx(1.0)
    assert not any("pack" in k for k in sg.state_dict())


@needs_ref
def test_install_binds_and_uninstall_restores():
    ref_harness.install()
    import ltr.data.processing_utils as prutils
    from ltr.models.target_candidate_matching.target_candidate_matching import DescriptorExtractor
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    import pytracking.tracker.keep_track.keep_track as ktm
    from pytracking_amd import install as amd
    refs = (prutils.find_local_maxima, DescriptorExtractor.get_descriptors, SuperGlue._forward, ktm.KeepTrack.localize_advanced,
            ktm.KeepTrack.optimize_boxes_default, ktm.KeepTrack.optimize_boxes_relative, ktm.sample_patch_multiscale)
    amd.install()
    try:
        now = (prutils.find_local_maxima, DescriptorExtractor.get_descriptors, SuperGlue._forward, ktm.KeepTrack.localize_advanced,
               ktm.KeepTrack.optimize_boxes_default, ktm.KeepTrack.optimize_boxes_relative, ktm.sample_patch_multiscale)
        for a, b in zip(now, refs):
            assert a is not b and a.__wrapped__ is b
        # CPU tensors keep the reference's code and reproduce its golden
        g = _load("tcm_peaks_23")
        amd.stats.clear()
        c, v = prutils.find_local_maxima(torch.from_numpy(g["scores"]), th=float(g["th"]), ks=int(g["ks"]))
        assert amd.stats["find_local_maxima.reference"] == 1 and amd.stats["find_local_maxima.fast"] == 0
        np.testing.assert_array_equal(c.numpy(), g["coords"])
    finally:
        amd.uninstall()
    assert (prutils.find_local_maxima, DescriptorExtractor.get_descriptors, SuperGlue._forward, ktm.KeepTrack.localize_advanced,
            ktm.KeepTrack.optimize_boxes_default, ktm.KeepTrack.optimize_boxes_relative, ktm.sample_patch_multiscale) == refs


def _code_only(fn):
    """The AST of a method with docstrings removed (comments are not in the AST)."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
    for node in ast.walk(tree):
        body = getattr(node, "body", None)
        if isinstance(body, list) and body and isinstance(body[0], ast.Expr) and isinstance(getattr(body[0], "value", None), ast.Constant) \
                and isinstance(body[0].value.value, str):
            node.body = body[1:] or [ast.Pass()]
    return ast.dump(tree)


@needs_ref
@pytest.mark.parametrize("method", ["localize_advanced", "optimize_boxes_default", "optimize_boxes_relative"])
def test_keep_track_methods_are_dimps(method):
    ref_harness.install()
    from pytracking.tracker.dimp.dimp import DiMP
    from pytracking.tracker.keep_track.keep_track import KeepTrack
    assert _code_only(getattr(KeepTrack, method)) == _code_only(getattr(DiMP, method))


@needs_ref
def test_uncovered_matcher_confs_and_zero_keypoint_branch_fall_back():
    """bottleneck_dim, input_proj (input_dim != descriptor_dim), double_softmax, an uncovered layer type, training mode and the
    reference's zero-keypoint branch are not covered: install() hands them to the reference."""
    ref_harness.install()
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    from pytracking_amd import candidate_matching as CM
    base = {'skip_gnn': False, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': 10, 'output_normalization': 'sinkhorn'}
    assert CM._conf_covered(SuperGlue(base).eval())
    assert CM._conf_covered(SuperGlue(dict(base, skip_gnn=True)).eval())
    for extra in ({'bottleneck_dim': 64}, {'input_dim': 128}, {'output_normalization': 'double_softmax'}):
        sg = SuperGlue(dict(base, **extra)).eval()
        assert not CM._conf_covered(sg), extra
        assert not CM.covered_match(sg, {}), extra
    sg = SuperGlue(base)
    sg.conf = dict(sg.conf, GNN_layers=['self', 'other'])
    assert not CM._conf_covered(sg)
    assert not CM.covered_match(SuperGlue(base).train(), {})
    empty = {"img_coords0": torch.zeros(1, 0, 2), "img_coords1": torch.zeros(1, 3, 2)}
    assert CM.zero_keypoint_branch(empty) and not CM.covered_match(SuperGlue(base).eval(), empty)
    assert not CM.zero_keypoint_branch({"img_coords0": torch.zeros(5, 2), "img_coords1": torch.zeros(3, 2)})
