"""KeepTrack target-candidate matching (pytracking_amd.candidate_matching, tcm.hip) without a GPU: the goldens of the unmodified
reference (tools/make_golden_keep_track.py) agree with the float64 restatement (tests/tcm_np.py), the weight pack folds the eval
BatchNorms exactly as the module computes, the C ABI refuses bad arguments before any launch, install() binds and uninstall()
restores the new names, and KeepTrack's localisation / box refinement methods are DiMP's in code.  On the cases off the deployed shapes
(tests/tcm_cases.py, run on the device by tests/test_gpu_keep_track_f64.py) the restatement agrees with the reference's own SuperGlue and
with torch's conv2d in float64, every matcher case is well-conditioned, and a restatement with the mistake a case is there for (side 1
normalised with side 0's image size, the layer list reversed, H and W swapped, the batch index dropped, one Sinkhorn iteration too few)
leaves that case's bound."""
import ast
import ctypes
import inspect
import os
import textwrap

import numpy as np
import pytest
import torch

import f64_bound
import tcm_cases as TC
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


# ---------------------------------------------------------------------------------------------------------------------------
# The cases off the deployed shapes (tests/tcm_cases.py): the float64 anchor is right on them, each has its ref_err, and a restatement
# with the mistake a case is there for leaves that case's bound.  Every test prints its figures before it asserts (run with -s).

@pytest.mark.parametrize("name", list(TC.PEAK_CASES))
def test_peak_cases_reach_the_paths_they_are_there_for(name):
    H, W, ks, th, _, _ = TC.PEAK_CASES[name]
    maps = TC.peak_map(name)
    assert maps.dtype == np.float32 and maps.shape[-2:] == (H, W)
    want = TC.peak_want(name)
    for c, v in want:
        idx = c[:, 0] * W + c[:, 1]
        assert len(set(idx.tolist())) == len(idx) and np.all(v[:-1] >= v[1:])
        assert all(i0 < i1 for i0, i1, a, b in zip(idx[:-1], idx[1:], v[:-1], v[1:]) if a == b)      # ties in ascending raster order
    c, v = want[0]
    idx = c[:, 0] * W + c[:, 1]
    print(f"\npeaks {name}: {[len(c) for c, _ in want]} hits, {sorted(set((idx // 1024).tolist()))} compaction passes with a hit")
    if name in ("33x33", "64x64", "64x64_ks1", "40x50_eighths"):           # a hit in every pass: `base` is carried into each
        assert set((idx // 1024).tolist()) == set(range((H * W + 1023) // 1024))
    if name == "64x64_ks1":
        assert len(c) > 1024 and len(c) == int((maps > np.float32(th)).sum())
    if name == "64x64_ks127":
        assert [tuple(r) for r in c] == list(TC.TWO_MAXIMA) and v.tolist() == [2.0, 2.0]
    if name == "1x1":
        assert len(c) == 1
    if name == "40x50_eighths":
        assert len(np.unique(v)) < len(v) / 8                                  # many exact ties
    if name == "23x23_nonfinite":
        assert tuple(c[0]) == TC.NONFINITE["+inf"] and np.isinf(v[0]) and np.isfinite(v[1:]).all()
        ny, nx = TC.NONFINITE["nan"]
        assert not any(abs(y - ny) <= ks // 2 and abs(x - nx) <= ks // 2 for y, x in c)    # a NaN in the window: no peak there
        assert np.isnan(maps).sum() == 1 and (maps == -np.inf).sum() == 1
    if name == "40x50_batch3":
        assert len(want) == 3 and all(len(c) > 0 for c, _ in want)
        assert len({tuple(map(tuple, c)) for c, _ in want}) == 3


@pytest.mark.parametrize("name", list(TC.DESC_CASES))
def test_numpy_descriptors_match_conv2d_in_float64(name):
    B, C, H, W, D, P, form, _ = TC.DESC_CASES[name]
    i, a = TC.desc_inputs(name), TC.desc_anchor(name)
    assert i.x.shape == (B, C, H, W) and i.weight.shape == (D, C, 4, 4) and i.coords3.shape == (B, P, 2)
    assert i.coords.shape == ((B, P, 2) if form == "per_image" else (P, 2)) and i.coords.dtype == (np.int32 if form == "int32" else np.int64)
    if P > 4:
        for b in range(B):
            assert {(0, 0), (0, W), (H, 0), (H, W)} <= set(map(tuple, i.coords3[b]))
    f64 = TC.conv2d_at_points(i.x, i.weight, i.bias, i.coords3, torch.float64)
    err = float(np.abs(f64 - a.want).max())
    print(f"\ndesc {name}: max |numpy - conv2d float64| {err:.3e}, ref_err {a.ref_err:.3e}, bound {f64_bound.bound(a.ref_err):.3e}")
    assert a.want.shape == (B, D, P) and err <= 1e-9
    assert 0 < a.ref_err < 1e-5                                                # fp32 rounding of sums of C * 16 terms of order 1


@pytest.mark.parametrize("name", list(TC.MATCH))
def test_matcher_cases_are_well_conditioned(name):
    """The discrete outputs are compared exactly on the device: every row's and column's maximum is 1e-3 ahead of its runner-up and every
    match score 1e-3 away from the filter threshold, in float64."""
    M, N = TC.MATCH[name][1:3]
    w = TC.match_want(name)
    rows, cols, thr = tcm_np.margins(w["log_assignment"], w["match_scores0"])
    print(f"\nmatch {name}: margins rows {rows:.3g}, columns {cols:.3g}, threshold {thr:.3g}")
    assert w["log_assignment"].shape == (M + 1, N + 1) and min(rows, cols, thr) > 1e-3


@needs_ref
@pytest.mark.parametrize("name", list(TC.MATCH))
def test_numpy_matcher_matches_the_reference_in_float64(name):
    w, a = TC.match_want(name), TC.match_anchor(name)
    r64 = TC.reference_match(name, torch.float64)
    err = float(np.abs(r64["log_assignment"] - w["log_assignment"]).max())
    print(f"\nmatch {name}: max |numpy - reference float64| {err:.3e}, ref_err {a.ref_err:.3e}, bound {f64_bound.bound(a.ref_err):.3e}")
    assert r64["log_assignment"].dtype == np.float64 and err <= 1e-9
    np.testing.assert_array_equal(r64["matches0"], w["matches0"])
    np.testing.assert_array_equal(r64["matches1"], w["matches1"])
    # exp(z) of an agreeing z: relative where the score exceeds 1 (without a Sinkhorn iteration Z is not normalised: `it0` reaches 1e13)
    np.testing.assert_allclose(r64["match_scores0"], w["match_scores0"], atol=1e-9, rtol=1e-9)
    np.testing.assert_allclose(r64["match_scores1"], w["match_scores1"], atol=1e-9, rtol=1e-9)
    assert 0 < a.ref_err < 1e-4                                                # under the flat tolerance of the golden tests


def _desc_mutant(name, swap_hw=False, drop_batch=False):
    """tcm_np.get_descriptors with the map indexed as (W, H) (bounds and row stride), or with every image read as image 0."""
    i = TC.desc_inputs(name)
    B, C, H, W = i.x.shape
    flat = i.x.astype(np.float64).reshape(B, C, H * W)
    w = i.weight.astype(np.float64)
    h_, w_ = (W, H) if swap_hw else (H, W)
    out = np.empty((B, w.shape[0], i.coords3.shape[1]))
    for b in range(B):
        for p, (y, x) in enumerate(i.coords3[b]):
            patch = np.zeros((C, 4, 4))
            for u in range(4):
                for v in range(4):
                    yy, xx = y + u - 2, x + v - 2
                    if 0 <= yy < h_ and 0 <= xx < w_:
                        patch[:, u, v] = flat[0 if drop_batch else b, :, yy * w_ + xx]
            out[b, :, p] = w.reshape(w.shape[0], -1) @ patch.reshape(-1) + i.bias
    return out


def test_desc_mutant_helper_is_the_anchor_without_a_mutation():
    for name in ("h9_w30", "b2_per_image"):
        assert np.abs(_desc_mutant(name) - TC.desc_anchor(name).want).max() <= 1e-12


@pytest.mark.parametrize("name,mutation", [("h9_w30", "swap_hw"), ("h30_w9", "swap_hw"), ("b2_per_image", "drop_batch"),
                                           ("b3_shared", "drop_batch")])
def test_the_descriptor_bound_catches_the_mutant(name, mutation):
    a = TC.desc_anchor(name)
    diff = np.abs(_desc_mutant(name, **{mutation: True}) - a.want)
    print(f"\ndesc {name}, mutant {mutation}: max |mutant - float64| {diff.max():.3e}, bound {f64_bound.bound(a.ref_err):.3e}")
    assert diff.max() > f64_bound.bound(a.ref_err)
    if mutation == "drop_batch":                                               # image 0 is right, every later image is not
        assert diff[0].max() == 0 and all(diff[b].max() > f64_bound.bound(a.ref_err) for b in range(1, diff.shape[0]))


@pytest.mark.parametrize("name", ["9x64", "64x9"])
def test_the_peak_comparison_catches_a_swapped_raster_index(name):
    H, W = TC.PEAK_CASES[name][:2]
    c, _ = TC.peak_want(name)[0]
    idx = c[:, 0] * W + c[:, 1]
    mutant = np.stack([idx // H, idx % H], 1)                                  # y = i / H, x = i % H
    assert not np.array_equal(mutant, c)


@needs_ref
@pytest.mark.parametrize("name,mutation", [("sizes", "side0_size"), ("ssc", "reversed"), ("css5", "reversed"), ("it1", "one_fewer")])
def test_the_matcher_bound_catches_the_mutant(name, mutation):
    """The float64 anchor with one mistake: side 1 normalised with side 0's image size, the layer list reversed (the weights stay in
    place), one Sinkhorn iteration too few.  The case made for the mistake leaves its bound and changes its discrete outputs."""
    sd, layers, iters, data = TC.match_inputs(name)
    a = TC.match_anchor(name)
    if mutation == "side0_size":
        data = dict(data, image_size1=data["image_size0"])
    elif mutation == "reversed":
        layers = layers[::-1]
        assert layers != TC.match_inputs(name)[1]
    else:
        iters -= 1
    Z, m0, m1, ms0, ms1 = tcm_np.match(sd, layers, iters, data)
    diff = float(np.abs(Z - a.want["log_assignment"]).max())
    discrete = (not np.array_equal(m0, a.want["matches0"]) or not np.array_equal(m1, a.want["matches1"])
                or not np.array_equal(ms0 == 0, a.want["match_scores0"] == 0))
    print(f"\nmatch {name}, mutant {mutation}: max |mutant - float64| {diff:.3e}, bound {f64_bound.bound(a.ref_err):.3e}, "
          f"discrete outputs differ: {discrete}")
    assert diff > f64_bound.bound(a.ref_err)
    assert discrete
