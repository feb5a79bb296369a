"""CPU side of the TaMOs heads (pt_tamos_bbreg_* / pt_fpn2_* of pytracking_amd/csrc/tomp.hip, FPN and DenseBoxRegressor of
pytracking_amd/tamos.py): the numpy restatement against the unmodified reference's recorded outputs, the seeded defects the float64 bound
has to catch, the refusals of the host-only queries, the pinned routes, the state_dict layouts and the install() flag.  No GPU.

The float64 anchor of the two deployed cases takes minutes in numpy, so their committed REF_ERR is not recomputed here; their float64
outputs are pinned by committed strides (tests/golden/tamos_heads_reg_deployed.npz is the reference's own run)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import tamos_heads_cases as HC
import f64_bound
import tamos_heads_f64 as F64
import tamos_heads_np as HN
from oracle import ref_harness
from pytracking_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("pt_tamos_bbreg_ws_bytes", "pt_tamos_bbreg_f32", "pt_tamos_bbreg_routes", "pt_fpn2_param_floats", "pt_fpn2_ws_bytes",
               "pt_fpn2_f32", "pt_fpn2_routes")
SMALL = HC.SMALL_REG + HC.SMALL_FPN + list(HC.CHAIN)


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"tamos_heads_{name}.npz"))


# ---- the restatement against the reference's recorded outputs ------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.SMALL_REG)
def test_restatement_matches_the_reference_golden(name):
    g = golden(name)
    a = F64.anchor(name)
    assert int(g["stride"]) == 1
    e64 = float(np.abs(a.want["ltrb"].reshape(-1) - g["ltrb_f64"]).max())
    e32 = float(np.abs(a.f32["ltrb"].reshape(-1).astype(np.float64) - g["ltrb_f64"]).max())
    ref32 = float(np.abs(g["ltrb_f32"].astype(np.float64) - g["ltrb_f64"]).max())
    print(f"\n{name}: float64 restatement vs reference float64 {e64:.3e}, fp32 restatement {e32:.3e}, reference fp32 vs its float64 {ref32:.3e}")
    assert e64 <= 1e-10 and e32 <= 1e-4 and e32 <= f64_bound.bound(HC.REF_ERR[name], F64.F) and ref32 <= 1e-4


def test_deployed_golden_is_a_stride_and_the_reference_is_close_to_its_own_float64():
    g = golden(HC.REG_DEPLOYED)
    n_img, T, D, H, W = HC.REG[HC.REG_DEPLOYED]
    k = HC.DEPLOYED_KEEP["ltrb"]
    assert int(g["stride"]) == k and g["ltrb_f64"].size == g["ltrb_f32"].size == -(-(n_img * T * 4 * H * W) // k)
    assert float(np.abs(g["ltrb_f32"].astype(np.float64) - g["ltrb_f64"]).max()) <= 1e-4           # the seed's own margin
    f = np.load(os.path.join(ROOT, "tests", "golden", "tamos_heads_fpn_deployed.npz"))
    n, _, _, Dp, H3, W3, H2, W2 = HC.FPN[HC.FPN_DEPLOYED]
    assert f["feat2_f64"].size == -(-(n * Dp * H2 * W2) // int(f["feat2_stride"])) and f["feat3_f64"].size == -(-(n * Dp * H3 * W3) // int(f["feat3_stride"]))
    for path in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if path.startswith("tamos_heads_"):
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", path)) < (1 << 20), path


def test_golden_keys_are_the_mirror_state_dict_keys():
    from pytracking_amd import tamos as TA
    for name in HC.SMALL_REG[:2]:
        D = HC.REG[name][2]
        assert list(golden(name)["keys"]) == list(TA.DenseBoxRegressor(num_channels=D).state_dict().keys())


@pytest.mark.parametrize("name", SMALL)
def test_ref_err_is_inside_the_band_of_the_committed_value(name):
    r = F64.anchor(name).ref_err
    lo, hi = F64.REF_ERR_BAND
    print(f"\n{name}: ref_err {r:.3e}, committed {HC.REF_ERR[name]:.3e}")
    assert lo * HC.REF_ERR[name] <= r <= hi * HC.REF_ERR[name]


def test_every_case_has_routes_and_ref_err():
    assert set(HC.ROUTES) == set(HC.REG) | set(HC.FPN) and set(HC.REF_ERR) == set(HC.REG) | set(HC.FPN) | set(HC.CHAIN)
    for name, (n_img, T, D, H, W) in HC.REG.items():
        _, _, filt = HC.reg_case(name) if name != HC.REG_DEPLOYED else (None, None, None)
        if filt is not None:
            for o in range(T):
                assert (not filt[:, o].any()) == (T >= 3 and o == T // 2)


# ---- the seeded defects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", HN.DEFECTS)
def test_seeded_defect_fails_the_bound(defect):
    """Each defect, run in fp32 like the kernel, must exceed F_MAX x ref_err on at least one small case (it does on every one)."""
    over = []
    for name in F64.DEFECT_CASES[defect]:
        e = max(f64_bound.errors(F64.anchor(name).want, F64.outputs(name, np.float32, defect)).values())
        print(f"\ndefect {defect} on {name}: {e:.3e} = {e / HC.REF_ERR[name]:.1f} x ref_err")
        over.append(e > F64.F_MAX * HC.REF_ERR[name])
    assert any(over) and F64.F <= F64.F_MAX


def test_nearest_index_is_floor_of_the_fp32_product():
    assert list(HN.nearest_index(10, 5)) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert list(HN.nearest_index(9, 5)) == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    assert list(HN.nearest_index(13, 7)) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    t = torch.arange(7, dtype=torch.float32).reshape(1, 1, 1, 7)
    assert list(torch.nn.functional.interpolate(t, size=(1, 13), mode="nearest").reshape(-1).long().numpy()) == list(HN.nearest_index(13, 7))


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared(L):
    hdr = open(os.path.join(ROOT, "include", "pt_hot.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(L, name)
    body = hdr[hdr.index("enum pt_heads_route {"):]
    body = body[:body.index("};")]
    names = re.findall(r"PT_HEADS_R_(\w+)", body)
    assert names[-1] == "END" and tuple("HEADS_" + n for n in names[:-1]) == _lib.HEADS_ROUTES
    assert int(re.search(r"PT_HEADS_R_NCHW_TOKENS = (\d+)", body).group(1)) == _lib.HEADS_ROUTE_BASE == 2000


def test_workspace_queries_refuse(L):
    assert L.pt_tamos_bbreg_ws_bytes(1, 10, 256, 48, 72) > 0 and L.pt_tamos_bbreg_ws_bytes(2, 16, 512, 1, 1) > 0
    for args in ((1, 0, 64, 5, 7), (1, 17, 64, 5, 7), (1, 3, 96, 5, 7), (1, 3, 576, 5, 7), (0, 3, 64, 5, 7), (1, 3, 64, 0, 7), (1, 3, 64, 5, -1),
                 (1, 3, 0, 5, 7), (-1, 3, 64, 5, 7), (1, 16, 512, 4096, 4096), (70000, 1, 64, 1, 1)):
        assert L.pt_tamos_bbreg_ws_bytes(*args) == 0, args
        rc, r = HC.reg_routes(L, *args)
        assert rc in (_lib.PT_ERR_SHAPE, _lib.PT_ERR_UNSUPPORTED) and r == (), args
    assert L.pt_fpn2_ws_bytes(1, 512, 256, 256, 48, 72, 24, 36) > 0 and L.pt_fpn2_param_floats(512, 256, 256) > 0
    for args in ((1, 96, 64, 64, 10, 14, 5, 7), (1, 128, 96, 64, 10, 14, 5, 7), (1, 128, 64, 96, 10, 14, 5, 7), (1, 128, 64, 576, 10, 14, 5, 7),
                 (0, 128, 64, 64, 10, 14, 5, 7), (1, 128, 64, 64, 0, 14, 5, 7), (1, 128, 64, 64, 10, 14, 5, 0), (1, 128, 64, 64, 10, -3, 5, 7),
                 (1, 0, 64, 64, 10, 14, 5, 7)):
        assert L.pt_fpn2_ws_bytes(*args) == 0, args
        n, C_hi, C_lo, D, H2, W2, H3, W3 = args
        rc, r = HC.fpn_routes(L, n, C_hi, C_lo, D, H3, W3, H2, W2)
        assert rc in (_lib.PT_ERR_SHAPE, _lib.PT_ERR_UNSUPPORTED) and r == (), args
    for args in ((96, 64, 64), (128, 64, 576), (0, 64, 64), (128, 64, 0)):
        assert L.pt_fpn2_param_floats(*args) == 0, args


def test_entry_points_refuse_before_any_launch(L):
    """NULL arguments and refused shapes come back before a stream is touched (this machine has no device to launch on)."""
    one = ctypes.c_void_p(256)
    assert L.pt_tamos_bbreg_f32(None, one, one, one, 1, 3, 64, 5, 7, one, 1 << 30, None) == _lib.PT_ERR_NULL
    assert L.pt_tamos_bbreg_f32(one, one, one, one, 1, 17, 64, 5, 7, one, 1 << 30, None) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_tamos_bbreg_f32(one, one, one, one, 1, 0, 64, 5, 7, one, 1 << 30, None) == _lib.PT_ERR_SHAPE
    assert L.pt_tamos_bbreg_f32(one, one, one, one, 1, 3, 64, 5, 7, one, 16, None) == _lib.PT_ERR_WORKSPACE
    assert L.pt_fpn2_f32(one, one, one, one, None, 1, 128, 64, 64, 10, 14, 5, 7, 1, one, 1 << 30, None) == _lib.PT_ERR_NULL
    assert L.pt_fpn2_f32(one, one, one, one, None, 1, 96, 64, 64, 10, 14, 5, 7, 0, one, 1 << 30, None) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_fpn2_f32(one, one, one, one, None, 1, 128, 64, 64, 10, 14, 5, 7, 0, one, 16, None) == _lib.PT_ERR_WORKSPACE


def test_pinned_routes_and_coverage(L):
    seen = set()
    for name in list(HC.REG) + list(HC.FPN):
        assert HC.case_routes(L, name) == (0, HC.ROUTES[name]), name
        seen |= set(HC.ROUTES[name])
    assert len(_lib.HEADS_ROUTES) == 7 and set(_lib.HEADS_ROUTES) <= seen    # every loader mode of launch_conv3, every new launch
    # without feat3 the plain convolution is not queued
    rc, r = HC.fpn_routes(L, *HC.FPN["fpn_x2"], want_feat3=0)
    assert rc == 0 and r == HC.ROUTES["fpn_x2"][:-1] and HC.ROUTES["fpn_x2"][-1] == "HEADS_CONV3_PLAIN"
    # existing ids keep their numbers: the new ones have an enum of their own
    assert len(_lib.TAMOS_ROUTES) == 8 and len(_lib.TOMP_ROUTES) == 41


# ---- the Python mirror ------------------------------------------------------------------------------------------------------------
def test_state_dicts_load_strict_in_both_fpn_layouts():
    from pytracking_amd import tamos as TA
    params, _, _ = HC.reg_case("reg_d64_5x7_t3")
    reg = TA.DenseBoxRegressor(num_channels=64)
    reg.load_state_dict(HC.to_sd(params), strict=True)
    fparams, _, _ = HC.fpn_case("fpn_x2")
    m = TA.FPN(output_dim=64, input_dims=(128, 64))
    assert list(m.state_dict().keys()) == [f"fpn.{b}.{i}.0.{t}" for b in ("inner_blocks", "layer_blocks") for i in (0, 1) for t in ("weight", "bias")]
    m.load_state_dict(HC.to_sd(fparams), strict=True)
    old = {k.replace(".0.weight", ".weight").replace(".0.bias", ".bias"): v for k, v in HC.to_sd(fparams).items()}
    assert "fpn.inner_blocks.0.weight" in old and "fpn.layer_blocks.1.bias" in old
    m2 = TA.FPN(output_dim=64, input_dims=(128, 64))
    m2.load_state_dict(old, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]) and torch.equal(v, torch.from_numpy(fparams[k].copy())), k
    with pytest.raises(RuntimeError):
        m2.load_state_dict({**old, "fpn.extra": torch.zeros(1)}, strict=True)


def test_mirror_refuses_cpu_tensors_and_training_without_a_fallback():
    from pytracking_amd import tamos as TA
    reg = TA.DenseBoxRegressor(num_channels=64).eval()
    with pytest.raises(NotImplementedError):
        reg(torch.zeros(1, 1, 64, 5, 7), torch.zeros(1, 3, 64, 1, 1))
    with pytest.raises(NotImplementedError):
        reg.train()(torch.zeros(1, 1, 64, 5, 7), torch.zeros(1, 3, 64, 1, 1))
    m = TA.FPN(output_dim=64, input_dims=(128, 64)).eval()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 64, 5, 7), {"layer2": torch.zeros(1, 128, 10, 14)})
    with pytest.raises(NotImplementedError):
        m.train()(torch.zeros(1, 1, 64, 5, 7), {"layer2": torch.zeros(1, 128, 10, 14)})
    with pytest.raises(NotImplementedError):
        TA.FPN(output_dim=64, input_dims=(128, 64, 32))


# ---- install(tamos=True) ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
def test_install_flag_rebinds_the_two_heads_and_uninstall_restores_them():
    ref_harness.install()
    import ltr.models.transformer.heads as rh
    from pytracking_amd import install as amd, tamos as TA, transformer as TM
    orig_reg, orig_fpn = rh.DenseBoxRegressor, rh.FPN
    ref_keys = list(orig_reg(num_channels=64).state_dict().keys())
    amd.install()                                              # the default set: the single-filter regressor, FPN untouched
    try:
        assert rh.FPN is orig_fpn
        assert type(rh.DenseBoxRegressor(num_channels=64)) is TM.DenseBoxRegressor
    finally:
        amd.uninstall()
    assert rh.DenseBoxRegressor is orig_reg and rh.FPN is orig_fpn
    amd.install(tamos=True)
    try:
        assert rh.DenseBoxRegressor is not orig_reg and issubclass(rh.DenseBoxRegressor, orig_reg) and rh.DenseBoxRegressor.__name__ == "DenseBoxRegressor"
        assert rh.FPN is not orig_fpn and issubclass(rh.FPN, orig_fpn) and rh.FPN.__name__ == "FPN"
        mine = rh.DenseBoxRegressor(num_channels=64)
        assert type(mine) is TA.DenseBoxRegressor and list(mine.state_dict().keys()) == ref_keys
        other = rh.DenseBoxRegressor(num_channels=48)
        assert isinstance(other, orig_reg) and not isinstance(other, TM.DenseBoxRegressor)
        f = rh.FPN(high_res_layer="layer2", output_dim=64, input_dims=(128, 64))
        assert type(f) is TA.FPN and f.high_res_layer == "layer2"
        assert type(rh.FPN()) is TA.FPN                        # the reference's defaults: (512, 256) -> 256
    finally:
        amd.uninstall()
    assert rh.DenseBoxRegressor is orig_reg and rh.FPN is orig_fpn


@pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
def test_default_install_rebinds_what_it_did():
    import test_install_ledger as TL
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install()
    amd.uninstall()
    before = TL.snapshot()
    amd.install()
    try:
        got = TL.changed(before, TL.snapshot())
    finally:
        amd.uninstall()
    # attribute rebindings only: which modules install() has to create depends on what earlier tests of the session left in sys.modules
    # (tests/test_install_ledger.py pins the whole list from its own clean start)
    attrs = lambda names: [n for n in names if not n.startswith("sys.modules[")]
    with open(TL.REBOUND) as fh:
        assert attrs(got) == attrs(json.load(fh))
    assert TL.changed(before, TL.snapshot()) == []
