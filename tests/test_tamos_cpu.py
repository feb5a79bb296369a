"""CPU checks of the TaMOs multi-object filter predictor (tests/tamos_cases.py, tests/tamos_np.py, tests/tamos_f64.py), no GPU:

* the float64 restatement equals the float64 output of the reference's own GOTFilterPredictor + LinearFilterClassifier
  (tests/golden/tamos_*.npz, tools/make_golden_tamos.py) within 1e-9, and the fp32 restatement stays within 4 x the golden's own
  fp32-vs-float64 distance; ref_err lies within [0.5, 2] x the committed value;
* the exports are declared in the header, refuse what the header says they refuse, and size the pack as the mirror packs it;
* every case lands on its pinned routes, and every id the routes query returns on the covered grid is hit by a case;
* install(tamos=True) chooses the mirror exactly for the covered constructor calls, uninstall restores, the default set is unchanged;
* the bound F x ref_err has teeth: five seeded defects of the fp32 restatement leave it on every case they reach."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tamos_cases as TC
import f64_bound
import tamos_f64 as F64
import tamos_np as TN
from f64_bound import FACTOR
from oracle import ref_harness
from pytracking_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(TC.CASES)
NEW_EXPORTS = ("pt_tamos_param_floats", "pt_tamos_prepared_floats", "pt_tamos_prepare_f32", "pt_tamos_predict_ws_bytes",
               "pt_tamos_predict_f32", "pt_tamos_predict_routes")


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"tamos_{name}.npz"))


def _strided(g, q, v):
    return v.reshape(-1)[::int(g[f"{q}_stride"])] if q.endswith("enc") else v


# ---- the restatement against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    g = golden(name)
    a = F64.anchor(name)
    assert set(a.want) == {k[:-4] for k in g.files if k.endswith("_f64")}
    for q, w in a.want.items():
        ref64, ref32 = g[f"{q}_f64"], g[f"{q}_f32"]
        assert ref64.dtype == np.float64 and ref32.dtype == np.float32
        d64 = float(np.abs(_strided(g, q, w).reshape(ref64.shape) - ref64).max())
        own = float(np.abs(ref32.astype(np.float64) - ref64).max())                      # the reference's own fp32 error on this output
        d32 = float(np.abs(_strided(g, q, a.f32[q]).reshape(ref64.shape).astype(np.float64) - ref64).max())
        print(f"\n{name} {q}: |f64 restatement - f64 reference| {d64:.3e}; fp32 restatement {d32:.3e} vs reference fp32 {own:.3e}")
        assert d64 <= 1e-9
        assert d32 <= 4 * own


@pytest.mark.parametrize("name", CASES)
def test_ref_err_is_the_committed_one(name):
    a = F64.anchor(name)
    assert list(a.ref_err) == list(TC.REF_ERR[name]) == ["predictor", "scores"]
    print(f64_bound.report(f"{name} (fp32 restatement)", a.ref_errs, TC.REF_ERR[name], F64.F, group=F64.group))
    for grp, r in a.ref_err.items():
        assert F64.REF_ERR_BAND[0] * TC.REF_ERR[name][grp] <= r <= F64.REF_ERR_BAND[1] * TC.REF_ERR[name][grp], (grp, r)
    assert f64_bound.within(a.ref_errs, TC.REF_ERR[name], F64.F, group=F64.group)


def test_factor():
    assert FACTOR <= F64.F <= F64.F_MAX == 8 and F64.bound(1.0) == F64.F


def test_cases_are_what_the_table_says():
    C = TC.CASES
    assert set(C) == set(TC.ROUTES) == set(TC.REF_ERR)
    for text in TC.ROUTES_TEXT.values():
        assert TC.compress(TC.expand(text)) == text
    keys = lambda c: (c["n_train"] + 1) * c["H"] * c["W"]
    assert keys(C["base_t3"]) == 105 and [C[f"base_t{t}"]["T"] for t in (1, 3, 10, 11, 16)] == [1, 3, 10, 11, 16]
    assert (C["base_t11"]["T"] * C["base_t11"]["nhead"]) % 16 != 0 and (C["base_t16"]["T"] * C["base_t16"]["nhead"]) % 16 == 0
    assert [C[f"mask9_gth{g}"]["num_gth_frames"] for g in (0, 1, 2)] == [0, 1, 2] and 2 * 81 > 128
    assert C["keys1444"]["nhead"] * (keys(C["keys1444"]) + 4) > 11000 and keys(C["keys1444"]) == 1444         # past pt_tomp's limit
    assert keys(C["head16_keys1452"]) == 1452 and C["head16_keys1452"]["D"] // C["head16_keys1452"]["nhead"] == 16
    assert C["head64_seq3"]["D"] // C["head64_seq3"]["nhead"] == 64 and C["head64_seq3"]["n_seq"] == 3
    assert [C[n]["n_seq"] for n in ("seq1", "seq2", "seq8")] == [1, 2, 8] and all(C[n]["n_train"] == 1 for n in ("seq1", "seq2", "seq8"))
    assert C["dec1"]["n_dec"] == 1 and (C["enc0_dec2"]["n_enc"], C["enc0_dec2"]["n_dec"]) == (0, 2)
    d = C["deployed"]
    assert (d["D"], d["nhead"], d["ff"], d["n_enc"], d["n_dec"], d["H"], d["W"], d["T"], d["n_train"]) == (256, 8, 2048, 6, 6, 24, 36, 10, 2)
    for name, c in C.items():                                   # a middle object is absent wherever there are three
        _, _, (_, _, lab, ltrb) = TC.case(name)
        for o in range(c["T"]):
            absent = o in TC.absent_objects(c["T"])
            assert (not lab[:, :, o].any() and not ltrb[:, :, o].any()) == absent
        assert c["T"] < 3 or 0 < TC.absent_objects(c["T"])[0] < c["T"] - 1


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared(L):
    hdr = open(os.path.join(ROOT, "include", "pt_hot.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(L, name)
    body = hdr[hdr.index("enum pt_tamos_route {"):]
    body = body[:body.index("};")]
    names = re.findall(r"PT_TAMOS_R_(\w+)", body)
    assert names[-1] == "END" and tuple("TAMOS_" + n for n in names[:-1]) == _lib.TAMOS_ROUTES
    assert int(re.search(r"PT_TAMOS_R_TOKENS = (\d+)", body).group(1)) == _lib.TAMOS_ROUTE_BASE == 1000
    assert int(re.search(r"#define PT_TAMOS_MAX_ROUTES (\d+)", hdr).group(1)) == _lib.PT_TAMOS_MAX_ROUTES
    # pt_tomp's enum and its limits have not moved
    assert _lib.TOMP_ROUTES[-1] == "REG_FINISH" and len(_lib.TOMP_ROUTES) == 41


def _d(D=256, nhead=8, ff=256, n_enc=1, n_dec=1, H=5, W=5):
    return _lib.TompDims(D, nhead, ff, n_enc, n_dec, H, W, max(H, W))


def test_refusals(L):
    ws = lambda d, T, nt, ns, par: L.pt_tamos_predict_ws_bytes(ctypes.byref(d), T, nt, ns, par)
    rq = lambda d, T, nt, ns, par: TC.query(L, d, T, nt, ns, par)[0]
    d = _d()
    U, S = _lib.PT_ERR_UNSUPPORTED, _lib.PT_ERR_SHAPE
    for args, rc in (((d, 1, 1, 1, 0), 0), ((d, 16, 1, 8, 0), 0), ((d, 10, 2, 1, 1), 0),
                     ((d, 0, 1, 1, 0), U), ((d, 17, 1, 1, 0), U), ((_d(nhead=32), 3, 1, 1, 0), U),          # head width 8
                     ((d, 3, 1, 9, 0), U), ((d, 3, 1, 2, 1), U), ((d, 3, 0, 1, 0), S), ((d, 3, 1, 0, 0), S),
                     ((_d(D=192, nhead=6), 3, 1, 1, 0), U), ((_d(ff=100), 3, 1, 1, 0), U), ((_d(n_dec=17), 3, 1, 1, 0), U)):
        assert (ws(*args) > 0) == (rc == 0), args[1:]
        assert rq(*args) == rc, args[1:]
    for T in (0, 17):
        assert L.pt_tamos_param_floats(ctypes.byref(d), T) == 0 and L.pt_tamos_prepared_floats(ctypes.byref(d), T) == 0
        assert L.pt_tamos_prepare_f32(ctypes.byref(d), T, 256, 256, None) == U
    assert L.pt_tamos_param_floats(ctypes.byref(_d(nhead=32)), 3) == 0
    # the entry point itself, before any launch: null arguments, then the same refusals, then the workspace
    f = lambda d, T, nt, ns, par, gth, ws_bytes=1 << 40, p=256: L.pt_tamos_predict_f32(
        ctypes.byref(d), T, p, 256, 256, 256, 256, 256, 256, nt, ns, par, gth, 256, 256, 256, ws_bytes, None)
    assert f(d, 3, 1, 1, 0, 0, p=None) == _lib.PT_ERR_NULL
    assert f(d, 17, 1, 1, 0, 0) == U and f(d, 3, 1, 9, 0, 0) == U and f(d, 3, 1, 2, 1, 0) == U and f(_d(nhead=32), 3, 1, 1, 0, 0) == U
    assert f(d, 3, 0, 1, 0, 0) == S and f(d, 3, 2, 1, 1, 3) == S and f(d, 3, 2, 1, 1, -1) == S
    assert f(d, 3, 1, 1, 0, 0, ws_bytes=ws(d, 3, 1, 1, 0) - 1) == _lib.PT_ERR_WORKSPACE
    # a memory long enough to push a buffer past the 32-bit byte offsets is refused, not truncated
    big = _lib.TompDims(512, 8, 2048, 1, 1, 400, 400, 400)
    assert ws(big, 16, 3, 1, 0) == 0 and rq(big, 16, 3, 1, 0) == U
    # pt_tomp's own limit is where it was
    dk = _d(H=19, W=19)
    assert L.pt_tomp_predict_ws_bytes(ctypes.byref(dk), 3, 1, 1) == 0 and ws(dk, 10, 3, 1, 1) > 0


@pytest.mark.parametrize("name", CASES)
def test_case_sizes_and_pinned_routes(L, name):
    cfg, params, _ = TC.case(name)
    d = TC.dims(cfg)
    pred, _ = TC.build_modules(cfg, params, "cpu")
    assert L.pt_tamos_param_floats(ctypes.byref(d), cfg["T"]) == sum(t.numel() for t in pred.pack_list())
    assert L.pt_tamos_prepared_floats(ctypes.byref(d), cfg["T"]) > 0
    assert L.pt_tamos_predict_ws_bytes(ctypes.byref(d), cfg["T"], cfg["n_train"], cfg["n_seq"], int(cfg["mode"] == "parallel")) > 0
    assert 0 <= cfg["num_gth_frames"] <= cfg["n_train"]
    rc, r = TC.case_routes(L, name)
    assert rc == 0 and r == TC.ROUTES[name], (rc, TC.compress(r))


def test_mirror_keeps_the_reference_state_dict_keys():
    for name in ("base_t3", "deployed"):
        cfg, params, _ = TC.case(name)
        pred, _ = TC.build_modules(cfg, params, "cpu")
        assert list(pred.state_dict().keys()) == list(golden(name)["state_dict_keys"])


def test_every_reachable_route_is_hit_by_a_case(L):
    """Every id pt_tamos_predict_routes returns anywhere on the covered grid is on some case's pinned list."""
    seen, calls = set(), 0
    maps = [(h, h) for h in (1, 2, 3, 5, 8, 9, 11, 16, 18, 19, 22, 23, 32)] + [(5, 7), (7, 19), (24, 36)]
    heads = {128: (2, 4, 8), 256: (4, 8, 16), 384: (6, 12), 512: (8, 16)}
    for D, nheads in heads.items():
        for nhead in nheads:
            for H, W in maps:
                for n_train in (1, 2, 3):
                    for n_seq, par in ((1, 1), (1, 0), (2, 0), (3, 0), (8, 0)):
                        for T in (1, 3, 10, 11, 16):
                            for ff in (256, 320, 512, 768, 1024, 2048):
                                for n_enc, n_dec in ((1, 2),) if ff != 256 else ((1, 2), (0, 2), (2, 1), (6, 6)):
                                    d = _lib.TompDims(D, nhead, ff, n_enc, n_dec, H, W, max(H, W))
                                    rc, r = TC.query(L, d, T, n_train, n_seq, par)
                                    assert rc == 0 and L.pt_tamos_predict_ws_bytes(ctypes.byref(d), T, n_train, n_seq, par) > 0
                                    seen.update(r)
                                    calls += 1
    assert calls > 50000
    hit = set().union(*TC.ROUTES.values())
    assert hit <= seen
    assert seen - hit == set(), sorted(seen - hit)
    assert set(_lib.TAMOS_ROUTES) <= hit                       # every launch that is new here


# ---- install ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
def test_install_flag_chooses_the_mirror_for_covered_calls_only():
    ref_harness.install()
    import ltr.models.transformer.filter_predictor as rf
    import ltr.models.transformer.transformer as rt
    from pytracking_amd import install as amd, tamos as TA, transformer as TM
    kw = dict(d_model=128, nhead=4, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=256)
    orig, orig_tr = rf.GOTFilterPredictor, rt.Transformer
    ref_keys = list(orig(orig_tr(**kw), feature_sz=6, num_tokens=3, label_enc="gaussian", box_enc="ltrb_token").state_dict().keys())
    amd.install()                                              # the default set leaves the class alone
    try:
        assert rf.GOTFilterPredictor is orig
    finally:
        amd.uninstall()
    amd.install(tamos=True)
    try:
        assert rf.GOTFilterPredictor is not orig and issubclass(rf.GOTFilterPredictor, orig) and rf.GOTFilterPredictor.__name__ == "GOTFilterPredictor"
        t = rt.Transformer(**kw)
        assert isinstance(t, TM.Transformer)
        mine = rf.GOTFilterPredictor(t, feature_sz=6, num_tokens=3, label_enc="gaussian", box_enc="ltrb_token")
        assert isinstance(mine, TA.GOTFilterPredictor) and list(mine.state_dict().keys()) == ref_keys
        for other in (dict(num_tokens=3, label_enc="gaussian", box_enc="ltrb"), dict(num_tokens=3, label_enc="other", box_enc="ltrb_token"),
                      dict(num_tokens=17, label_enc="gaussian", box_enc="ltrb_token")):
            m = rf.GOTFilterPredictor(t, feature_sz=6, **other)
            assert isinstance(m, orig) and not isinstance(m, TA.GOTFilterPredictor)
        pre = rt.Transformer(normalize_before=True, **kw)          # the reference's own transformer: the reference's predictor
        m = rf.GOTFilterPredictor(pre, feature_sz=6, num_tokens=3, label_enc="gaussian", box_enc="ltrb_token")
        assert isinstance(m, orig) and not isinstance(m, TA.GOTFilterPredictor)
    finally:
        amd.uninstall()
    assert rf.GOTFilterPredictor is orig and rt.Transformer is orig_tr and not amd.installed()


def test_mirror_refuses_what_it_does_not_cover():
    from pytracking_amd import tamos as TA, transformer as TM
    t = TM.Transformer(d_model=128, nhead=4, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=256)
    for kw in (dict(num_tokens=3, box_enc="ltrb"), dict(num_tokens=3, label_enc="x", box_enc="ltrb_token"),
               dict(num_tokens=0, box_enc="ltrb_token"), dict(num_tokens=17, box_enc="ltrb_token")):
        with pytest.raises(NotImplementedError):
            TA.GOTFilterPredictor(t, 6, **kw)
    with pytest.raises(NotImplementedError):
        TA.GOTFilterPredictor(torch.nn.Identity(), 6, num_tokens=3, box_enc="ltrb_token")


# ---- seeded defects ---------------------------------------------------------------------------------------------------------------
SMALL = [n for n in CASES if n not in ("deployed", "keys1444", "head16_keys1452")]
_par = lambda c: c["mode"] == "parallel"
REACHES = {
    "rotated_embeddings": lambda c: c["T"] >= 2,
    "self_only": lambda c: c["T"] >= 2 and c["n_dec"] >= 2,            # the first layer's self-attention sees tgt = 0: a constant
    "mask_one_late": lambda c: _par(c) and c["num_gth_frames"] < c["n_train"],
    "gth_plus_one": lambda c: _par(c) and c["num_gth_frames"] < c["n_train"],
    "ln_eps": lambda c: True,
}


@pytest.mark.parametrize("defect", TN.DEFECTS)
def test_bound_catches_seeded_defect(defect):
    """On every small case the defect reaches, the mutated fp32 run leaves F_MAX x ref_err of float64 on the predictor's own outputs (so it
    fails under every F the rule of tests/tamos_f64.py can choose); the LayerNorm eps is also held to 12 x on the base case."""
    reached = [n for n in SMALL if REACHES[defect](TC.CASES[n])]
    assert len(reached) >= 3
    ratios = {}
    for name in reached:
        a = F64.anchor(name)
        errs = f64_bound.errors(a.want, F64.outputs(name, np.float32, defect=defect))
        ratios[name] = max(e / TC.REF_ERR[name]["predictor"] for q, e in errs.items() if F64.group(q) == "predictor")
        assert not f64_bound.within(errs, TC.REF_ERR[name], F64.F, group=F64.group), (name, ratios[name])
    print(f"\n{defect}: worst output / ref_err " + " ".join(f"{n} {r:.3g}" for n, r in ratios.items()))
    assert min(ratios.values()) > F64.F_MAX
    if defect == "ln_eps":
        assert ratios["base_t3"] >= 12
    # the unmodified fp32 run stays inside
    assert all(f64_bound.within(F64.anchor(n).ref_errs, TC.REF_ERR[n], F64.F, group=F64.group) for n in reached)
