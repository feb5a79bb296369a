"""CPU checks of the ToMP route cases (tests/tomp_cases.py, tests/tomp_f64.py), no GPU:

* every case lands on its pinned route list (pt_tomp_predict_routes / pt_tomp_bbreg_routes / pt_tomp_linear_routes, host only);
* coverage is a condition on the table: every route id the queries return anywhere on the advertised grid is hit by a case, and the ids
  the grid never returns are exactly the ones listed as unreachable from ToMP;
* the refusals sit exactly at the documented limits, in the queries and in the *_ws_bytes functions alike;
* the fp32 oracle run stays fp32, and its distance from float64 -- ref_err -- lies within [0.5, 2] x the committed value;
* the bound F x ref_err has teeth: five seeded defects of the fp32 oracle run (LayerNorm eps 2e-5, one masked key unmasked, max_res + 1,
  num_gth_frames +- 1, the query scaled before its bias) each leave the bound on every case that reaches the mutated code; the unmodified fp32 run stays
  within it."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import tomp_cases as TC
import f64_bound
import tomp_f64 as F64
from f64_bound import FACTOR
from oracle import tomp_oracle as TO
from pytracking_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never returned on the advertised grid with aligned buffers: the scalar-epilogue k_gemm_ps variants (wide_store_ok holds for every
# plain product of the predictor), k_gemm<64,64,0,32> and k_gemm_big (k_gemm_ps takes every N >= 1024 product first), k_ln_rows_t<1>
# (d_model % 128), the two-addend mode of k_ln_rows_t<4> (FFN2 is split in four or not at all) and the decoder whose first layer is not
# served from the prepared constants (d_model >= 96 always is)
UNREACHABLE = {"GEMM_PS2", "GEMM_PS4", "GEMM_PS4_SPLITK", "GEMM_T64", "GEMM_BIG", "LN64", "LN256_SPLIT2", "DEC0_LIVE"}
ALL_CASES = [(kind, name) for kind, table in F64.TABLES for name in table]


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _dims(D=256, nhead=8, ff=256, n_enc=1, n_dec=1, H=5, W=5):
    return _lib.TompDims(D, nhead, ff, n_enc, n_dec, H, W, max(H, W))


def _pred(L, d, n_train, n_seq, parallel):
    return TC._query(L.pt_tomp_predict_routes, ctypes.byref(d), n_train, n_seq, parallel)


def test_route_names_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "pt_hot.h")).read()
    body = hdr[hdr.index("enum pt_tomp_route {"):]
    body = body[:body.index("};")]
    names = re.findall(r"PT_TOMP_R_(\w+)", body)
    assert names[-1] == "COUNT" and tuple(names[:-1]) == _lib.TOMP_ROUTES
    assert int(re.search(r"#define PT_TOMP_MAX_ROUTES (\d+)", hdr).group(1)) == _lib.PT_TOMP_MAX_ROUTES
    assert _lib.lib().pt_abi_version() == 1


def test_tables_are_complete():
    names = [n for _, t in F64.TABLES for n in t]
    assert len(set(names)) == len(names) and set(names) == set(TC.ROUTES) == set(TC.REF_ERR)
    for text in TC.ROUTES_TEXT.values():
        assert TC.compress(TC.expand(text)) == text


@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_case_lands_on_its_pinned_routes(L, kind, name):
    if kind == "predict":
        cfg = TC.PREDICT[name]
        d = TC.dims(cfg)
        assert L.pt_tomp_predict_ws_bytes(ctypes.byref(d), cfg["n_train"], cfg["n_seq"], int(cfg["mode"] == "parallel")) > 0
        assert 0 <= cfg["num_gth_frames"] <= cfg["n_train"]
        if cfg["mode"] == "parallel":                          # the classifier's correlation and the regressor take the encoded maps
            assert L.pt_apply_filter_ws_bytes(1, cfg["D"], cfg["H"], cfg["W"], 1, 1, cfg["H"], cfg["W"]) > 0
            assert L.pt_tomp_bbreg_ws_bytes(1, cfg["D"], cfg["H"], cfg["W"]) > 0
        rc, r = TC.case_routes(L, name)
    elif kind == "bbreg":
        assert L.pt_tomp_bbreg_ws_bytes(*TC.BBREG[name]) > 0
        rc, r = TC.bbreg_routes(L, *TC.BBREG[name])
    else:
        rc, r = TC.linear_routes(L, *TC.LINEAR[name][:3])
    assert rc == 0 and r == TC.ROUTES[name], (rc, TC.compress(r))


def test_cases_reach_what_they_are_there_for():
    """The shape arithmetic behind the table's comments."""
    P, rows = TC.PREDICT, lambda c: (2 if c["mode"] == "parallel" else c["n_seq"]) * (c["n_train"] + 1) * c["H"] * c["W"]
    assert all(rows(P[n]) == 1024 for n in P if n.startswith("m1024")) and rows(P["m1296_ff1280"]) % 128 != 0
    assert [P[n]["ff"] // 64 // 4 for n in ("m1024_ff256", "m1024_ff768", "m1024_ff1024", "m1296_ff1280")] == [1, 3, 4, 5]   # split-K stages
    assert P["m1024_ff320"]["ff"] % 256 != 0 and (P["m1024_ff320"]["ff"] // 64) % 4 != 0
    assert 481 <= rows(P["swz_pad_532"]) < 1024 and ((rows(P["swz_pad_532"]) + 31) // 32) % 8 != 0
    for n in ("mask9_gth0", "mask16_gth0"):                  # the bbreg row's first 128-key iteration is nothing but masked keys
        assert P[n]["num_gth_frames"] == 0 and P[n]["n_train"] * P[n]["H"] * P[n]["W"] >= 128
    c = P["lds_limit"]
    Lk = (c["n_train"] + 1) * c["H"] * c["W"]
    assert c["nhead"] * (Lk + 4) <= 11000 < c["nhead"] * (Lk + c["W"] + 4) and Lk % 16 != 0
    c = P["long_scores"]
    assert (c["n_train"] + 1) * c["H"] * c["W"] > 64 * 22                                   # k_dec_ctx: more scores than its registers hold
    assert sorted(P[n]["n_seq"] for n in P if n.startswith("seq")) == [3, 3, 5, 5, 8, 8]
    assert {(P[n]["D"], P[n]["D"] // P[n]["nhead"]) for n in P} >= {(D, hd) for D in (128, 256, 384, 512) for hd in (32, 64)} | {(128, 16), (256, 16)}
    slices = lambda n, D, H, W: -(-H * W * D // 1024)
    assert slices(*TC.BBREG["reg_d512_23x23_n1"]) > 256 >= slices(*TC.BBREG["reg_d512_6x6_n1"]) and 5 * 5 < 32


def _grid_routes(L):
    """Every route id the three queries return on the advertised grid (accepted, aligned configurations)."""
    seen = set()
    maps = [(h, h) for h in (1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 13, 16, 18, 20, 22, 23, 26, 32)] + [(5, 7), (7, 19), (18, 19), (3, 43), (19, 19)]
    heads = {128: (2, 4, 8), 256: (4, 8, 16), 384: (6, 12), 512: (8, 16)}
    ffs = [64 * k for k in range(1, 41)]
    calls = 0
    for D, nheads in heads.items():
        for nhead in nheads:
            for H, W in maps:
                for n_train in (1, 2, 3):
                    if nhead * ((n_train + 1) * H * W + 4) > 11000:
                        continue
                    # dim_ff only enters through FFN1 / FFN2 and the decoder's two FFN GEMVs: the full range of it at two batch shapes
                    for n_seq, par in [(1, 1)] + [(s, 0) for s in range(1, 9)]:
                        for ff in (ffs if (n_seq, par) in ((1, 1), (3, 0)) else (256, 320, 768, 1024)):
                            for n_enc, n_dec in ((1, 2),) if ff != 256 else ((1, 2), (0, 1), (1, 0), (0, 0), (16, 16)):
                                d = _lib.TompDims(D, nhead, ff, n_enc, n_dec, H, W, max(H, W))
                                rc, r = _pred(L, d, n_train, n_seq, par)
                                assert rc == 0 and bool(L.pt_tomp_predict_ws_bytes(ctypes.byref(d), n_train, n_seq, par)), (D, nhead, ff, H, W, n_train, n_seq, par)
                                seen.update(r)
                                calls += 1
    for n in (1, 2, 3, 8):
        for D in range(64, 513, 64):
            for H, W in maps:
                rc, r = TC.bbreg_routes(L, n, D, H, W)
                assert rc == 0
                seen.update(r)
    for B in range(1, 9):
        for N in (1, 4, 130, 256, 258, 2048, 65535, 65536, 70000):
            for K in range(64, 2049 + 64, 64):
                rc, r = TC.linear_routes(L, B, N, K)
                assert rc == 0
                seen.update(r)
    assert calls > 50000
    return seen


def test_every_reachable_route_is_hit_by_a_case(L):
    reachable = _grid_routes(L)
    hit = set().union(*TC.ROUTES.values())
    assert hit <= reachable
    assert reachable - hit == set(), sorted(reachable - hit)
    assert set(TC.R[1:]) - reachable == UNREACHABLE, sorted(set(TC.R[1:]) - reachable)


def test_refusals_sit_at_the_documented_limits(L):
    ok = lambda d, nt, ns, par: (bool(L.pt_tomp_predict_ws_bytes(ctypes.byref(d), nt, ns, par)), _pred(L, d, nt, ns, par)[0])
    d = _dims()
    assert ok(d, 1, 8, 0) == (True, 0) and ok(d, 1, 9, 0) == (False, _lib.PT_ERR_UNSUPPORTED)              # batch rows
    assert ok(d, 1, 1, 1) == (True, 0) and ok(d, 1, 2, 1) == (False, _lib.PT_ERR_UNSUPPORTED)              # parallel: one sequence
    assert ok(d, 0, 1, 0) == (False, _lib.PT_ERR_SHAPE) and ok(d, 1, 0, 0) == (False, _lib.PT_ERR_SHAPE)
    # LDS of k_dec_ctx: nhead (L + 4) <= 11000.  nhead 8: L = 1371 is the last one in; 18x19 x 4 frames = 1368 in, 19x19 x 4 = 1444 out
    assert ok(_dims(nhead=8, H=1, W=457), 2, 1, 0) == (True, 0) and 8 * (3 * 457 + 4) == 11000           # exactly on the limit
    assert ok(_dims(nhead=8, H=1, W=686), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED) and 8 * (2 * 686 + 4) == 11008
    assert ok(_dims(H=18, W=19), 3, 1, 0) == (True, 0) and ok(_dims(H=19, W=19), 3, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)
    # model width, head width, dim_ff
    assert ok(_dims(D=512, nhead=8), 1, 1, 0) == (True, 0) and ok(_dims(D=640, nhead=10), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)
    assert ok(_dims(D=192, nhead=6), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)                          # d_model % 128
    assert ok(_dims(D=128, nhead=8), 1, 1, 0) == (True, 0) and ok(_dims(D=128, nhead=16), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)   # head width 16 / 8
    assert ok(_dims(D=512, nhead=4), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)                          # head width 128
    assert ok(_dims(D=256, nhead=6), 1, 1, 0) == (False, _lib.PT_ERR_SHAPE)                                # d_model % nhead
    assert ok(_dims(ff=64), 1, 1, 0) == (True, 0) and ok(_dims(ff=96), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)
    assert ok(_dims(n_enc=16, n_dec=16), 1, 1, 0) == (True, 0) and ok(_dims(n_enc=17), 1, 1, 0) == (False, _lib.PT_ERR_UNSUPPORTED)
    assert ok(_dims(n_enc=0, n_dec=0), 1, 1, 0) == (True, 0)
    # the longest list fits PT_TOMP_MAX_ROUTES; a short buffer is refused with everything zeroed
    big = _dims(n_enc=16, n_dec=16)
    rc, r = _pred(L, big, 1, 1, 0)
    assert rc == 0 and len(r) == 4 + 16 * 7 + 1 + 16 * 7 - 2 + 1 + 1 <= _lib.PT_TOMP_MAX_ROUTES
    out, n = (ctypes.c_int * 8)(*([7] * 8)), ctypes.c_int(-1)
    assert L.pt_tomp_predict_routes(ctypes.byref(big), 1, 1, 0, out, 8, ctypes.byref(n)) == _lib.PT_ERR_WORKSPACE and n.value == 0 and not any(out)
    assert L.pt_tomp_predict_routes(ctypes.byref(big), 1, 1, 0, None, 8, ctypes.byref(n)) == _lib.PT_ERR_NULL
    assert L.pt_tomp_predict_routes(ctypes.byref(big), 1, 1, 0, out, 8, None) == _lib.PT_ERR_NULL
    assert L.pt_tomp_predict_routes(None, 1, 1, 0, out, 8, ctypes.byref(n)) == _lib.PT_ERR_NULL
    # box regressor: d_model % 64, <= 512
    for args, want in (((1, 512, 6, 6), 0), ((1, 576, 6, 6), _lib.PT_ERR_UNSUPPORTED), ((1, 96, 6, 6), _lib.PT_ERR_UNSUPPORTED),
                       ((0, 256, 6, 6), _lib.PT_ERR_SHAPE), ((1, 256, 0, 6), _lib.PT_ERR_SHAPE)):
        assert TC.bbreg_routes(L, *args)[0] == want and bool(L.pt_tomp_bbreg_ws_bytes(*args)) == (want == 0), args
    assert L.pt_tomp_bbreg_routes(1, 256, 6, 6, None, 8, ctypes.byref(n)) == _lib.PT_ERR_NULL
    # linear: B <= 8, K % 64
    assert TC.linear_routes(L, 8, 130, 192)[0] == 0 and TC.linear_routes(L, 9, 130, 192)[0] == _lib.PT_ERR_UNSUPPORTED
    assert TC.linear_routes(L, 1, 4, 64)[0] == 0 and TC.linear_routes(L, 1, 4, 96)[0] == _lib.PT_ERR_UNSUPPORTED
    assert TC.linear_routes(L, 0, 4, 64)[0] == _lib.PT_ERR_SHAPE
    assert L.pt_tomp_linear_routes(1, 4, 64, None, 8, ctypes.byref(n)) == _lib.PT_ERR_NULL
    # ... and the entry point itself refuses B = 9 and K = 96 before anything is queued (no GPU here)
    one = ctypes.c_void_p(256)
    assert L.pt_tomp_linear_f32(one, one, one, one, 9, 130, 192, 0, None) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_tomp_linear_f32(one, one, one, one, 1, 4, 96, 0, None) == _lib.PT_ERR_UNSUPPORTED


@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_fp32_oracle_stays_within_the_bound_and_ref_err_is_the_committed_one(kind, name):
    a = F64.anchor(kind, name)                                   # asserts that the fp32 run's outputs are fp32
    assert list(a.ref_err) == list(TC.REF_ERR[name])
    f64_bound.held(f"{name} (fp32 oracle)", a.ref_errs, None, TC.REF_ERR[name], F64.F, group=F64.group)
    lo, hi = F64.REF_ERR_BAND
    for g, r in a.ref_err.items():
        assert lo * TC.REF_ERR[name][g] <= r <= hi * TC.REF_ERR[name][g], (g, r, TC.REF_ERR[name][g])


def test_fp32_oracle_keeps_fp32_inside():
    """Not only the outputs: the attention of an fp32 run works on fp32 operands (the -inf mask, the scale and the LayerNorm eps are
    python scalars and must not promote)."""
    seen = []
    orig = TO.mha

    def spy(p, prefix, query, key, value, nhead, key_padding_mask=None):
        out = orig(p, prefix, query, key, value, nhead, key_padding_mask)
        seen.append((query.dtype, key.dtype, value.dtype, out.dtype))
        return out
    cfg, params, inputs = TC.predict_case("mask9_gth1")
    TO.mha = spy
    try:
        F64.predict_outputs(cfg, params, inputs, np.float32)
    finally:
        TO.mha = orig
    assert len(seen) == cfg["n_enc"] + 2 * cfg["n_dec"] and all(t == (np.float32,) * 4 for t in seen), seen


def test_factor():
    assert F64.F >= FACTOR and F64.F <= F64.F_MAX == 32 and F64.bound(1.0) == F64.F


# ------------------------------------------------------------------------------------------------------------------
# seeded defects of the fp32 oracle run
# ------------------------------------------------------------------------------------------------------------------
def _ln_eps(monkeypatch, cfg):
    orig = TO.layer_norm
    monkeypatch.setattr(TO, "layer_norm", lambda x, g, b, eps=1e-5: orig(x, g, b, 2e-5))
    return {}


def _unmask_one_key(monkeypatch, cfg):
    orig = TO.transformer

    def patched(p, pre, feat, mask, *rest):
        mask = mask.copy()
        mask[1, np.flatnonzero(mask[1])[0]] = False
        return orig(p, pre, feat, mask, *rest)
    monkeypatch.setattr(TO, "transformer", patched)
    return {}


def _max_res(monkeypatch, cfg):
    return dict(feature_sz=cfg["feature_sz"] + 1)


def _gth(monkeypatch, cfg):
    g = cfg["num_gth_frames"]
    return dict(gth=g + 1 if g < cfg["n_train"] else g - 1)


def _scale_before_bias(monkeypatch, cfg):
    orig = TO.mha

    def patched(p, prefix, query, key, value, nhead, key_padding_mask=None):
        E = query.shape[-1]
        q = dict(p)
        b = p[prefix + "in_proj_bias"].copy()
        b[:E] *= math.sqrt(E // nhead)                          # (x W^T) s + b  ==  (x W^T + b / s) s
        q[prefix + "in_proj_bias"] = b.astype(p[prefix + "in_proj_bias"].dtype)
        return orig(q, prefix, query, key, value, nhead, key_padding_mask)
    monkeypatch.setattr(TO, "mha", patched)
    return {}


_layers = lambda c: c["n_enc"] + c["n_dec"] > 0
_masked = lambda c: c["mode"] == "parallel" and _layers(c) and c["num_gth_frames"] < c["n_train"]
DEFECTS = {                                    # name: (seed, reaches the case)
    "layer_norm_eps_2e-5": (_ln_eps, _layers),          # without layers the only LayerNorm sees the all-zero query: eps drops out
    "one_masked_key_unmasked": (_unmask_one_key, _masked),
    "max_res_plus_1": (_max_res, _layers),
    "num_gth_frames_off_by_one": (_gth, lambda c: c["mode"] == "parallel" and _layers(c)),
    "query_scaled_before_bias": (_scale_before_bias, _layers),
}
SMALL = [n for n in TC.PREDICT if n not in TC.DEPLOYED]


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_bound_catches_seeded_defect(monkeypatch, defect):
    """On every case the defect reaches, the mutated fp32 run leaves F x ref_err of float64 on the predictor's own outputs."""
    seed, reaches = DEFECTS[defect]
    ratios = {}
    for name in TC.PREDICT if defect == "layer_norm_eps_2e-5" else SMALL:
        cfg, params, inputs = TC.predict_case(name)
        if not reaches(cfg):
            continue
        with monkeypatch.context() as m:
            kw = seed(m, cfg)
            got = F64.predict_outputs(cfg, params, inputs, np.float32, **kw)
        errs = f64_bound.by_group(f64_bound.errors(F64.anchor("predict", name).want, got), F64.group)
        ratio = errs["predictor"] / TC.REF_ERR[name]["predictor"]
        ratios[name] = ratio
        assert ratio > F64.F, (name, ratio)
    weakest = min(ratios, key=ratios.get)
    print(f"\n{defect}: {len(ratios)} cases, weakest {weakest} at {ratios[weakest]:.0f} x ref_err (F = {F64.F})")
    # why F may never exceed F_MAX: wherever a decoder runs, even the weakest defect -- the LayerNorm eps, 47 x ref_err at the deployed
    # size -- stays outside F_MAX x ref_err.  (One encoder layer alone, enc1_dec0, moves by 13 x ref_err: caught at F = 4, not at 32.)
    assert all(r > F64.F_MAX for n, r in ratios.items() if TC.PREDICT[n]["n_dec"] > 0), ratios
