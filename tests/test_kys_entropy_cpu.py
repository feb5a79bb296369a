"""The trained KYS predictor structure -- one 16-wide representation layer, conf_measure 'entropy' (ltr/train_settings/kys/kys.py:110-114) --
without a GPU: the float64 restatement (tests/kys_entropy_np.py) reproduces the kys_ent_* goldens of the unmodified reference
(tools/make_golden_kys.py ent ent_loop), the case set spans the entropy range, the C ABI accepts exactly the covered list of
include/pt_hot.h and checks its arguments before any launch, the weight pack has the documented order, and every seeded defect of the
restatement leaves the bound the GPU test holds (kys_entropy_np.FACTOR x max(ref_fp32_err, one ulp of the output's range)) on a committed case."""
import ctypes
import os

import numpy as np
import pytest
import torch

import f64_bound
import kys_ent_modules
import kys_entropy_np as KE
import kys_np
from pytracking_amd import _lib, kys as K, synth

from kys_entropy_np import CASES, GOLDEN, SIZES, golden_outputs, load, restated


def test_the_case_set_is_the_committed_one():
    have = sorted(fn[:-4] for fn in os.listdir(GOLDEN) if fn.startswith("kys_ent_") and "_pw_" not in fn and fn != "kys_ent_loop.npz")
    assert have == sorted(CASES)
    for fn in os.listdir(GOLDEN):
        if fn.startswith("kys_ent_"):
            assert os.path.getsize(os.path.join(GOLDEN, fn)) <= 512 << 10, fn


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_golden(name):
    g, c, want = restated(name)
    assert float(g["thresh_margin"]) > 1e-3
    ref, pw = golden_outputs(g)
    assert sorted(list(ref) + ["propagation_weights"]) == sorted(want)
    assert ("propagation_conf" in want) == (c["conf"] != "none")
    assert sorted(g["aux_keys"]) == sorted(list(k for k in want if k not in ("response", "state_cur")) + ["cost_volume_processed"])
    for k, r in ref.items():
        err = np.abs(want[k].reshape(r.shape) - r).max()
        assert err <= float(g["err_" + k]) * 1.0000001 <= 1e-4, (k, err, float(g["err_" + k]))    # the stored error IS this distance
    w = want["propagation_weights"].reshape(-1)
    assert w.size == int(pw["numel"])
    err = np.abs(w - pw["propagation_weights"].reshape(-1)).max() if "propagation_weights" in pw else np.abs(w[pw["sample_idx"]] - pw["sample"]).max()
    assert err <= float(pw["ref_fp32_err"]) * 1.0000001 <= 1e-4          # 2.4e-5 at 20 x 20, gain 30: the gain scales the logits' fp32 rounding too


def test_numpy_closed_loop_matches_golden():
    g = load("kys_ent_loop")
    B, C, H, W, md = (int(g[k]) for k in ("B", "C", "H", "W", "md"))
    sd = KE.predictor_state(int(g["state_seed"]), "entropy")
    assert float(g["dimp_thresh"]) == 0.05
    for t in (0, int(g["frames"]) - 1):                          # the first frame (label_prev) and the last (golden state of the one before)
        cur, prev = synth.kys_features(int(g["seed"]) + t, B, C, H, W)
        inp = synth.kys_frame_inputs(int(g["seed"]) + 100 + t, B, H, W)
        out = KE.predict_response(sd, kys_np.cost_volume_gram(cur, prev, md), inp["dimp_score_cur"], state_prev=None if t == 0 else g["state_cur"][t - 1],
                                  label_prev=inp["label_prev"], dimp_thresh=0.05, window=inp["window"], conf_measure="entropy")
        np.testing.assert_allclose(out["response"].reshape(g["response"][t].shape), g["response"][t], atol=1e-5, rtol=0)
        np.testing.assert_allclose(out["state_cur"], g["state_cur"][t], atol=1e-5, rtol=0)


@pytest.mark.parametrize("size", SIZES)
def test_the_cases_span_the_entropy_range(size):
    """Below a quarter and above nine tenths of ln(HW) somewhere at every size with more than one position; a single position has the
    one-term softmax, whose entropy is -log(1.0001)."""
    conf = np.concatenate([restated(n)[2]["propagation_conf"].reshape(-1) for n in CASES if n.split("_")[2] == size and restated(n)[1]["conf"] == "entropy"])
    g = restated(f"kys_ent_{size}_a")[0]
    HW = int(g["shape"][2]) * int(g["shape"][3])
    print(f"\n{size}: float64 entropy {conf.min():.4g} .. {conf.max():.4g} of ln(HW) = {np.log(HW):.4g}")
    if HW == 1:
        np.testing.assert_allclose(conf, -np.log(1.0 + KE.EPS), atol=1e-15, rtol=0)
    else:
        assert conf.min() < 0.25 * np.log(HW) and conf.max() > 0.9 * np.log(HW)


@pytest.fixture(scope="module")
def L():
    if _lib.needs_build():
        _lib.build_library()
    return _lib.lib()


def test_the_covered_list_is_closed(L):
    assert (_lib.PT_KYS_CONF_NONE, _lib.PT_KYS_CONF_MAX, _lib.PT_KYS_CONF_ENTROPY) == (0, 1, 2)
    wf = L.pt_kys_weight_floats
    assert wf(8, 16, 0, 3, 2) == wf(8, 16, 0, 3, 1) == 4924 and wf(8, 16, 0, 3, 0) == 4780
    assert wf(8, 64, 32, 3, 1) == 27900 and wf(8, 64, 32, 3, 0) == 27900 - 64 * 9
    assert wf(8, 64, 32, 3, 2) == 0                              # (64, 32) with entropy: refused (tests/test_gpu_kys.py pins it)
    assert wf(8, 16, 16, 3, 2) == wf(8, 16, 16, 3, 1) == wf(8, 32, 0, 3, 2) == wf(8, 64, 0, 3, 1) == wf(8, 16, 32, 3, 1) == 0
    assert wf(8, 16, 0, 3, 3) == wf(8, 16, 0, 3, -1) == wf(8, 64, 32, 3, 3) == 0
    assert wf(16, 16, 0, 3, 2) == wf(8, 16, 0, 5, 2) == 0
    assert L.pt_kys_predict_ws_bytes(1, 18, 18) == (324 * 324 + (8 + 1 + 64 + 32) * 324) * 4      # its value is the parent's


def test_predict_argument_checks_do_not_launch(L):
    n, one, big = None, ctypes.c_void_p(256), 1 << 40

    def prm(B=1, H=18, W=18, sd=8, r0=16, r1=0, gk=3, conf=2, floats=4924, wstride=0):
        return _lib.KysPredictParams(B, H, W, sd, r0, r1, gk, conf, 1, 0.05, 0.25, wstride, floats)

    def call(p, ptrs=None, nbytes=big):
        return L.pt_kys_predict_response_f32(ctypes.byref(p), *(ptrs or [one] * 16), nbytes, n)

    assert call(prm(), [one] * 10 + [n] + [one] * 5) == _lib.PT_ERR_NULL                       # entropy without its output
    assert call(prm(conf=1), [one] * 10 + [n] + [one] * 5) == _lib.PT_ERR_NULL
    assert call(prm(conf=0, floats=4780), [one] * 10 + [n] + [one] * 5, nbytes=0) == _lib.PT_ERR_WORKSPACE  # 'none' has no such output
    assert call(prm(floats=4923)) == call(prm(conf=1, floats=4779)) == call(prm(wstride=7)) == _lib.PT_ERR_SHAPE   # a short pack
    assert call(prm(conf=3)) == call(prm(r0=64, r1=32, floats=27900)) == call(prm(r1=16)) == call(prm(r0=32)) == _lib.PT_ERR_UNSUPPORTED
    assert call(prm(H=21, W=20)) == call(prm(sd=16)) == call(prm(gk=5)) == _lib.PT_ERR_UNSUPPORTED
    assert call(prm(), nbytes=L.pt_kys_predict_ws_bytes(1, 18, 18) - 4) == _lib.PT_ERR_WORKSPACE


def test_pack_of_the_trained_structure_has_the_documented_order(L):
    sd = KE.predictor_state(1310, "entropy")
    w = kys_ent_modules.wrapper(sd, "entropy", 9, "cpu", dimp_thresh=0.05)
    assert K._dims(w.predictor) == (8, 16, 0, 3, _lib.PT_KYS_CONF_ENTROPY)
    pack = K.pack_weights(w.predictor).numpy()
    assert pack.shape == (4924,) and pack.dtype == np.float32
    # behind the two cost-volume stacks (306), init_hidden_state (72) and is_target (329): W 16 x 10, b 16, response W 1 x 16, b 1, the ConvGRU
    at = 306 + 72 + 329
    for key in ("representation_predictor.0.0.weight", "representation_predictor.0.0.bias", "response_predictor.0.0.weight",
                "response_predictor.0.0.bias", "state_predictor.conv_reset.weight"):
        np.testing.assert_array_equal(pack[at:at + sd[key].size], sd[key].reshape(-1), err_msg=key)
        at += sd[key].size
    assert at == 707 + 1440 + 16 + 144 + 1 + 864
    np.testing.assert_array_equal(pack[-8:], sd["state_predictor.conv_state_new.bias"])
    np.testing.assert_array_equal(pack[306:378], sd["init_hidden_state_predictor.0.0.weight"].reshape(-1))
    assert K.pack_weights(kys_ent_modules.wrapper(KE.predictor_state(1310, "none"), "none", 9, "cpu").predictor).numel() == 4780
    for conf, dims in (("entropy", (64, 32)), ("entropy", (16, 16)), ("max", (32,)), ("bogus", (16,))):
        odd = kys_ent_modules.Predictor(conf, dims=dims)
        assert K._dims(odd) is None
        with pytest.raises(NotImplementedError, match=r"\(16,\)"):
            K.pack_weights(odd)
    assert K._dims(kys_ent_modules.Predictor("max", dims=(64, 32))) == (8, 64, 32, 3, 1)
    assert K._dims(kys_ent_modules.Predictor("none", dims=(16,))) == (8, 16, 0, 3, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# seeded defects: each must leave the GPU test's bound on at least one committed case (if one ever passes: add a case, not a factor)

def _worst_ratio(name, defect):
    """largest err / (max(ref_fp32_err, ulp of the output's range)) over the outputs of a case, restatement with `defect` against without"""
    g, c, want = restated(name)
    got = KE.flat(KE.restate(c, defect))
    worst = 0.0
    for k, w in want.items():
        ref_err = float(load("kys_ent_pw_" + str(g["pw"]))["ref_fp32_err"]) if k == "propagation_weights" else float(g["err_" + k])
        unit = max(ref_err, f64_bound.ulp_of_max(w))
        worst = max(worst, float(np.abs(got[k] - w).max()) / unit)
    return worst


@pytest.mark.parametrize("defect", KE.DEFECTS)
def test_the_bound_catches_the_seeded_defect(defect):
    for name in ("kys_ent_5x7_b", "kys_ent_4x4_s", "kys_ent_1x1_a"):
        r = _worst_ratio(name, defect)
        print(f"\n{defect} on {name}: {r:.3g} x max(ref_fp32_err, ulp); the bound is {KE.FACTOR} x")
        if r > KE.FACTOR:
            return
    pytest.fail(f"{defect} stays inside the bound on every case tried")


def test_the_restatement_itself_is_inside_the_bound():
    assert _worst_ratio("kys_ent_5x7_b", None) == 0.0


def test_entropy_of_known_distributions():
    w = np.zeros((1, 4, 1, 2))
    w[0, :, 0, 0] = 0.25                                                   # uniform over 4: ln 4, less the 1e-4 inside the logarithm
    w[0, 0, 0, 1] = 1.0                                                    # one-hot: -log(1.0001), below zero
    e = KE.entropy(w)
    np.testing.assert_allclose(e[0, 0, 0], [-np.log(0.25 + KE.EPS), -np.log(1.0 + KE.EPS)], atol=1e-15, rtol=0)
    assert e[0, 0, 0, 1] < 0 and abs(e[0, 0, 0, 1] + 1e-4) < 1e-8
    t = torch.from_numpy(w).float()
    ref = -(t * (t + 1e-4).log()).sum(dim=1)                               # response_predictor.py:116
    np.testing.assert_allclose(e[0, 0], ref[0].numpy(), atol=1e-7, rtol=0)
