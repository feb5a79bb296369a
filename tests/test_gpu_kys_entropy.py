"""The trained KYS predictor structure on the MI355X: one 16-wide representation layer (kept in LDS by k_kys_head) and conf_measure 'entropy'
(k_kys_propagate), the network ltr/train_settings/kys/kys.py:110-114 builds and pytracking/parameter/kys/default.py loads.

Every case of tests/golden/kys_ent_*.npz (tools/make_golden_kys.py ent ent_loop; the unmodified reference on CPU) is held, output by output,
  * to the float64 restatement tests/kys_entropy_np.py within FACTOR x max(ref_fp32_err, one fp32 ulp of that output's range), ref_fp32_err
    being the reference's own fp32 distance from the same float64 run, recorded in the golden (tests/f64_bound.py);
  * to the reference's fp32 output within the flat 1e-4 of the existing predictor test;
  * to a second call on the same inputs bit for bit.
Then the 8-frame closed loop, the refusals of the covered list, and the reference's own kysnet_res50 with the train setting's arguments
through install().  The worst ratio per output goes to the file KYS_ENTROPY_F64_OUT names (profiles/kys_entropy_f64.txt).

FACTOR is kys_entropy_np.FACTOR = f64_bound.raised_factor(2.88, 64) = 6: the worst ratio measured on the MI355X is 2.88 (propagation_conf of
4x4_s), above FACTOR / 2; the seeded defects of tests/test_kys_entropy_cpu.py are held to the same raised factor.

Every test prints its measured errors before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import f64_bound
import kys_ent_modules
import kys_entropy_np as KE
from f64_bound import dev
from oracle import ref_harness
from pytracking_amd import kys as K, synth
from kys_entropy_np import CASES, golden_outputs, load, restated

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FACTOR = KE.FACTOR
TABLE = f64_bound.Table("KYS_ENTROPY_F64_OUT", "KYS predictor, (16,) representation stack, conf_measure entropy / max / none: MI355X output against "
                        "the float64 restatement,\nerr / max(ref_fp32_err, one ulp of the output's range); the bound is " + str(FACTOR) + " x")


def _run(w, c):
    """the case through the wrapper's own predict_response where it has one (the reference's class under install()), else through K"""
    i = c["inp"]
    data = {"feat1": dev(c["prev"]), "feat2": dev(c["cur"]), "dimp_score_cur": dev(i["dimp_score_cur"]), "label_prev": dev(i["label_prev"]),
            "state_prev": dev(c["state"])}
    with torch.no_grad():
        if hasattr(w, "predict_response"):
            return w.predict_response(data, dimp_thresh=c["thresh"], output_window=dev(c["window"]))
        return K.predict_response(w, data, dimp_thresh=c["thresh"], output_window=dev(c["window"]))


def _check(name, out):
    g, c, want = restated(name)
    B, H, W = c["B"], c["H"], c["W"]
    aux = out["auxiliary_outputs"]
    assert sorted(aux) == sorted(g["aux_keys"]) and sorted(out) == ["auxiliary_outputs", "cost_volume", "response", "state_cur"]
    assert aux["cost_volume_processed"] is aux["propagation_weights"] or torch.equal(aux["cost_volume_processed"], aux["propagation_weights"])
    assert out["cost_volume"].shape == (B, H * W, H, W) and out["response"].shape == c["inp"]["dimp_score_cur"].shape
    got = KE.flat({"response": out["response"].cpu(), "state_cur": out["state_cur"].cpu(), "auxiliary_outputs": {k: v.cpu() for k, v in aux.items()}})
    assert sorted(got) == sorted(want)
    ref, pw = golden_outputs(g)
    assert float(g["thresh_margin"]) > 10 * 1e-4                   # no shifted score within the comparison tolerance of the threshold
    flat = {}
    for k, a in got.items():
        a = a.numpy()
        if k == "propagation_weights":
            assert a.shape == (B, H * W, 1, H, W)
            flat[k] = float(np.abs(a.reshape(-1) - pw["propagation_weights"].reshape(-1)).max() if "propagation_weights" in pw else
                            np.abs(a.reshape(-1)[pw["sample_idx"]] - pw["sample"]).max())
        else:
            assert a.shape == ref[k].shape, (k, a.shape, ref[k].shape)
            flat[k] = float(np.abs(a - ref[k]).max())
    print(f"\n{name}: max |gpu - reference fp32| per output: " + ", ".join(f"{k} {v:.2e}" for k, v in flat.items()))
    for k, w64 in want.items():
        ref_err = float(pw["ref_fp32_err"]) if k == "propagation_weights" else float(g["err_" + k])
        f64_bound.held(f"{name[8:]} {k}", got[k].numpy().reshape(w64.shape), w64, ref_err, factor=FACTOR, floor=f64_bound.ulp_of_max, table=TABLE)
    assert max(flat.values()) <= 1e-4, flat


@pytest.mark.parametrize("name", CASES)
def test_case_holds_float64_bound_reference_golden_and_repeats(name):
    g, c, _ = restated(name)
    w = kys_ent_modules.wrapper(c["sd"], c["conf"], c["md"], DEV)
    out = _run(w, c)
    _check(name, out)
    again = _run(w, c)
    for k in ("response", "state_cur", "cost_volume"):
        assert torch.equal(out[k], again[k]), k
    for k, v in out["auxiliary_outputs"].items():
        assert torch.equal(v, again["auxiliary_outputs"][k]), k


def test_closed_loop_follows_reference_trajectory():
    g = load("kys_ent_loop")
    B, C, H, W, md = (int(g[k]) for k in ("B", "C", "H", "W", "md"))
    w = kys_ent_modules.wrapper(KE.predictor_state(int(g["state_seed"]), "entropy"), "entropy", md, DEV, dimp_thresh=float(g["dimp_thresh"]))
    state, worst = None, 0.0
    for t in range(int(g["frames"])):
        cur, prev = synth.kys_features(int(g["seed"]) + t, B, C, H, W)
        inp = synth.kys_frame_inputs(int(g["seed"]) + 100 + t, B, H, W)
        data = {"feat1": dev(prev), "feat2": dev(cur), "dimp_score_cur": dev(inp["dimp_score_cur"]), "label_prev": dev(inp["label_prev"]),
                "state_prev": state}
        with torch.no_grad():
            out = K.predict_response(w, data, output_window=dev(inp["window"]))             # dimp_thresh: the module's own 0.05
        state = out["state_cur"]
        e = max(float(np.abs(out["response"].cpu().numpy() - g["response"][t]).max()), float(np.abs(state.cpu().numpy() - g["state_cur"][t]).max()))
        worst = max(worst, e)
        print(f"\nframe {t}: max |gpu - reference| = {e:.2e}")
        assert e <= 1e-4, (t, e)
    print(f"\nclosed loop: max |gpu - reference| over {int(g['frames'])} frames = {worst:.2e}")


def test_structures_off_the_list_are_refused():
    x = torch.zeros(1, 4, 5, 7, device=DEV)
    data = {"feat1": x, "feat2": x, "dimp_score_cur": x[:, :1], "label_prev": x[:, :1], "state_prev": None}
    with torch.no_grad():
        for conf in ("entropy", "max", "none"):
            assert K.covered_predict_response(kys_ent_modules.wrapper(KE.predictor_state(1310, conf), conf, 2, DEV), data)
        for conf, dims in (("entropy", (64, 32)), ("entropy", (16, 16)), ("max", (16, 16)), ("max", (32,))):
            odd = kys_ent_modules.wrapper(KE.predictor_state(1310, conf, dims), conf, 2, DEV, dims=dims)
            assert not K.covered_predict_response(odd, data), (conf, dims)
            with pytest.raises(NotImplementedError, match=r"\(16,\)"):
                K.predict_response(odd, data)
        assert K.covered_predict_response(kys_ent_modules.wrapper(KE.predictor_state(1310, "max", (64, 32)), "max", 2, DEV, dims=(64, 32)), data)
        w = kys_ent_modules.wrapper(KE.predictor_state(1310, "entropy"), "entropy", 2, DEV)
        assert not K.covered_predict_response(w, dict(data, feat1=[x]))                      # several reference frames: the reference's code
        assert not K.covered_predict_response(w.train(), data)


@pytest.mark.skipif(not ref_harness.available(), reason="reference bundle missing")
def test_reference_kysnet_of_the_train_setting_takes_the_fast_branch():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install()
    try:
        from ltr.models.kys.predictor_wrapper import PredictorWrapper
        from ltr.models.tracking.kysnet import kysnet_res50
        # ltr/train_settings/kys/kys.py:110-114 (init_gauss_sigma = output_sigma * feature_sz = 1/4 / 5 * 18); the backbone is not loaded
        net = kysnet_res50(backbone_pretrained=False, optim_iter=3, cv_kernel_size=3, cv_max_displacement=9, cv_stride=1, init_gauss_sigma=0.9,
                           train_feature_extractor=False, train_iounet=False, detach_length=0, state_dim=8,
                           representation_predictor_dims=(16,), conf_measure="entropy", dimp_thresh=0.05)
        w = net.predictor
        assert isinstance(w, PredictorWrapper) and w.predictor.dimp_thresh == 0.05
        name = "kys_ent_18x18_b"
        g, c, _ = restated(name)
        w.predictor.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["sd"].items()})
        w = w.to(DEV).eval()
        amd.stats.clear()
        out = _run(w, c)
        assert amd.stats["PredictorWrapper.predict_response.fast"] == 1 and amd.stats["PredictorWrapper.predict_response.reference"] == 0
        _check(name, out)
    finally:
        amd.uninstall()
