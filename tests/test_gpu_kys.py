"""KYS response prediction on the MI355X (kys.hip through pytracking_amd.kys): the cost volume in both output forms against the float64
restatement (tests/kys_np.py) within 4x the reference's own fp32 error (stored in the goldens), exact structured probes, the predictor
against the goldens of the unmodified reference (tools/make_golden_kys.py) within 1e-4 on every output and auxiliary output, an 8-frame
closed loop, and the reference's kysnet modules through install().

Every test prints its measured maximum error before it asserts (run with -s)."""
import os

import numpy as np
import pytest
import torch

import kys_modules
import kys_np
import f64_bound
from f64_bound import dev
from oracle import ref_harness
from pytracking_amd import kys as K, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
CV = ["kys_cv_1x1", "kys_cv_5x7", "kys_cv_6x6", "kys_cv_9x4", "kys_cv_18x18"]
PRED = [f"kys_pred_{s}_{v}" for s in ("5x7", "18x18") for v in "abcd"]
_REF = {}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _cv_reference(name):
    """float64 displacement and remapped forms of a cost-volume case, computed once per session."""
    if name not in _REF:
        g = _load(name)
        B, C, H, W = (int(v) for v in g["shape"])
        cur, prev = synth.kys_features(int(g["seed"]), B, C, H, W)
        disp = kys_np.cost_volume(cur, prev, int(g["md"]), remap=False) if "out" in g else kys_np.cost_volume_shifted(cur, prev, int(g["md"]))
        _REF[name] = (g, cur, prev, disp, kys_np.remap_cost_volume(disp))
    return _REF[name]


@pytest.mark.parametrize("remap", [True, False])
@pytest.mark.parametrize("name", CV)
def test_cost_volume_matches_float64(name, remap):
    g, cur, prev, disp, rem = _cv_reference(name)
    out = K.cost_volume(dev(cur), dev(prev), int(g["md"]), remap=remap).cpu().numpy()
    want = rem if remap else disp
    assert out.shape == want.shape
    err, bound = np.abs(out - want).max(), f64_bound.bound(g["ref_fp32_err" if remap else "ref_fp32_err_disp"])
    print(f"\n{name} remap={remap}: max |gpu - float64| = {err:.3e}, bound 4 x ref_fp32_err = {bound:.3e}")
    assert err <= bound
    layer = K.CostVolume(3, int(g["md"]), abs_coordinate_output=remap)
    assert torch.equal(layer(dev(cur), dev(prev)), torch.from_numpy(out).to(DEV))     # the module form, and bit-identical repeats


def test_cost_volume_one_hot_probe():
    H, W, md = 5, 6, 2
    cur, prev = np.zeros((1, 2, H, W), np.float32), np.zeros((1, 2, H, W), np.float32)
    cur[0, 1, 2, 3], prev[0, 1, 3, 2] = 2.0, 3.0
    want = np.zeros((H, W, H, W), np.float32)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            want[3 - i, 2 - j, 2 - i, 3 - j] = 6.0
    out = K.cost_volume(dev(cur), dev(prev), md).cpu().numpy().reshape(H, W, H, W)
    np.testing.assert_array_equal(out, want)
    raw = K.SpatialCorrelationSampler(3, 2 * md + 1, 1, 1)(dev(cur), dev(prev)).cpu().numpy()
    assert raw.shape == (1, 5, 5, H, W)
    np.testing.assert_array_equal(raw, kys_np.cost_volume(cur, prev, md, remap=False).reshape(raw.shape))


def test_cost_volume_constant_map_border_counts():
    ones = np.ones((1, 1, 4, 4), np.float32)
    rem = K.cost_volume(dev(ones), dev(ones), 1).cpu().numpy().reshape(4, 4, 4, 4)
    assert rem[0, 0, 0, 0] == 4 and rem[0, 1, 0, 1] == 6 and rem[1, 1, 1, 1] == 9 and rem[3, 3, 3, 3] == 4
    assert rem[0, 0, 1, 1] == 4 and rem[3, 3, 0, 0] == 0
    np.testing.assert_array_equal(rem.reshape(1, 16, 4, 4), kys_np.cost_volume(ones, ones, 1))
    disp = K.cost_volume(dev(ones), dev(ones), 1, remap=False).cpu().numpy()
    np.testing.assert_array_equal(disp, kys_np.cost_volume(ones, ones, 1, remap=False))   # centres outside the map keep their inside taps
    assert disp[0, 0, 0, 0] == 1                                                               # displacement (-1, -1) at the corner: one tap


def _compare(out, g, name):
    worst = {}

    def check(key, got, want):
        got = got.cpu().numpy()
        assert got.shape == want.shape, (key, got.shape, want.shape)
        worst[key] = float(np.abs(got - want).max())

    check("response", out["response"], g["response"])
    check("state_cur", out["state_cur"], g["state_cur"])
    aux = out["auxiliary_outputs"]
    assert sorted(aux) == list(g["aux_keys"])
    pw = _load("kys_pw_" + name.split("_")[2])["propagation_weights"]
    for k in g["aux_keys"]:
        check(k, aux[k], pw if k in ("cost_volume_processed", "propagation_weights") else g["aux_" + k])
    print(f"\n{name}: max |gpu - reference fp32| per output: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-4, worst


@pytest.mark.parametrize("name", PRED)
def test_predictor_matches_reference_golden(name):
    g = _load(name)
    B, C, H, W = (int(v) for v in g["shape"])
    cur, prev = synth.kys_features(int(g["feat_seed"]), B, C, H, W)
    inp = synth.kys_frame_inputs(int(g["input_seed"]), B, H, W)
    conf = str(g["conf_measure"])
    w = kys_modules.wrapper(int(g["state_seed"]), conf, int(g["md"]), DEV)
    data = {"feat1": dev(prev), "feat2": dev(cur), "dimp_score_cur": dev(inp["dimp_score_cur"]), "label_prev": dev(inp["label_prev"]),
            "state_prev": dev(inp["state_prev"]) if g["with_state"] else None}
    assert float(g["thresh_margin"]) > 10 * 1e-4                   # no shifted score within the comparison tolerance of the threshold
    with torch.no_grad():
        out = K.predict_response(w, data, dimp_thresh=float(g["dimp_thresh"]) if g["with_thresh"] else None,
                                 output_window=dev(inp["window"]) if g["with_window"] else None)
    assert out["cost_volume"].shape == (B, H * W, H, W)
    _compare(out, g, name)


def test_closed_loop_follows_reference_trajectory():
    g = _load("kys_loop")
    B, C, H, W, md = (int(g[k]) for k in ("B", "C", "H", "W", "md"))
    w = kys_modules.wrapper(int(g["state_seed"]), "max", md, DEV)
    state, worst = None, 0.0
    for t in range(int(g["frames"])):
        cur, prev = synth.kys_features(int(g["seed"]) + t, B, C, H, W)
        inp = synth.kys_frame_inputs(int(g["seed"]) + 100 + t, B, H, W)
        data = {"feat1": dev(prev), "feat2": dev(cur), "dimp_score_cur": dev(inp["dimp_score_cur"]), "label_prev": dev(inp["label_prev"]),
                "state_prev": state}
        with torch.no_grad():
            out = K.predict_response(w, data, output_window=dev(inp["window"]))
        state = out["state_cur"]
        e = max(float(np.abs(out["response"].cpu().numpy() - g["response"][t]).max()), float(np.abs(state.cpu().numpy() - g["state_cur"][t]).max()))
        worst = max(worst, e)
        assert e <= 1e-4, (t, e)
    print(f"\nclosed loop: max |gpu - reference| over {int(g['frames'])} frames = {worst:.2e}")


def test_weight_pack_follows_in_place_updates_and_dims_are_refused():
    w = kys_modules.wrapper(1300, "max", 2, DEV)
    p1 = K.packed_weights(w.predictor)
    assert K.packed_weights(w.predictor) is p1
    with torch.no_grad():
        w.predictor.state_predictor.conv_state_new.bias.add_(1.0)
    p2 = K.packed_weights(w.predictor)
    assert p2 is not p1 and float((p2[-8:] - p1[-8:]).mean()) == pytest.approx(1.0)
    odd = kys_modules.Wrapper(K.CostVolume(3, 2, abs_coordinate_output=True), kys_modules.Predictor("max", state_dim=8, dims=(32, 32))).to(DEV).eval()
    x = torch.zeros(1, 4, 5, 7, device=DEV)
    data = {"feat1": x, "feat2": x, "dimp_score_cur": x[:, :1], "label_prev": x[:, :1], "state_prev": None}
    assert not K.covered_predict_response(w, data)               # grad enabled and the parameters require it: the reference's autograd path
    with torch.no_grad():
        assert K.covered_predict_response(w, data)
        assert not K.covered_predict_response(odd, data)
        with pytest.raises(NotImplementedError):
            K.predict_response(odd, data)
        ent = kys_modules.wrapper(1300, "max", 2, DEV)
        ent.predictor.conf_measure = "entropy"
        assert not K.covered_predict_response(ent, data)
        assert not K.covered_predict_response(w, dict(data, feat1=[x]))                      # several reference frames: the reference's code
        assert not K.covered_predict_response(w.train(), data)


@pytest.mark.skipif(not ref_harness.available(), reason="reference bundle missing")
def test_reference_kysnet_modules_through_install():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install()
    try:
        from ltr.models.kys.cost_volume import CostVolume
        from ltr.models.kys.predictor_wrapper import PredictorWrapper
        from ltr.models.kys.response_predictor import ResponsePredictor
        name = "kys_pred_5x7_b"
        g = _load(name)
        B, C, H, W = (int(v) for v in g["shape"])
        pred = ResponsePredictor(conf_measure="max")
        pred.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.kys_predictor_state(int(g["state_seed"]), "max").items()})
        w = PredictorWrapper(CostVolume(3, int(g["md"]), abs_coordinate_output=True), pred).to(DEV).eval()
        cur, prev = synth.kys_features(int(g["feat_seed"]), B, C, H, W)
        inp = synth.kys_frame_inputs(int(g["input_seed"]), B, H, W)
        data = {"feat1": dev(prev), "feat2": dev(cur), "dimp_score_cur": dev(inp["dimp_score_cur"]), "label_prev": dev(inp["label_prev"]),
                "state_prev": dev(inp["state_prev"])}
        amd.stats.clear()
        with torch.no_grad():
            out = w.predict_response(data, dimp_thresh=float(g["dimp_thresh"]), output_window=dev(inp["window"]))
            cv = w.cost_volume(dev(cur), dev(prev))
        assert amd.stats["PredictorWrapper.predict_response.fast"] == 1 and amd.stats["PredictorWrapper.predict_response.reference"] == 0
        assert amd.stats["CostVolume.forward.fast"] == 1
        assert torch.equal(cv, out["cost_volume"])
        _compare(out, g, name)
        # grad enabled with parameters that require it: the reference's own predictor code, on the gfx950 cost volume
        out2 = w.predict_response(data, dimp_thresh=float(g["dimp_thresh"]), output_window=dev(inp["window"]))
        assert amd.stats["PredictorWrapper.predict_response.reference"] == 1 and amd.stats["CostVolume.forward.fast"] == 2
        assert float(np.abs(out2["response"].detach().cpu().numpy() - g["response"]).max()) <= 1e-4
    finally:
        amd.uninstall()
