"""TEST INFRASTRUCTURE ONLY -- tests/golden/kys_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_kys.py
KYS response prediction (pytracking/tracker/kys/kys.py:314 -> ltr/models/kys).  `spatial_correlation_sampler` cannot be installed here:
tests/kys_standin.py (plain torch, the UNPINNED piece) is registered under its name before ltr.models.kys is imported.
  kys_cv_*     CostVolume(3, md, abs_coordinate_output=True / False) on synth.kys_features: seed + shape, the reference's fp32 output (a
               1000-entry sample of it at the deployed shape) and `ref_fp32_err` / `ref_fp32_err_disp`: the largest error of the reference's
               own fp32 CPU result against the float64 restatement (tests/kys_np.py), remapped / displacement form
  kys_pw_*     the propagation weights (= cost_volume_processed) of a size: they depend on the features and the two cost-volume stacks only
  kys_pred_*   PredictorWrapper.predict_response, eval mode: every output and auxiliary output except the propagation weights
  kys_loop     8 frames, 2 sequences, 18 x 18 x 1024, state_cur fed back
Weights: synth.kys_predictor_state (BatchNorm statistics away from their defaults); inputs: synth.kys_frame_inputs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()
import kys_standin  # noqa: E402

kys_standin.register()

from pytracking_amd import synth  # noqa: E402
import kys_np  # noqa: E402

OUT = os.environ.get("KYS_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
T = torch.from_numpy

CV_CASES = {      # name: (seed, B, C, H, W, md)
    "kys_cv_1x1": (1101, 1, 3, 1, 1, 1),
    "kys_cv_5x7": (1102, 2, 40, 5, 7, 2),
    "kys_cv_6x6": (1103, 1, 64, 6, 6, 9),
    "kys_cv_9x4": (1104, 1, 70, 9, 4, 3),
    "kys_cv_18x18": (1105, 1, 1024, 18, 18, 9),
}
SIZES = {"5x7": (2, 40, 5, 7, 2), "18x18": (1, 1024, 18, 18, 9)}      # B, C, H, W, md
VARIANTS = {      # name: (state_prev given, dimp_thresh set, output_window set, conf_measure)
    "a": (False, False, False, "max"),
    "b": (True, True, True, "max"),
    "c": (True, False, True, "none"),
    "d": (False, True, False, "none"),
}
THRESH_CANDIDATES = (0.05, 0.04, 0.06, 0.03, 0.07)
FEAT_SEED, STATE_SEED, INPUT_SEED = 1200, 1300, 1400
LOOP = dict(frames=8, B=2, C=1024, H=18, W=18, md=9, seed=1500)


def wrapper(conf_measure, md, seed=STATE_SEED):
    from ltr.models.kys.cost_volume import CostVolume
    from ltr.models.kys.predictor_wrapper import PredictorWrapper
    from ltr.models.kys.response_predictor import ResponsePredictor
    pred = ResponsePredictor(conf_measure=conf_measure)
    pred.load_state_dict({k: T(v.copy()) for k, v in synth.kys_predictor_state(seed, conf_measure).items()})
    return PredictorWrapper(CostVolume(3, md, abs_coordinate_output=True), pred).eval()


def make_cv():
    from ltr.models.kys.cost_volume import CostVolume
    for name, (seed, B, C, H, W, md) in CV_CASES.items():
        cur, prev = synth.kys_features(seed, B, C, H, W)
        with torch.no_grad():
            ref = CostVolume(3, md, abs_coordinate_output=True)(T(cur), T(prev)).numpy()
            ref_d = CostVolume(3, md, abs_coordinate_output=False)(T(cur), T(prev)).numpy()
        disp = kys_np.cost_volume(cur, prev, md, remap=False) if C * H * W < 100000 else kys_np.cost_volume_shifted(cur, prev, md)
        rem = kys_np.remap_cost_volume(disp)
        g = dict(seed=seed, shape=np.array([B, C, H, W]), md=md, ref_fp32_err=np.abs(ref - rem).max(), ref_fp32_err_disp=np.abs(ref_d - disp).max(),
                 max_abs=np.abs(rem).max())
        if ref.size <= 20000:
            g["out"], g["out_disp"] = ref, ref_d
        else:
            idx = np.random.default_rng(seed).choice(ref.size, 1000, replace=False)
            g["sample_idx"], g["sample"] = idx, ref.reshape(-1)[idx]
            idx_d = np.random.default_rng(seed + 1).choice(ref_d.size, 1000, replace=False)
            g["sample_idx_disp"], g["sample_disp"] = idx_d, ref_d.reshape(-1)[idx_d]
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **g)
        print(name, "ref_fp32_err", g["ref_fp32_err"], g["ref_fp32_err_disp"], "max |v|", g["max_abs"])


def run(w, cur, prev, inp, state, thresh, window):
    data = {"feat1": T(prev), "feat2": T(cur), "dimp_score_cur": T(inp["dimp_score_cur"]), "label_prev": T(inp["label_prev"]),
            "state_prev": None if state is None else T(state)}
    with torch.no_grad():
        return w.predict_response(data, dimp_thresh=thresh, output_window=None if window is None else T(window))


def make_pred():
    from ltr.models.kys.utils import shift_features
    for size, (B, C, H, W, md) in SIZES.items():
        cur, prev = synth.kys_features(FEAT_SEED, B, C, H, W)
        inp = synth.kys_frame_inputs(INPUT_SEED, B, H, W)
        # the thresholded scores are the SHIFTED ones: pick the candidate threshold farthest from any of them
        s = T(inp["dimp_score_cur"])
        shifted = shift_features(s.clone(), -torch.ones(B, 2) * 0.5 / torch.tensor([[W, H]]).float()).numpy()
        margins = [np.abs(shifted - t).min() for t in THRESH_CANDIDATES]
        thr, margin = THRESH_CANDIDATES[int(np.argmax(margins))], max(margins)
        assert margin > 1e-3, margin
        pw = None
        for v, (with_state, with_thr, with_win, conf) in VARIANTS.items():
            out = run(wrapper(conf, md), cur, prev, inp, inp["state_prev"] if with_state else None, thr if with_thr else None,
                      inp["window"] if with_win else None)
            aux = out["auxiliary_outputs"]
            assert aux["cost_volume_processed"].data_ptr() == aux["propagation_weights"].data_ptr()
            if pw is None:
                pw = aux["propagation_weights"].numpy().copy()
                np.savez_compressed(os.path.join(OUT, f"kys_pw_{size}.npz"), propagation_weights=pw)
            assert np.array_equal(pw, aux["propagation_weights"].numpy())
            g = dict(feat_seed=FEAT_SEED, state_seed=STATE_SEED, input_seed=INPUT_SEED, shape=np.array([B, C, H, W]), md=md,
                     with_state=with_state, with_thresh=with_thr, with_window=with_win, conf_measure=conf, dimp_thresh=thr,
                     thresh_margin=margin, aux_keys=np.array(sorted(aux.keys())), response=out["response"].numpy(),
                     state_cur=out["state_cur"].numpy())
            for k, t in aux.items():
                if k not in ("cost_volume_processed", "propagation_weights"):
                    g["aux_" + k] = t.numpy()
            np.savez_compressed(os.path.join(OUT, f"kys_pred_{size}_{v}.npz"), **g)
            print(f"kys_pred_{size}_{v}", "thr margin", margin, "response max", float(out["response"].max()), "pw max", float(pw.max()))


def make_loop():
    c = LOOP
    w = wrapper("max", c["md"])
    state, resp, states = None, [], []
    for t in range(c["frames"]):
        cur, prev = synth.kys_features(c["seed"] + t, c["B"], c["C"], c["H"], c["W"])
        inp = synth.kys_frame_inputs(c["seed"] + 100 + t, c["B"], c["H"], c["W"])
        out = run(w, cur, prev, inp, state, None, inp["window"])
        state = out["state_cur"].numpy()
        resp.append(out["response"].numpy())
        states.append(state)
    np.savez_compressed(os.path.join(OUT, "kys_loop.npz"), state_seed=STATE_SEED, response=np.stack(resp), state_cur=np.stack(states),
                        **{k: v for k, v in c.items()})
    print("kys_loop", np.stack(resp).shape, "response max per frame", [float(r.max()) for r in resp])


if __name__ == "__main__":
    what = sys.argv[1:] or ["cv", "pred", "loop"]
    if "cv" in what:
        make_cv()
    if "pred" in what:
        make_pred()
    if "loop" in what:
        make_loop()
