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
  kys_ent_*    (`ent`, `ent_loop`: written only when asked for, and only these files) the trained structure of ltr/train_settings/kys/kys.py:110-114,
               ResponsePredictor(representation_predictor_dims=(16,), conf_measure='entropy'): per case the reference's fp32 outputs and
               `err_<output>`, the reference's own fp32 distance (8 threads) from the float64 restatement tests/kys_entropy_np.py;
               kys_ent_pw_*  the propagation weights of a size and gain (a 20000-entry sample of them above that size);
               kys_ent_loop  8 frames, 2 sequences, dimp_thresh 0.05, state_cur fed back
  tracker_kys  (`tracker`) the unmodified pytracking.tracker.kys.kys.KYS on CPU without install() (tests/kys_tracker.py): initialize() and 6
               track() calls, its boundary calls event by event
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


# ---------------------------------------------------------------------------------------------------------------------------
# the trained structure: one 16-wide representation layer, entropy confidence
ENT_SIZES = {"1x1": (1, 8, 1, 1, 1), "4x4": (1, 16, 4, 4, 2), "5x7": (2, 40, 5, 7, 2), "20x20": (1, 16, 20, 20, 3),
             "18x18": (1, 1024, 18, 18, 9)}                            # B, C, H, W, md
SHARP_GAIN = 30.0                                                      # raise it if a size misses the entropy-range condition below
ENT_VARIANTS = {      # name: (state_prev given, dimp_thresh set, output_window set, conf_measure, gain of the propagation softmax)
    "a": (False, False, False, "entropy", 1.0),
    "b": (True, True, True, "entropy", 1.0),
    "s": (False, True, True, "entropy", SHARP_GAIN),
}
FLAT_GAIN = 0.05                                                       # 4 x 4 at gain 1 stays below 0.9 ln(HW): a near-uniform softmax there
ENT_EXTRA = {"4x4": {"f": (True, False, False, "entropy", FLAT_GAIN)},
             "5x7": {"m": (True, False, True, "max", 1.0), "n": (False, True, False, "none", 1.0)}}
ENT_FEAT_SEED, ENT_STATE_SEED, ENT_INPUT_SEED = 1210, 1310, 1410
ENT_LOOP = dict(frames=8, B=2, C=1024, H=18, W=18, md=9, seed=1600, dimp_thresh=0.05)
PW_FULL = 20000


def ent_wrapper(conf_measure, md, sd, dimp_thresh=None):
    from ltr.models.kys.cost_volume import CostVolume
    from ltr.models.kys.predictor_wrapper import PredictorWrapper
    from ltr.models.kys.response_predictor import ResponsePredictor
    pred = ResponsePredictor(representation_predictor_dims=(16,), conf_measure=conf_measure, dimp_thresh=dimp_thresh)
    pred.load_state_dict({k: T(v.copy()) for k, v in sd.items()})
    return PredictorWrapper(CostVolume(3, md, abs_coordinate_output=True), pred).eval()


def _threads8(fn):
    import f64_bound
    ambient = torch.get_num_threads()
    torch.set_num_threads(f64_bound.THREADS)
    try:
        return fn()
    finally:
        torch.set_num_threads(ambient)


def make_ent():
    import kys_entropy_np as KE
    from ltr.models.kys.utils import shift_features
    for size, (B, C, H, W, md) in ENT_SIZES.items():
        inp = synth.kys_frame_inputs(ENT_INPUT_SEED, B, H, W)
        s = T(inp["dimp_score_cur"])
        shifted = shift_features(s.clone(), -torch.ones(B, 2) * 0.5 / torch.tensor([[W, H]]).float()).numpy()
        margins = [np.abs(shifted - t).min() for t in THRESH_CANDIDATES]                       # the margin rule of make_pred
        thr, margin = THRESH_CANDIDATES[int(np.argmax(margins))], max(margins)
        assert margin > 1e-3, margin
        lo, hi, pws = np.inf, -np.inf, {}
        for v, (with_state, with_thr, with_win, conf, gain) in {**ENT_VARIANTS, **ENT_EXTRA.get(size, {})}.items():
            per_seq = bool(B > 1 and v == "b")
            g = dict(feat_seed=ENT_FEAT_SEED, state_seed=ENT_STATE_SEED, input_seed=ENT_INPUT_SEED, shape=np.array([B, C, H, W]), md=md,
                     with_state=with_state, with_thresh=with_thr, with_window=with_win, window_per_seq=per_seq, conf_measure=conf,
                     rep_dims=np.array([16]), gain=gain, dimp_thresh=thr, thresh_margin=margin)
            c = KE.case(g)
            w = ent_wrapper(conf, md, c["sd"])
            out = _threads8(lambda: run(w, c["cur"], c["prev"], c["inp"], c["state"], c["thresh"], c["window"]))
            aux = out["auxiliary_outputs"]
            assert aux["cost_volume_processed"].data_ptr() == aux["propagation_weights"].data_ptr()
            want = KE.flat(KE.restate(c))
            got = KE.flat({"response": out["response"], "state_cur": out["state_cur"], "auxiliary_outputs": aux})
            assert sorted(got) == sorted(want)
            g["aux_keys"] = np.array(sorted(aux.keys()))
            g["response"], g["state_cur"] = out["response"].numpy(), out["state_cur"].numpy()
            for k, t in got.items():
                a = t.numpy()
                e = float(np.abs(a.astype(np.float64).reshape(want[k].shape) - want[k]).max())
                if k == "propagation_weights":
                    tag = size + ("" if gain == 1.0 else "_sharp" if gain > 1.0 else "_flat")
                    if tag not in pws:
                        pw = dict(ref_fp32_err=e, gain=gain, numel=a.size)
                        if a.size <= PW_FULL:
                            pw["propagation_weights"] = a
                        else:
                            pw["sample_idx"] = np.sort(np.random.default_rng(ENT_STATE_SEED).choice(a.size, PW_FULL, replace=False))
                            pw["sample"] = a.reshape(-1)[pw["sample_idx"]]
                        np.savez_compressed(os.path.join(OUT, f"kys_ent_pw_{tag}.npz"), **pw)
                        pws[tag] = a.copy()
                    assert np.array_equal(pws[tag], a)
                    g["pw"] = tag
                elif k not in ("response", "state_cur"):
                    g["aux_" + k] = a
                g["err_" + k] = e
            if conf == "entropy":
                pc = want["propagation_conf"]
                lo, hi = min(lo, pc.min()), max(hi, pc.max())
            np.savez_compressed(os.path.join(OUT, f"kys_ent_{size}_{v}.npz"), **g)
            print(f"kys_ent_{size}_{v}", "thr", thr, "margin", float(margin), "response max", float(out["response"].max()),
                  "errs", {k[4:]: float(f"{val:.2e}") for k, val in g.items() if k.startswith("err_")})
        lnhw = np.log(H * W)
        print(f"kys_ent_{size}: float64 entropy spans {lo:.4g} .. {hi:.4g} of ln(HW) = {lnhw:.4g}")
        assert H * W == 1 or (lo < 0.25 * lnhw and hi > 0.9 * lnhw), "raise SHARP_GAIN (low side) or add a flat variant (high side)"


def make_ent_loop():
    import kys_entropy_np as KE
    c = ENT_LOOP
    w = ent_wrapper("entropy", c["md"], KE.predictor_state(ENT_STATE_SEED, "entropy"), dimp_thresh=c["dimp_thresh"])
    state, resp, states = None, [], []
    for t in range(c["frames"]):
        cur, prev = synth.kys_features(c["seed"] + t, c["B"], c["C"], c["H"], c["W"])
        inp = synth.kys_frame_inputs(c["seed"] + 100 + t, c["B"], c["H"], c["W"])
        out = run(w, cur, prev, inp, state, None, inp["window"])                              # dimp_thresh: the module's own 0.05
        state = out["state_cur"].numpy()
        resp.append(out["response"].numpy())
        states.append(state)
    np.savez_compressed(os.path.join(OUT, "kys_ent_loop.npz"), state_seed=ENT_STATE_SEED, response=np.stack(resp), state_cur=np.stack(states),
                        **{k: v for k, v in c.items()})
    print("kys_ent_loop", np.stack(resp).shape, "response max per frame", [float(r.max()) for r in resp])


def make_tracker():
    import kys_tracker as KT
    boxes, rec, _ = KT.run_cpu_reference()
    path = os.path.join(OUT, "tracker_kys.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    kinds = [e["kind"] for e in rec.events]
    print(f"tracker_kys: {len(kinds)} events ({ {k: kinds.count(k) for k in sorted(set(kinds))} }), {os.path.getsize(path) / 1024:.1f} KiB, last box",
          boxes[-1])


if __name__ == "__main__":
    what = sys.argv[1:] or ["cv", "pred", "loop"]
    if "cv" in what:
        make_cv()
    if "pred" in what:
        make_pred()
    if "loop" in what:
        make_loop()
    if "ent" in what:
        make_ent()
    if "ent_loop" in what:
        make_ent_loop()
    if "tracker" in what:
        make_tracker()
