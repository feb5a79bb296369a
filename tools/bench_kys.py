"""KYS response prediction on one MI355X at the deployed size (1 x 1024 x 18 x 18, max displacement 9):
    python -B tools/bench_kys.py [--rounds N] [--out profiles/kys_bench.json]
  cost_volume                     pytracking_amd.kys.cost_volume (remap fused), two launches
  predict_response_16_entropy     the whole PredictorWrapper.predict_response through pytracking_amd.kys (cost volume + four launches) for the
                                  trained structure: representation_predictor_dims (16,), conf_measure 'entropy', dimp_thresh 0.05
  predict_response_64_32_max      the same call for the constructor defaults (64, 32) / 'max'
  stock_predict_response_*        the reference's own PredictorWrapper.predict_response / ResponsePredictor.forward in stock PyTorch on the
                                  same GPU, on THIS project's cost volume (the CUDA sampler extension cannot exist here); needs the reference
                                  tree or its bundle
All rows run interleaved in one process: every round times each row once, as one batch of back-to-back calls between two device events
(device time of the batch / calls in it; the host only enqueues inside a batch), and a row's figure is the median over the rounds.  No
threshold is asserted anywhere.  Kernel times: run this script under `rocprofv3 --kernel-trace --stats -- python -B tools/bench_kys.py`
in a run of its own."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pytracking_amd import kys as K, synth  # noqa: E402
import kys_ent_modules  # noqa: E402

DEV = "cuda:0"
STRUCTURES = {"16_entropy": ((16,), "entropy", 0.05), "64_32_max": ((64, 32), "max", None)}     # name: (dims, conf_measure, dimp_thresh)


def batch_us(fn, calls):
    """device time per call of `calls` back-to-back calls, in microseconds"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def interleaved(rows, rounds, warmup=3):
    """rows: {name: (fn, calls per batch)} -> {name: {median_us, min_us, max_us, rounds, calls_per_batch}}"""
    for fn, _ in rows.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in rows}
    for r in range(rounds):
        for name in (list(rows) if r % 2 == 0 else list(rows)[::-1]):
            fn, calls = rows[name]
            ts[name].append(batch_us(fn, calls))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": rounds, "calls_per_batch": rows[name][1]}
            for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kys_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_kys.py measures on the GPU; there is none here")
    c = synth.KYS
    cur, prev = (torch.from_numpy(x).to(DEV) for x in synth.kys_features(1, 1, c["C"], c["H"], c["W"]))
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in synth.kys_frame_inputs(2, 1, c["H"], c["W"]).items()}
    data = {"feat1": prev, "feat2": cur, "dimp_score_cur": inp["dimp_score_cur"], "label_prev": inp["label_prev"], "state_prev": inp["state_prev"]}
    res = {"device": torch.cuda.get_device_name(0), "shape": [1, c["C"], c["H"], c["W"]], "md": c["md"],
           "timing": "device events around batches of back-to-back calls, rows interleaved per round, median over rounds"}
    rows = {"cost_volume": (lambda: K.cost_volume(cur, prev, c["md"]), 20)}
    states = {}
    for name, (dims, conf, thresh) in STRUCTURES.items():
        states[name] = synth.kys_predictor_state(3, conf, rep_dims=dims)
        w = kys_ent_modules.wrapper(states[name], conf, c["md"], DEV, dims=dims, dimp_thresh=thresh)
        with torch.no_grad():
            assert K.covered_predict_response(w, data, None, inp["window"]), name     # the fused route, not a hand-back
        rows["predict_response_" + name] = (lambda w=w: K.predict_response(w, data, output_window=inp["window"]), 20)
    from oracle import ref_harness
    if ref_harness.available():
        ref_harness.install()
        import kys_standin
        kys_standin.register()                                 # only so that ltr.models.kys imports; the cost volume below is this project's
        from ltr.models.kys.predictor_wrapper import PredictorWrapper
        from ltr.models.kys.response_predictor import ResponsePredictor
        for name, (dims, conf, thresh) in STRUCTURES.items():
            pred = ResponsePredictor(representation_predictor_dims=dims, conf_measure=conf, dimp_thresh=thresh)
            pred.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in states[name].items()})
            ref = PredictorWrapper(K.CostVolume(3, c["md"], abs_coordinate_output=True), pred).to(DEV).eval()
            rows["stock_predict_response_" + name] = (lambda ref=ref: ref.predict_response(data, output_window=inp["window"]), 3)
    with torch.no_grad():
        res.update(interleaved(rows, a.rounds))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
