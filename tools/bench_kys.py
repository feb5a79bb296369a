"""KYS response prediction on one MI355X (host-timed medians after warm-up, one synchronisation per timed call):
    python -B tools/bench_kys.py [--reps N] [--out profiles/kys_bench.json]
  cost_volume          pytracking_amd.kys.cost_volume at 18 x 18 x 1024, md = 9 (remap fused)
  predict_response     the whole PredictorWrapper.predict_response through pytracking_amd.kys
  stock_*              the same two calls through the reference's own modules in stock PyTorch on the same GPU, with the plain-torch
                       STAND-IN sampler of tests/kys_standin.py under the name of the CUDA extension (the real one cannot exist here);
                       needs the reference tree or its bundle
Device time of the kernels: run this script under `rocprofv3 --kernel-trace --stats -- python -B tools/bench_kys.py` in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pytracking_amd import kys as K, synth  # noqa: E402
import kys_modules  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": statistics.median(ts), "min_us": min(ts), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kys_bench.json"))
    a = ap.parse_args()
    c = synth.KYS
    cur, prev = (torch.from_numpy(x).to(DEV) for x in synth.kys_features(1, 1, c["C"], c["H"], c["W"]))
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in synth.kys_frame_inputs(2, 1, c["H"], c["W"]).items()}
    data = {"feat1": prev, "feat2": cur, "dimp_score_cur": inp["dimp_score_cur"], "label_prev": inp["label_prev"], "state_prev": inp["state_prev"]}
    w = kys_modules.wrapper(3, "max", c["md"], DEV)
    res = {"device": torch.cuda.get_device_name(0), "shape": [1, c["C"], c["H"], c["W"]], "md": c["md"]}
    with torch.no_grad():
        res["cost_volume"] = timed(lambda: K.cost_volume(cur, prev, c["md"]), a.reps)
        res["predict_response"] = timed(lambda: K.predict_response(w, data, output_window=inp["window"]), a.reps)
        from oracle import ref_harness
        if ref_harness.available():
            ref_harness.install()
            import kys_standin
            kys_standin.register()
            from ltr.models.kys.cost_volume import CostVolume
            from ltr.models.kys.predictor_wrapper import PredictorWrapper
            from ltr.models.kys.response_predictor import ResponsePredictor
            pred = ResponsePredictor(conf_measure="max")
            pred.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.kys_predictor_state(3, "max").items()})
            ref = PredictorWrapper(CostVolume(3, c["md"], abs_coordinate_output=True), pred).to(DEV).eval()
            reps = max(3, a.reps // 10)
            res["stock_cost_volume_standin_sampler"] = timed(lambda: ref.cost_volume(cur, prev), reps, warmup=1)
            res["stock_predict_response_standin_sampler"] = timed(lambda: ref.predict_response(data, output_window=inp["window"]), reps, warmup=1)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
