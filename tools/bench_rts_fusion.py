"""RTS instance-score encoder and learners fusion on one MI355X, per call, at the deployed size (16 x 27 score map -> 30 x 52 mask encoding,
layer dims (16, 32, 64, 16), 16 filters; rts50.py):
    python -B tools/bench_rts_fusion.py [--rounds N] [--out profiles/rts_fusion_bench.json]
  encoder      pytracking_amd.rts_fusion.encode without sample_w, as the tracker uses it (six launches)     vs  the module's forward
  fuse_add     pytracking_amd.rts_fusion.fuse, 'add' (one launch)                                           vs  interpolate + LearnersFusion
  fuse_concat  pytracking_amd.rts_fusion.fuse, 'concat' (one launch)                                        vs  interpolate + LearnersFusion
  chain_add / chain_concat   the encoder, then the fuse
`stock` is the same modules in stock PyTorch-ROCm on the same GPU, eval, no_grad: the reference's classes from the reference tree or its
bundle, plain-torch modules of the same layers when neither is there (`stock_kind` says which).  Both variants of a case are interleaved in
ONE process: every round times each once, so clock and thermal drift hit them alike.  Two figures per variant: `device_us` = event-timed
batch of 20 back-to-back calls / 20 (what the GPU spends), `host_us` = one call + synchronisation, host clock (what a tracker that waits
for the decoder input sees).  Medians over the rounds."""
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

from pytracking_amd import rts_fusion as RF, synth  # noqa: E402
import rts_fusion_cases as RC  # noqa: E402

DEV = "cuda:0"
BATCH = 20


def modules(sd_enc, sd_concat, dims):
    """({name: module} for the fused side, the same for the stock side, the stock side's resize, what the stock side is)."""
    from oracle import ref_harness
    f = dims[3]
    if not ref_harness.available():
        kind, resize = "plain-torch layers", RC.resize
        make = lambda: {"enc": RC.ResidualDS16SW_Clf(dims, False), "add": RC.LearnersFusion("add", f), "concat": RC.LearnersFusion("concat", f)}  # noqa: E731
    else:
        ref_harness.install()
        from ltr.models.rts.label_encoder import ResidualDS16SW_Clf
        from ltr.models.rts.learners_fusion import LearnersFusion
        from ltr.models.rts.utils import interpolate as resize
        kind = "reference ResidualDS16SW_Clf / LearnersFusion"
        make = lambda: {"enc": ResidualDS16SW_Clf(layer_dims=dims, use_bn=False), "add": LearnersFusion("add"), "concat": LearnersFusion("concat")}  # noqa: E731
    sides = []
    for _ in range(2):
        nets = make()
        nets["enc"].load_state_dict(RC.state_tensors(sd_enc))
        nets["concat"].load_state_dict(RC.state_tensors(sd_concat))
        sides.append({k: m.to(DEV).eval() for k, m in nets.items()})
    return sides[0], sides[1], resize, kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rts_fusion_bench.json"))
    a = ap.parse_args()
    c = synth.RTS_CHAIN_CASE
    dims, f = c["dims"], c["dims"][3]
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "score_map": [c["H"], c["W"]],
           "target": list(c["target"]), "layer_dims": list(dims), "cases": {}}
    ours, ref, resize, kind = modules(synth.label_enc_state(2605, dims, False), synth.learners_fusion_state(2805, f, "concat"), dims)
    scores = torch.from_numpy(synth.score_maps(2705, 1, c["H"], c["W"])).to(DEV)[None]
    seg, clf = [torch.from_numpy(t).to(DEV) for t in synth.learners_fuse_inputs(2905, 1, f, (c["H"], c["W"]), c["target"])]

    def stock_fuse(k, enc):
        return ref[k](seg, resize(enc[0, :, :, :, :], seg.shape[-2:]).unsqueeze(0))

    cases = {"encoder": (lambda: RF.encode(ours["enc"], scores, want_sample_w=False)[0], lambda: ref["enc"](scores)[0])}
    for k in ("add", "concat"):
        cases["fuse_" + k] = (lambda k=k: RF.fuse(ours[k], seg, clf), lambda k=k: stock_fuse(k, clf))
        cases["chain_" + k] = (lambda k=k: RF.fuse(ours[k], seg, RF.encode(ours["enc"], scores, want_sample_w=False)[0]),
                               lambda k=k: stock_fuse(k, ref["enc"](scores)[0]))
    with torch.no_grad():
        assert RF.encoder_covered(ours["enc"], scores) and all(RF.fuse_covered(ours[k], seg, clf) for k in ("add", "concat"))
        for name, (fused, stock) in cases.items():
            variants = {"fused": fused, "stock": stock}
            diff = float((fused() - stock()).abs().max())
            for fn in variants.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            dev_t, host_t = {k: [] for k in variants}, {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(BATCH):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    dev_t[k].append(e0.elapsed_time(e1) * 1e3 / BATCH)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    host_t[k].append((time.perf_counter() - t0) * 1e6)
            out = {"stock_kind": kind, "max_abs_fused_minus_stock": diff}
            for k in variants:
                out[k] = {"device_us": statistics.median(dev_t[k]), "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k])}
            out["stock_over_fused_device"] = out["stock"]["device_us"] / out["fused"]["device_us"]
            out["stock_over_fused_host"] = out["stock"]["host_us"] / out["fused"]["host_us"]
            res["cases"][name] = out
            print(name, json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
