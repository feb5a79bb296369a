"""IoU feature extraction on one MI355X, per call, at the three deployed cases (DiMP-50, PrDiMP-50, ATOM ResNet-18):
    python -B tools/bench_iou_feat.py [--rounds N] [--out profiles/iou_feat_bench.json]
  fused        pytracking_amd.iou_feat.get_iou_feat (both towers, one C ABI call)
  stock        the reference's AtomIoUNet.get_iou_feat in stock PyTorch-ROCm on the same GPU (module from the reference tree or its bundle; a
               plain-torch module of the same four blocks when neither is there: `stock_kind` says which), eval, no_grad
  tower3/4     the fused call with the OTHER tower shrunk to 64 -> 16 -> 16 on a 1 x 1 map (the C ABI always runs both)
All variants of a case are interleaved in ONE process: every round times each variant once, so clock and thermal drift hit them alike.
Two figures per variant: `device_us` = event-timed batch of 10 back-to-back calls / 10 (what the GPU spends), `host_us` = one call +
synchronisation, host clock (what a tracker that waits for the features sees).  Medians over the rounds."""
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

from pytracking_amd import iou_feat as IF, synth  # noqa: E402
import iou_feat_cases as IC  # noqa: E402

DEV = "cuda:0"
BATCH = 10


def reference_module(t3, t4, sd):
    from oracle import ref_harness
    if not ref_harness.available():
        net, kind = IC.Towers(t3, t4), "plain-torch blocks"
    else:
        ref_harness.install()
        from ltr.models.bbreg.atom_iou_net import AtomIoUNet
        net, kind = AtomIoUNet(input_dim=(t3[0], t4[0]), pred_input_dim=(t3[2], t4[2])), "reference AtomIoUNet"
    net.load_state_dict(IC.state_tensors(sd), strict=False)
    return net.to(DEV).eval(), kind


def one_tower(t, other_first, sd_seed, n):
    """(module, feats) of the fused call with tower `t` at full size and the other one at 64 -> 16 -> 16 @ 1 x 1."""
    tiny = (64, 16, 16, 1, 1)
    t3, t4 = (tiny, t) if other_first else (t, tiny)
    net = IC.Towers(t3, t4)
    net.load_state_dict(IC.state_tensors(synth.iou_feat_state(sd_seed, t3[0], t4[0], t3[1], t3[2], t4[1], t4[2])))
    feats = [torch.from_numpy(f).to(DEV) for f in synth.iou_feat_inputs(sd_seed + 1, n, t3[0], t3[3], t3[4], t4[0], t4[3], t4[4])]
    return net.to(DEV).eval(), feats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iou_feat_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "cases": {}}
    with torch.no_grad():
        for name in IC.DEPLOYED:
            g, n, t3, t4, sd, feats = IC.case(name)
            feats = [torch.from_numpy(f).to(DEV) for f in feats]
            ours = IC.module(name, DEV)
            ref, kind = reference_module(t3, t4, sd)
            n3, f3 = one_tower(t3, False, 11, n)
            n4, f4 = one_tower(t4, True, 13, n)
            variants = {"fused": lambda: IF.get_iou_feat(ours, feats), "stock": lambda: ref.get_iou_feat(feats),
                        "tower3": lambda: IF.get_iou_feat(n3, f3), "tower4": lambda: IF.get_iou_feat(n4, f4)}
            c, s = variants["fused"](), variants["stock"]()
            diff = max(float((c[0] - s[0]).abs().max()), float((c[1] - s[1]).abs().max()))
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
            out = {"n": n, "tower3": list(t3), "tower4": list(t4), "stock_kind": kind, "max_abs_fused_minus_stock": diff}
            for k in variants:
                out[k] = {"device_us": statistics.median(dev_t[k]), "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k])}
            out["stock_over_fused_device"] = out["stock"]["device_us"] / out["fused"]["device_us"]
            out["stock_over_fused_host"] = out["stock"]["host_us"] / out["fused"]["host_us"]
            res["cases"][name] = out
            print(name, json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
