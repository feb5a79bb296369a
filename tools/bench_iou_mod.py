"""IoU modulation vectors on one MI355X, per call, at the three deployed cases (DiMP-50, PrDiMP-50, ATOM ResNet-18):
    python -B tools/bench_iou_mod.py [--rounds N] [--out profiles/iou_mod_bench.json]
  fused            pytracking_amd.iou_mod.get_modulation (windowed convolutions, poolings and the linear tail; one C ABI call, 4 launches)
  stock            AtomIoUNet.get_modulation restated in stock PyTorch-ROCm on the same GPU: the five nn.Sequential blocks of the same
                   state (whole-map MIOpen convolutions) with pytracking_amd.prroi_pool for the pooling, so that both sides pool on the
                   same kernel; eval, no_grad
  stock_convs      conv3_1r and conv4_1r of `stock` alone: what the whole-map convolutions cost there
  fused_whole_map  the fused call with every box replaced by the whole image: each window is the whole map, every workgroup of the grid
                   live -- what the fused convolution costs when the window saves nothing
(A whole-map convolution of ONE layer through pt_iou_feat_f32 is not expressible: that call always runs two layers per tower and n <= 8.)
All variants of a case are interleaved in ONE process: every round times each variant once, so clock and thermal drift hit them alike.
Two figures per variant: `device_us` = event-timed batch of 20 back-to-back calls / 20 (what the GPU spends), `host_us` = one call +
synchronisation, host clock (what init_iou_net waits for).  Medians over the rounds, and the least device figure."""
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

from pytracking_amd import iou_mod as IM, prroi_pool  # noqa: E402
import iou_mod_cases as IC  # noqa: E402

DEV = "cuda:0"
BATCH = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iou_mod_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "cases": {}}
    with torch.no_grad():
        for name in IC.DEPLOYED:
            g, n, l3, l4, dims, sd, (f3, f4, bb) = IC.case(name)
            feats = [torch.from_numpy(f.copy()).to(DEV) for f in (f3, f4)]
            boxes = torch.from_numpy(bb.copy()).to(DEV)
            whole = torch.tensor([[0.0, 0.0, 8.0 * l3[2], 8.0 * l3[1]]] * n, device=DEV)
            net = IC.module(name, DEV, pool=prroi_pool.prroi_pool2d)
            assert IM.covered(net, feats, boxes)
            variants = {"fused": lambda: IM.get_modulation(net, feats, boxes), "stock": lambda: net.get_modulation(feats, boxes),
                        "stock_convs": lambda: (net.conv3_1r(feats[0]), net.conv4_1r(feats[1])),
                        "fused_whole_map": lambda: IM.get_modulation(net, feats, whole)}
            c, s = variants["fused"](), variants["stock"]()
            diff = max(float((c[0] - s[0]).abs().max()), float((c[1] - s[1]).abs().max()))
            cw, sw = variants["fused_whole_map"](), net.get_modulation(feats, whole)
            diff_whole = max(float((cw[0] - sw[0]).abs().max()), float((cw[1] - sw[1]).abs().max()))
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
            wins = [[IM.window(b, sc, l[1], l[2]) for b in bb] for sc, l in ((IC.S3, l3), (IC.S4, l4))]
            out = {"n": n, "level3": list(l3), "level4": list(l4), "dims": list(dims),
                   "window_pixels": [sum((w[2] - w[0] + 1) * (w[3] - w[1] + 1) for w in lv if w is not None) for lv in wins],
                   "map_pixels": [n * l3[1] * l3[2], n * l4[1] * l4[2]],
                   "max_abs_fused_minus_stock": diff, "max_abs_fused_minus_stock_whole_map": diff_whole}
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
