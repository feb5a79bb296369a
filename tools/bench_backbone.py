"""Measurement of the ResNet backbone forward on the MI355X (needs a GPU):

    python -B tools/bench_backbone.py [--batches 20] [--batch 10] [--rows r50_288,...] [--out profiles/backbone_bench.json]

One process, the two variants alternating call by call (host clock) and batch by batch (device events), medians with quartiles.  Per row:
  fused   pytracking_amd.backbone.forward(module, x, outputs): libpt_bbn.so
  stock   the same module -- the same Conv2d / BatchNorm2d / ReLU / MaxPool2d objects with the same seeded parameters -- called layer by
          layer in stock PyTorch-ROCm as ResNet.forward calls them (MIOpen convolutions, eval BatchNorm, in-place ReLU and add)
  event_us   device events around a batch of calls, per call: what the stream is busy for, launch gaps included
  host_us    host clock of one call with the device synchronised before and after
  launches   launches of the fused call (pt_bbn_plan)
  gflop      2 M N K over the call's convolutions (the stem with its 147 real K), tflops = gflop / event_us, peak_frac = tflops / 157.3
The rows are the deployed backbones (ResNet-50 to layer3 at 288, 352, 384x576; the mrcnn ResNet-50 at 480x832; ResNet-18 and ResNet-101 at
288) and the DiMP-50 first-frame batch of 13 images.  The file is rewritten behind every row.  Nothing here promises a speed-up: rows that
lose are reported as they are."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import backbone_np as RN  # noqa: E402
from pytracking_amd import _lib_bbn as K  # noqa: E402
from pytracking_amd import backbone as B  # noqa: E402

DEV = "cuda:0"
PEAK_TFLOPS = 157.3
R50, R18, R101 = [3, 4, 6, 3], [2, 2, 2, 2], [3, 4, 23, 3]
L23 = ["layer2", "layer3"]
# name: kind, blocks, mrcnn, input shape, outputs, the trackers
ROWS = {
    "r50_288": ("Bottleneck", R50, False, (1, 3, 288, 288), L23, "DiMP-50 / ToMP / KYS / KeepTrack"),
    "r50_352": ("Bottleneck", R50, False, (1, 3, 352, 352), L23, "PrDiMP-50"),
    "r50_384x576": ("Bottleneck", R50, False, (1, 3, 384, 576), L23, "TaMOs"),
    "r50_mrcnn_480x832": ("Bottleneck", R50, True, (1, 3, 480, 832), ["conv1", "layer1", "layer2", "layer3"], "LWL / RTS"),
    "r18_288": ("BasicBlock", R18, False, (1, 3, 288, 288), L23, "ATOM"),
    "r101_288": ("Bottleneck", R101, False, (1, 3, 288, 288), L23, "ToMP-101"),
    "r50_288_n13": ("Bottleneck", R50, False, (13, 3, 288, 288), L23, "DiMP-50 first-frame batch"),
}


def seeded_module(spec, outputs, seed):
    """the stand-in with parameters in the ranges of tests/backbone_cases.params, drawn on the device"""
    m = RN.ResNet(spec, outputs).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for name, mod in m.named_modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.normal_(0, (2.0 / (mod.kernel_size[0] * mod.kernel_size[1] * mod.out_channels)) ** 0.5, generator=g)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                last = name.endswith("bn3") or (spec["kind"] == "BasicBlock" and name.endswith("bn2"))
                mod.weight.uniform_(*((0.1, 0.4) if last else (0.5, 1.5)), generator=g)
                mod.bias.normal_(0, 0.1, generator=g)
                mod.running_mean.normal_(0, 0.1, generator=g)
                mod.running_var.uniform_(0.5, 1.5, generator=g)
    return m


def stock_forward(m, x, outputs, after_pool):
    """ResNet.forward of either reference file on the module's own layers"""
    out = {}
    x = m.relu(m.bn1(m.conv1(x)))
    if not after_pool and "conv1" in outputs:
        out["conv1"] = x
    x = m.maxpool(x)
    if after_pool and "conv1" in outputs:
        out["conv1"] = x
    for name in ("layer1", "layer2", "layer3", "layer4"):
        if len(out) == len(outputs):
            break
        for blk in getattr(m, name):
            res = x if blk.downsample is None else blk.downsample(x)
            y = blk.relu(blk.bn1(blk.conv1(x)))
            if hasattr(blk, "conv3"):
                y = blk.bn3(blk.conv3(blk.relu(blk.bn2(blk.conv2(y)))))
            else:
                y = blk.bn2(blk.conv2(y))
            y += res
            x = blk.relu(y)
        if name in outputs:
            out[name] = x
    return out


def quartiles(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"q1": round(float(q[0]), 1), "median": round(float(q[1]), 1), "q3": round(float(q[2]), 1)}


def bench_row(name, batches, batch):
    kind, blocks, mrcnn, shape, outputs, trackers = ROWS[name]
    spec = dict(kind=kind, blocks=blocks, inplanes=64, mrcnn=mrcnn)
    m = seeded_module(spec, outputs, 7)
    x = torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    rows = B.plan(m, shape, outputs)
    convs = [r for r in rows if r.kernel in (K.PT_BBN_K_CONV, K.PT_BBN_K_STEM)]
    gflop = sum(2.0 * r.M * r.N * (147 if r.kernel == K.PT_BBN_K_STEM else r.K) for r in convs) / 1e9
    calls = {"fused": lambda: B.forward(m, x, outputs), "stock": lambda: stock_forward(m, x, outputs, mrcnn)}
    with torch.no_grad():
        assert B.covered(m, x, outputs)
        a, b = calls["fused"](), calls["stock"]()
        agree = {o: float((a[o] - b[o]).abs().max()) for o in outputs}
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        host, ev = {v: [] for v in calls}, {v: [] for v in calls}
        for _ in range(batches):
            for v, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                host[v].append((time.perf_counter() - t0) * 1e6)
        for _ in range(batches):
            for v, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(batch):
                    fn()
                e1.record()
                e1.synchronize()
                ev[v].append(e0.elapsed_time(e1) * 1e3 / batch)
    res = {"trackers": trackers, "shape": list(shape), "outputs": outputs, "convolutions": len(convs), "launches": len(rows), "gflop": round(gflop, 2),
           "routes": {K.ROUTES[r]: sum(q.route == r for q in rows) for r in sorted({q.route for q in rows})},
           "max_abs_difference_fused_stock": agree}
    for v in calls:
        us = quartiles(ev[v])
        res[v] = {"event_us": us, "host_us": quartiles(host[v]), "tflops": round(gflop * 1e3 / us["median"], 2),
                  "peak_frac": round(gflop * 1e3 / us["median"] / PEAK_TFLOPS, 3)}
    res["stock_over_fused"] = round(res["stock"]["event_us"]["median"] / res["fused"]["event_us"]["median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_bench.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batches": args.batches, "batch": args.batch,
           "peak_tflops": PEAK_TFLOPS, "rows": {}}
    for name in args.rows.split(","):
        out["rows"][name] = r = bench_row(name, args.batches, args.batch)
        print(f"{name:20s} {r['gflop']:6.2f} GFLOP  fused {r['fused']['event_us']['median']:8.1f} us ({r['launches']} launches, "
              f"{r['fused']['tflops']:5.1f} TFLOP/s)  stock {r['stock']['event_us']['median']:8.1f} us  stock/fused {r['stock_over_fused']:.2f}", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
