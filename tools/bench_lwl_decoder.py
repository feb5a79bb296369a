"""Segmentation decoder on one MI355X, per call, at the deployed size (480 x 832 image, ResNet-50 layers 4..1, mdim 64, 16 score channels,
BatchNorm) and n = 1:
    python -B tools/bench_lwl_decoder.py [--rounds N] [--out profiles/lwl_decoder_bench.json]
  fused        pytracking_amd.lwl_decoder.forward (one C ABI call)
  stock        the same decoder in stock PyTorch-ROCm on the same GPU (the reference's LWTLDecoder from the reference tree or its bundle; a
               plain-torch module of the same layers when neither is there: `stock_kind` says which), eval, no_grad
Both variants are interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.  Per variant:
`device_us` = event pair around one call after warm-up (median and p95 over the rounds), `host_us` = one call + synchronisation on the host
clock, `launches` = kernels the profiler sees in one call.  `flops` = 2 * Cout * Cin * k * k * output positions summed over every
convolution the module runs (forward hooks on the stock run); `fraction_of_fp32_matrix_peak` = flops / device time / 157.3 TFLOP/s."""
import argparse
import json
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pytracking_amd import lwl_decoder as LD, synth  # noqa: E402
import lwl_decoder_cases as DC  # noqa: E402

DEV = "cuda:0"
PEAK_FP32_MATRIX = 157.3e12


def modules(c, sd):
    from oracle import ref_harness
    chans = OrderedDict((L, fc) for L, fc, _, _ in c["levels"])
    if not ref_harness.available():
        nets, kind = [DC.Decoder(c["ic"], c["mdim"], chans, c["use_bn"]) for _ in range(2)], "plain-torch layers"
    else:
        ref_harness.install()
        from ltr.models.lwl.decoder import LWTLDecoder
        nets, kind = [LWTLDecoder(c["ic"], c["mdim"], chans, use_bn=c["use_bn"]) for _ in range(2)], "reference LWTLDecoder"
    for net in nets:
        net.load_state_dict(DC.state_tensors(sd))
        net.to(DEV).eval()
    return nets, kind


def conv_flops(net, call):
    total = [0]

    def hook(m, inp, out):
        total[0] += 2 * out.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
    handles = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    call()
    for h in handles:
        h.remove()
    return total[0]


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if "kernel" in str(getattr(e, "device_type", "")).lower() or getattr(e, "device_time", 0) > 0)
    except Exception:                                                     # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lwl_decoder_bench.json"))
    a = ap.parse_args()
    g, c, sd, _, _ = DC.case("deployed")
    (ours, ref), kind = modules(c, sd)
    s, feats = DC.inputs("deployed", DEV)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "case": "deployed", "n": c["n"], "image": list(c["image"]),
           "mdim": c["mdim"], "ic": c["ic"], "stock_kind": kind}
    with torch.no_grad():
        assert LD.covered(ours, s, feats, c["image"])
        variants = {"fused": lambda: LD.forward(ours, s, feats, c["image"]), "stock": lambda: ref(s, feats, c["image"])}
        res["flops"] = conv_flops(ref, variants["stock"])
        res["max_abs_fused_minus_stock"] = float((variants["fused"]()[0] - variants["stock"]()[0]).abs().max())
        for fn in variants.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        dev_t, host_t = {k: [] for k in variants}, {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                dev_t[k].append(e0.elapsed_time(e1) * 1e3)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                host_t[k].append((time.perf_counter() - t0) * 1e6)
        for k, fn in variants.items():
            d = sorted(dev_t[k])
            res[k] = {"device_us": statistics.median(d), "device_us_p95": d[min(len(d) - 1, int(0.95 * len(d)))], "device_us_min": d[0],
                      "host_us": statistics.median(host_t[k]), "launches": launches(fn)}
            res[k]["fraction_of_fp32_matrix_peak"] = res["flops"] / (res[k]["device_us"] * 1e-6) / PEAK_FP32_MATRIX
        res["stock_over_fused_device"] = res["stock"]["device_us"] / res["fused"]["device_us"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
