"""LWL / RTS feature heads on one MI355X, per call, at the two deployed shapes (lwl_net.py:173-177, rts_net.py:294-298, 339-344):
    python -B tools/bench_feat_head.py [--rounds N] [--out profiles/feat_head_bench.json]
  target_model  1 x 1024 x 30 x 52 -> 512 x 30 x 52, stride 1 (pt_clf_head_f32 through features.residual_basic_block)
  classifier    1 x 1024 x 30 x 52 -> 512 x 15 x 26, stride 2 (pt_feat_head_f32 through features.residual_bottleneck)
  fused         the ClfHead module, one C ABI call
  stock         nn.Sequential(Conv2d(1024, 512, 3, stride, padding=1, bias=False), InstanceL2Norm) with the same weight in stock
                PyTorch-ROCm on the same GPU, eval, no_grad (the norm is the expression of ltr/models/layers/normalization.py:15-18)
Both variants of a shape are interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.  Two
figures per variant: `device_us` = event-timed batch of 10 back-to-back calls / 10 (what the GPU spends), `host_us` = one call +
synchronisation, host clock.  Medians over the rounds.  `tflops` = 2 * 9 * Cin * Cout * Ho * Wo over device_us: the convolution's
arithmetic over the time of the whole head (token transposes, reduction and normalisation included)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytracking_amd import features as FM, synth  # noqa: E402

DEV = "cuda:0"
BATCH = 10
SCALE = 0.0147                                 # sqrt(1 / (512 * 3 * 3)): lwl_net.py:171


class StockNorm(torch.nn.Module):
    def __init__(self, scale, eps=1e-5):
        super().__init__()
        self.scale, self.eps = scale, eps

    def forward(self, input):
        return input * (self.scale * ((input.shape[1] * input.shape[2] * input.shape[3]) / (
            torch.sum((input * input).view(input.shape[0], 1, 1, -1), dim=3, keepdim=True) + self.eps)).sqrt())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feat_head_bench.json"))
    a = ap.parse_args()
    n, Cin, Cout, H, W = synth.FEAT_HEAD_DEPLOYED
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "shape": [n, Cin, H, W], "Cout": Cout, "cases": {}}
    xs, w = synth.feat_head_problem(2500, n, Cin, Cout, H, W)
    x, w = torch.from_numpy(xs).to(DEV), torch.from_numpy(w)
    with torch.no_grad():
        for name, stride in (("target_model", 1), ("classifier", 2)):
            if stride == 1:
                ours = FM.residual_basic_block(feature_dim=Cin, num_blocks=0, l2norm=True, final_conv=True, norm_scale=SCALE, out_dim=Cout)
            else:
                ours = FM.residual_bottleneck(feature_dim=Cout, num_blocks=0, l2norm=True, final_conv=True, norm_scale=SCALE, out_dim=Cout,
                                              input_dim=Cin, final_stride=2)
            ours.load_state_dict({"0.weight": w.clone()})
            ours.to(DEV).eval()
            stock = torch.nn.Sequential(torch.nn.Conv2d(Cin, Cout, 3, stride=stride, padding=1, bias=False), StockNorm(SCALE))
            stock.load_state_dict({"0.weight": w.clone()})
            stock.to(DEV).eval()
            variants = {"fused": lambda: ours(x), "stock": lambda: stock(x)}
            c, s = variants["fused"](), variants["stock"]()
            diff = float((c - s).abs().max())
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
            gflop = 2 * 9 * Cin * Cout * c.shape[-2] * c.shape[-1] * n / 1e9
            out = {"stride": stride, "out_shape": list(c.shape), "GFLOP": gflop, "max_abs_fused_minus_stock": diff,
                   "max_abs_out": float(s.abs().max())}
            for k in variants:
                d = statistics.median(dev_t[k])
                out[k] = {"device_us": d, "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k]), "tflops": gflop / d * 1e3}
            out["stock_over_fused_device"] = out["stock"]["device_us"] / out["fused"]["device_us"]
            res["cases"][name] = out
            print(name, json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
