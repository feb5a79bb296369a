"""Device time of the TaMOs heads at the deployed cases of tests/tamos_heads_cases.py -- the box regressor on 10 objects' attended copies
of a 256 x 48 x 72 map (34 560 token rows per tower layer) and the two-level FPN from 512 x 48 x 72 and 256 x 24 x 36 -- by three routes
in one run:

    gfx950      pt_tamos_bbreg_f32 / pt_fpn2_f32 through pytracking_amd.tamos (the direct 3x3 token convolution)
    stock       a stock PyTorch-ROCm restatement of the reference's sequence (heads.py:119-162) written here on nn.Conv2d / nn.GroupNorm /
                F.interpolate (the reference itself is not available where this runs)
    per_tap     the parent commit's route to the regressor's numbers: T calls of pt_tomp_bbreg_f32 with n = 1 on the same map, one per
                object's filter (nine per-tap partial products per convolution, summed by k_gn_reduce)

    python tools/bench_tamos_heads.py [--batches 8] [--out profiles/tamos_heads_bench.json]

Timing: after warm-up the routes alternate in the same process; each sample is one event-timed batch of CALLS calls, the record holds the
median per call and the spread.  GFLOP is counted from the shapes (2 flops per multiply-add of every product the reference forms)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tamos_heads_cases as HC                 # noqa: E402
import tomp_cases as TPC                       # noqa: E402
from pytracking_amd import _lib                # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.3                # MI355X, v_mfma_f32_16x16x4_f32
CALLS = 10


def reg_gflop(n_img, T, D, H, W):
    HW = H * W
    mac = n_img * T * D * D + n_img * HW * D * T + n_img * T * HW * (4 * 9 * D * D + 9 * D * 4)
    return 2 * mac / 1e9


def fpn_gflop(n, C_hi, C_lo, D, H3, W3, H2, W2):
    mac = n * (H2 * W2 * (C_hi * D + 9 * D * D) + H3 * W3 * (C_lo * D + 9 * D * D))
    return 2 * mac / 1e9


class StockRegressor(nn.Module):
    def __init__(self, D, params):
        super().__init__()
        self.linear = nn.Linear(D, D)
        layers = []
        for _ in range(4):
            layers += [nn.Conv2d(D, D, 3, padding=1), nn.GroupNorm(1, D), nn.ReLU(inplace=True)]
        self.tower = nn.Sequential(*layers)
        self.bbreg_layer = nn.Conv2d(D, 4, 3, padding=1)
        self.load_state_dict(HC.to_sd(params), strict=True)

    def forward(self, feat, filt):                                  # feat (n, D, H, W), filt (n, T, D)
        n, D, H, W = feat.shape
        att = torch.einsum("nchw,ntc->nthw", feat, self.linear(filt))
        x = (feat.unsqueeze(1) * att.unsqueeze(2)).reshape(-1, D, H, W)
        return torch.exp(self.bbreg_layer(self.tower(x))).reshape(n, -1, 4, H, W)


class StockFPN(nn.Module):
    def __init__(self, C_hi, C_lo, D, params):
        super().__init__()
        self.i0, self.i1 = nn.Conv2d(C_hi, D, 1), nn.Conv2d(C_lo, D, 1)
        self.l0, self.l1 = nn.Conv2d(D, D, 3, padding=1), nn.Conv2d(D, D, 3, padding=1)
        with torch.no_grad():
            for m, k in ((self.i0, "inner_blocks.0"), (self.i1, "inner_blocks.1"), (self.l0, "layer_blocks.0"), (self.l1, "layer_blocks.1")):
                m.weight.copy_(torch.from_numpy(params[f"fpn.{k}.0.weight"].copy()))
                m.bias.copy_(torch.from_numpy(params[f"fpn.{k}.0.bias"].copy()))

    def forward(self, hi, lo):
        lat3 = self.i1(lo)
        lat2 = self.i0(hi) + Fn.interpolate(lat3, size=hi.shape[-2:], mode="nearest")
        return self.l0(lat2), self.l1(lat3)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tamos_heads_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    dv = lambda x: torch.from_numpy(x.copy()).to(dev)
    n_img, T, D, H, W = HC.REG[HC.REG_DEPLOYED]
    rp, feat, filt = HC.reg_case(HC.REG_DEPLOYED)
    fp, hi, lo = HC.fpn_case(HC.FPN_DEPLOYED)
    n, C_hi, C_lo, Df, H3, W3, H2, W2 = HC.FPN[HC.FPN_DEPLOYED]
    with torch.no_grad():
        reg = HC.build_regressor(D, rp, dev)
        single = TPC.build_regressor(D, {"reg." + k: v for k, v in rp.items()}, dev)
        stock_reg = StockRegressor(D, rp).to(dev).eval()
        fpn = HC.build_fpn(HC.FPN_DEPLOYED, fp, dev)
        stock_fpn = StockFPN(C_hi, C_lo, Df, fp).to(dev).eval()
        f5, w5, f4, w3 = dv(feat)[None], dv(filt).reshape(n_img, T, D, 1, 1), dv(feat), dv(filt)
        one = [w3[0, o].reshape(1, D, 1, 1).contiguous() for o in range(T)]
        enc, back, hi_d, lo_d = dv(lo)[None], {"layer2": dv(hi)}, dv(hi), dv(lo)
        routes = dict(
            regressor_gfx950=lambda: reg(f5, w5),
            regressor_stock_torch=lambda: stock_reg(f4, w3),
            regressor_per_tap=lambda: [single(f5, one[o]) for o in range(T)],
            fpn_gfx950=lambda: fpn(enc, back),
            fpn_stock_torch=lambda: stock_fpn(hi_d, lo_d))
        ours, theirs, taps = routes["regressor_gfx950"](), routes["regressor_stock_torch"](), routes["regressor_per_tap"]()
        diffs = dict(regressor_vs_stock=float((ours[0] - theirs).abs().max()),
                     regressor_vs_per_tap=max(float((ours[0, 0, o] - taps[o][0, 0]).abs().max()) for o in range(T)),
                     fpn_vs_stock=float((routes["fpn_gfx950"]()["feat2"][0] - routes["fpn_stock_torch"]()[0]).abs().max()))
        for _ in range(2):
            for fn in routes.values():
                timed(fn)
        t = {k: [] for k in routes}
        for _ in range(a.batches):
            for k, fn in routes.items():
                t[k].append(timed(fn))
    L = _lib.lib()
    gr, gf = reg_gflop(n_img, T, D, H, W), fpn_gflop(n, C_hi, C_lo, Df, H3, W3, H2, W2)
    rec = dict(regressor_case=HC.REG_DEPLOYED, fpn_case=HC.FPN_DEPLOYED, calls_per_batch=CALLS, batches=a.batches,
               regressor_gflop=round(gr, 2), fpn_gflop=round(gf, 2), max_abs_diff=diffs,
               regressor_launches=len(HC.reg_routes(L, n_img, T, D, H, W)[1]), per_tap_launches=T * len(TPC.bbreg_routes(L, 1, D, H, W)[1]),
               fpn_launches=len(HC.case_routes(L, HC.FPN_DEPLOYED)[1]))
    for k, v in t.items():
        ms = statistics.median(v)
        g = gr if k.startswith("regressor") else gf
        rec[k] = dict(ms=round(ms, 4), ms_min_max=[round(min(v), 4), round(max(v), 4)], tflops=round(g / ms, 2),
                      share_of_fp32_matrix_peak=round(g / ms / FP32_MATRIX_PEAK_TFLOPS, 4))
    rec["regressor_speedup_vs_stock"] = round(rec["regressor_stock_torch"]["ms"] / rec["regressor_gfx950"]["ms"], 3)
    rec["regressor_speedup_vs_per_tap"] = round(rec["regressor_per_tap"]["ms"] / rec["regressor_gfx950"]["ms"], 3)
    rec["fpn_speedup_vs_stock"] = round(rec["fpn_stock_torch"]["ms"] / rec["fpn_gfx950"]["ms"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
