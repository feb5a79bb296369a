"""Device time of the TaMOs multi-object filter predictor at the deployed case of tests/tamos_cases.py (24 x 36 maps, two memory frames
plus the test frame, 10 object queries, cls + bbreg rows: 5184 token rows), next to a stock-torch restatement of the same predictor
written here on nn.MultiheadAttention (the reference itself is not available where this runs).

    python tools/bench_tamos.py [--batches 8] [--out profiles/tamos_bench.json]
    python tools/bench_tamos.py --kernel-stats STATS.csv      # add per-kernel times from a separate `rocprofv3 --kernel-trace --stats`
                                                              # run of `python tools/bench_tamos.py --profile-run`

Timing: after warm-up the two implementations alternate in the same process; each sample is one event-timed batch of 20 calls, the record
holds the median per call.  GFLOP is counted here from the shapes (2 flops per multiply-add of every matrix product the reference
forms: token MLP, encoder, decoder with unfolded projections), launches per call come from pt_tamos_predict_routes."""
import argparse
import csv
import ctypes
import json
import os
import re
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tamos_cases as TC                       # noqa: E402
from pytracking_amd import _lib                # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.3                # MI355X, v_mfma_f32_16x16x4_f32
CALLS = 20
NEW_KERNELS = ("k_tamos_tokens", "k_tamos_box1", "k_tamos_self_attn", "k_tamos_xattn", "k_tamos_xmerge")


def gflop(cfg):
    D, ff, nh, T = cfg["D"], cfg["ff"], cfg["nhead"], cfg["T"]
    HW = cfg["H"] * cfg["W"]
    B = 2 if cfg["mode"] == "parallel" else cfg["n_seq"]
    Ltr, L = cfg["n_train"] * HW, (cfg["n_train"] + 1) * HW
    mac = B * Ltr * T * (4 * D // 4 + D // 4 * D + D * D)                           # box MLP per object
    mac += B * Ltr * T * D                                                           # label encoding
    enc = L * (3 * D * D + D * D + 2 * D * ff) + 2 * L * L * D                       # projections, FFN, QK^T and PV
    mac += cfg["n_enc"] * B * enc
    dec = T * (4 * D * D) + 2 * T * T * D + T * (2 * D * D) + 2 * L * D * D + 2 * T * L * D + 2 * T * D * ff
    mac += cfg["n_dec"] * B * dec
    return 2 * mac / 1e9


class StockPredictor(nn.Module):
    """GOTFilterPredictor ('gaussian', 'ltrb_token') + Transformer.forward restated on stock torch modules."""

    def __init__(self, cfg, params):
        super().__init__()
        D, nh, ff = cfg["D"], cfg["nhead"], cfg["ff"]
        self.cfg = cfg
        mk = lambda: nn.MultiheadAttention(D, nh, dropout=0.0)
        self.enc = nn.ModuleList([nn.ModuleDict(dict(sa=mk(), l1=nn.Linear(D, ff), l2=nn.Linear(ff, D), n1=nn.LayerNorm(D), n2=nn.LayerNorm(D)))
                                  for _ in range(cfg["n_enc"])])
        self.dec = nn.ModuleList([nn.ModuleDict(dict(sa=mk(), ca=mk(), l1=nn.Linear(D, ff), l2=nn.Linear(ff, D), n1=nn.LayerNorm(D),
                                                     n2=nn.LayerNorm(D), n3=nn.LayerNorm(D))) for _ in range(cfg["n_dec"])])
        self.norm = nn.LayerNorm(D)
        self.box = nn.Sequential(nn.Conv1d(4, D // 4, 1), nn.BatchNorm1d(D // 4), nn.ReLU(), nn.Conv1d(D // 4, D, 1), nn.BatchNorm1d(D),
                                 nn.ReLU(), nn.Conv1d(D, D, 1))
        self.E = nn.Parameter(torch.zeros(cfg["T"], D))
        t = lambda k: torch.from_numpy(params[k].copy())
        names = dict(sa="self_attn", ca="multihead_attn", l1="linear1", l2="linear2", n1="norm1", n2="norm2", n3="norm3")
        with torch.no_grad():
            for kind, layers in (("encoder", self.enc), ("decoder", self.dec)):
                for i, layer in enumerate(layers):
                    pre = f"fp.transformer.{kind}.layers.{i}."
                    for short, mod in layer.items():
                        for pn, p in mod.named_parameters():
                            p.copy_(t(pre + names[short] + "." + pn))
            self.norm.weight.copy_(t("fp.transformer.decoder.norm.weight"))
            self.norm.bias.copy_(t("fp.transformer.decoder.norm.bias"))
            for k, v in self.box.state_dict().items():
                if k.endswith("num_batches_tracked"):
                    continue
                v.copy_(t("fp.box_encoding." + k))
            self.E.copy_(t("fp.query_embed_fg.weight"))

    def forward(self, train_feat, test_feat, label, ltrb, pos, num_gth_frames):
        nf, ns, D, H, W = train_feat.shape
        T = self.E.shape[0]
        st = lambda a: torch.cat([a, a], dim=1)
        tr = st(train_feat).permute(1, 2, 0, 3, 4).flatten(2).permute(2, 0, 1)
        te = st(test_feat).permute(1, 2, 0, 3, 4).flatten(2).permute(2, 0, 1)
        lab = st(label).permute(1, 2, 0, 3, 4).flatten(2).permute(2, 0, 1)
        tr = tr + lab @ self.E
        lt = st(ltrb)
        enc = self.box(lt.permute(1, 2, 3, 0, 4, 5).reshape(2 * T, 4, nf * H * W)).reshape(2, T, D, nf * H * W)
        tr = tr + (enc * self.E.reshape(1, T, D, 1)).sum(dim=1).permute(2, 0, 1)
        x = torch.cat([tr, te], dim=0)
        L = x.shape[0]
        mask = torch.zeros(2, L, dtype=torch.bool, device=x.device)
        mask[1, num_gth_frames * H * W:L - H * W] = True
        for m in self.enc:
            qk = x + pos
            x = m["n1"](x + m["sa"](qk, qk, x, key_padding_mask=mask, need_weights=False)[0])
            x = m["n2"](x + m["l2"](Fn.relu(m["l1"](x))))
        qp = self.E[:, None, :].expand(T, 2, D)
        tgt = torch.zeros_like(qp)
        for m in self.dec:
            q = tgt + qp
            tgt = m["n1"](tgt + m["sa"](q, q, tgt, need_weights=False)[0])
            tgt = m["n2"](tgt + m["ca"](tgt + qp, x + pos, x, key_padding_mask=mask, need_weights=False)[0])
            tgt = m["n3"](tgt + m["l2"](Fn.relu(m["l1"](tgt))))
        return self.norm(tgt).transpose(0, 1), x[-H * W:].permute(1, 2, 0).reshape(2, D, H, W)


def setup(dev):
    cfg, params, inputs = TC.case(TC.DEPLOYED)
    pred, _ = TC.build_modules(cfg, params, dev)
    stock = StockPredictor(cfg, params).to(dev).eval()
    ins = [torch.from_numpy(a.copy()).to(dev) for a in inputs]
    pos = pred._pos_table(cfg["H"], cfg["W"], torch.device(dev)).repeat(cfg["n_train"] + 1, 1)[:, None, :]
    ours = lambda: pred.predict_cls_bbreg_filters_parallel(ins[0], ins[1], ins[2], cfg["num_gth_frames"], ins[3])
    theirs = lambda: stock(ins[0], ins[1], ins[2], ins[3], pos, cfg["num_gth_frames"])
    return cfg, ours, theirs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS


def kernel_stats(path):
    """{kernel: {calls, mean_us, total_us}} of the TaMOs launches, from rocprofv3's kernel stats CSV."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            m = re.search(r"(k_tamos_\w+(?:<\d+>)?)", name)
            if m and m.group(1).split("<")[0] in NEW_KERNELS:
                out[m.group(1)] = dict(calls=int(row["Calls"]), mean_us=round(float(row["AverageNs"]) / 1e3, 2),
                                       total_us=round(float(row["TotalDurationNs"]) / 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tamos_bench.json"))
    ap.add_argument("--profile-run", action="store_true", help="a few calls of the gfx950 path only (the program a profiler wraps)")
    ap.add_argument("--kernel-stats", help="kernel stats CSV of a separate rocprofv3 run to add to the record at --out")
    a = ap.parse_args()
    if a.kernel_stats:
        rec = json.load(open(a.out))
        rec["kernels"] = kernel_stats(a.kernel_stats)                # of --profile-run: 5 calls of the predictor
        json.dump(rec, open(a.out, "w"), indent=1)
        print(json.dumps(rec["kernels"]))
        return
    dev = "cuda:0"
    with torch.no_grad():
        cfg, ours, theirs = setup(dev)
        if a.profile_run:
            for _ in range(5):
                ours()
            torch.cuda.synchronize()
            return
        f_ours, f_theirs = ours(), theirs()
        diff = max(float((f_ours[0][0, :, :, 0, 0] - f_theirs[0][0]).abs().max()), float((f_ours[1][0, :, :, 0, 0] - f_theirs[0][1]).abs().max()))
        for _ in range(3):
            timed(ours), timed(theirs)
        t_ours, t_theirs = [], []
        for _ in range(a.batches):
            t_ours.append(timed(ours))
            t_theirs.append(timed(theirs))
    rc, routes = TC.case_routes(_lib.lib(), TC.DEPLOYED)
    assert rc == 0
    g = gflop(cfg)
    ms, ms_stock = statistics.median(t_ours), statistics.median(t_theirs)
    rec = dict(case=TC.DEPLOYED, cfg=cfg, calls_per_batch=CALLS, batches=a.batches, gfx950_ms=round(ms, 4), gfx950_ms_min_max=[round(min(t_ours), 4), round(max(t_ours), 4)],
               stock_torch_ms=round(ms_stock, 4), stock_torch_ms_min_max=[round(min(t_theirs), 4), round(max(t_theirs), 4)],
               speedup=round(ms_stock / ms, 3), launches_per_call=len(routes), gflop=round(g, 2), tflops=round(g / ms, 2),
               share_of_fp32_matrix_peak=round(g / ms / FP32_MATRIX_PEAK_TFLOPS, 4), filters_max_abs_diff_vs_stock=diff)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
