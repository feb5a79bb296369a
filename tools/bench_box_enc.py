"""Box label encoders on one MI355X, per call, at the deployed sizes (image 480 x 832, feature 512 x 30 x 52):
    python -B tools/bench_box_enc.py [--rounds N] [--out profiles/box_enc_bench.json]
  box          ResidualDS16FeatSWBox, layer_dims (16, 32, 64, 128, 16), one box (STANet.label_encoder / RTSNet.box_label_encoder)
  box_pair     both encoders of an STANet back to back on the same box and feature (label_encoder, then bbox_encoder)
  cat          ResidualDS16FeatSWBoxCatMultiBlock, layer_dims (64, 64, 16), BatchNorm (lwl_boxinit)
  fused        pytracking_amd.box_encoder.forward
  stock        the same module in stock PyTorch-ROCm on the same GPU (the reference's class from the reference tree or its bundle; the
               plain-torch stand-in of tests/box_enc_cases.py, which rasterises on the host, when neither is there: `stock_kind` says
               which), eval, no_grad.  The reference reads every box on the host (`int(bb)`), so a stock call synchronises.
Both variants of a case are interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.
`device_us` = event-timed batch of 20 back-to-back calls / 20, `host_us` = one call + synchronisation on the host clock.  Medians over the
rounds.  There is no threshold: the figures are reported whichever way they fall."""
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

from pytracking_amd import box_encoder as BE  # noqa: E402
import box_enc_cases as BC  # noqa: E402

DEV = "cuda:0"
BATCH = 20


def stock_module(kind, c, sd):
    from oracle import ref_harness
    if not ref_harness.available():
        net, what = BC.build(kind, c), "plain-torch stand-in (host rasteriser)"
    else:
        ref_harness.install()
        from ltr.models.lwl import label_encoder as M
        kw = dict(layer_dims=c["dims"], feat_dim=c["feat_dim"], use_final_relu=c["final_relu"], use_gauss=False, use_bn=c["use_bn"])
        net = (M.ResidualDS16FeatSWBox(use_sample_w=c["use_sample_w"], **kw) if kind == BC.BOX
               else M.ResidualDS16FeatSWBoxCatMultiBlock(final_bn=c["final_bn"], **kw))
        what = "reference " + type(net).__name__
    net.load_state_dict(BC.state_tensors(sd))
    return net.to(DEV).eval(), what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_enc_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "cases": {}}
    with torch.no_grad():
        for tag, kind, copies in (("box", BC.BOX, 1), ("box_pair", BC.BOX, 2), ("cat", BC.CAT, 1)):
            _, c, sd, boxes, feat = BC.case(kind, "deployed")
            args = BC.call_args(kind, c, boxes, feat, DEV)
            ours = [BC.module(kind, "deployed", DEV) for _ in range(copies)]
            stock, what = zip(*[stock_module(kind, c, sd) for _ in range(copies)])
            assert all(BE.covered(net, *args) for net in ours)
            variants = {"fused": lambda: [BE.forward(net, *args) for net in ours], "stock": lambda: [net(*args) for net in stock]}
            got, want = variants["fused"]()[0], variants["stock"]()[0]
            got, want = (got, want) if kind == BC.BOX else ((got,), (want,))
            diff = max(float((g - w).abs().max()) for g, w in zip(got, want))
            for fn in variants.values():
                for _ in range(3):
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
            out = {"n": c["n"], "image": list(c["image"]), "feat": [c["feat_dim"], *c["feat"]], "layer_dims": list(c["dims"]),
                   "encoders_per_call": copies, "stock_kind": what[0], "max_abs_fused_minus_stock": diff}
            for k in variants:
                out[k] = {"device_us": statistics.median(dev_t[k]), "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k])}
            out["stock_over_fused_device"] = out["stock"]["device_us"] / out["fused"]["device_us"]
            out["stock_over_fused_host"] = out["stock"]["host_us"] / out["fused"]["host_us"]
            res["cases"][tag] = out
            print(tag, json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
