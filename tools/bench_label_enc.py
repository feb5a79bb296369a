"""Mask label encoder on one MI355X, per call, at 1 / 8 / 32 masks of 480 x 832 (lwl_ytvos.py: image_sample_size, sample_memory_size):
    python -B tools/bench_label_enc.py [--rounds N] [--out profiles/label_enc_bench.json]
  fused        pytracking_amd.label_encoder.forward (six launches, one C ABI call)
  stock        the same ResidualDS16SW (layer_dims (16, 32, 64, 16), use_bn=False) in stock PyTorch-ROCm on the same GPU (the reference's
               class from the reference tree or its bundle; a plain-torch module of the same layers when neither is there: `stock_kind`
               says which), eval, no_grad
Both variants of a size are interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.  Two
figures per variant: `device_us` = event-timed batch of 5 back-to-back calls / 5 (what the GPU spends), `host_us` = one call +
synchronisation, host clock (what a tracker that waits for the encodings sees).  Medians over the rounds."""
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

from pytracking_amd import label_encoder as LE, synth  # noqa: E402
import label_enc_cases as LC  # noqa: E402

DEV = "cuda:0"
BATCH = 5
H, W = 480, 832


def modules(sd):
    from oracle import ref_harness
    dims = synth.LABEL_ENC_DIMS
    if not ref_harness.available():
        cls, kind = LC.ResidualDS16SW, "plain-torch layers"
        nets = [cls(dims, False) for _ in range(2)]
    else:
        ref_harness.install()
        from ltr.models.lwl.label_encoder import ResidualDS16SW
        nets, kind = [ResidualDS16SW(layer_dims=dims, use_bn=False) for _ in range(2)], "reference ResidualDS16SW"
    for net in nets:
        net.load_state_dict(LC.state_tensors(sd))
        net.to(DEV).eval()
    return nets, kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_enc_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "H": H, "W": W,
           "layer_dims": list(synth.LABEL_ENC_DIMS), "cases": {}}
    (ours, ref), kind = modules(synth.label_enc_state(2105))
    with torch.no_grad():
        for n in (1, 8, 32):
            masks = torch.from_numpy(synth.label_enc_masks(2300 + n, n, H, W)).to(DEV)[:, None]
            assert LE.covered(ours, masks)
            variants = {"fused": lambda: LE.forward(ours, masks), "stock": lambda: ref(masks)}
            c, s = variants["fused"](), variants["stock"]()
            diff = max(float((c[0] - s[0]).abs().max()), float((c[1] - s[1]).abs().max()))
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
            out = {"n": n, "stock_kind": kind, "max_abs_fused_minus_stock": diff}
            for k in variants:
                out[k] = {"device_us": statistics.median(dev_t[k]), "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k])}
            out["stock_over_fused_device"] = out["stock"]["device_us"] / out["fused"]["device_us"]
            out["stock_over_fused_host"] = out["stock"]["host_us"] / out["fused"]["host_us"]
            res["cases"][f"n{n}"] = out
            print(f"n{n}", json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
