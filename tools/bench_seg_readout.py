"""Segmentation read-out and object merge on one MI355X, per call, at deployed sizes:
    python -B tools/bench_seg_readout.py [--rounds N] [--out profiles/seg_readout_bench.json]
  readout_480x854 / readout_720x1280   pytracking_amd.seg_readout.crop_to_image (480 x 832 crop scores -> score, probability and mask
                                       image + statistics; two launches)                    vs  the reference's sequence in stock torch
  merge_n1 / merge_n3 / merge_n6       pytracking_amd.seg_readout.merge at 480 x 854 (probabilities, label map, per-object statistics; two
                                       launches)                                             vs  the reference's sequence in stock torch
`stock` restates what the reference trackers run -- convert_scores_crop_to_image, `> 0`, sigmoid and get_target_state
(pytracking/tracker/lwl/lwl.py:276-359); merge_results' soft aggregation, arg-max and one get_target_state per object (lwl.py:228-269) --
with stock PyTorch-ROCm operators on the SAME GPU (the trackers themselves run these stages on the CPU).  It is this project's own
restatement: it reads no reference file.  Both variants of a case are interleaved in ONE process: every round times each once, so clock
and thermal drift hit them alike.  Two figures per variant: `device_us` = event-timed batch of 20 back-to-back calls / 20 (what the GPU
spends), `host_us` = one call + synchronisation, host clock.  Medians over the rounds.  `bytes` is what the fused call must move (inputs
read once, outputs written once), `fused_GBps` that over `device_us`."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pytracking_amd import seg_readout as SR  # noqa: E402
import seg_readout_cases as SC  # noqa: E402

DEV = "cuda:0"
BATCH = 20
CROP = (480, 832)
READOUTS = {"readout_480x854": ((480, 854), 0.83, (236.3, 430.6)), "readout_720x1280": ((720, 1280), 1.31, (350.4, 600.7))}
MERGES = {"merge_n1": 1, "merge_n3": 3, "merge_n6": 6}
MERGE_HW = (480, 854)


def target_state(prob):
    """get_target_state (lwl.py:285-298) on the device: five reductions."""
    H, W = prob.shape
    ay, ax = torch.arange(H, dtype=torch.float32, device=prob.device), torch.arange(W, dtype=torch.float32, device=prob.device)
    prob_sum = prob.sum()
    rows, cols = prob.sum(dim=-1), prob.sum(dim=-2)
    e_y, e_x = torch.sum(rows * ay) / prob_sum, torch.sum(cols * ax) / prob_sum
    e_h, e_w = torch.sum(rows * (ay - e_y) ** 2) / prob_sum, torch.sum(cols * (ax - e_x) ** 2) / prob_sum
    return torch.stack([prob_sum, e_y, e_x, e_h, e_w])


def stock_readout(scores, image_hw, scale, pos):
    """lwl.py:335-357, then `> 0`, sigmoid and get_target_state as LWL.track chains them."""
    re = F.interpolate(scores, scale_factor=scale, mode='bilinear')
    re = re.view(*re.shape[-2:])
    im = torch.ones(image_hw, dtype=re.dtype, device=re.device) * (-100.0)
    r1, c1 = int(pos[0] - 0.5 * re.shape[-2]), int(pos[1] - 0.5 * re.shape[-1])
    r2, c2 = r1 + re.shape[-2], c1 + re.shape[-1]
    r1_pad, c1_pad, r2_pad, c2_pad = max(0, -r1), max(0, -c1), max(r2 - image_hw[0], 0), max(c2 - image_hw[1], 0)
    im[r1 + r1_pad:r2 - r2_pad, c1 + c1_pad:c2 - c2_pad] = re[r1_pad:re.shape[0] - r2_pad, c1_pad:re.shape[1] - c2_pad]
    mask = (im > 0).float()
    prob = torch.sigmoid(im)
    return im, prob, mask, target_state(prob)


def stock_merge(scores):
    """lwl.py:229-269 on the device."""
    prob = torch.sigmoid(scores)
    eps = 1e-7
    bg_p = torch.prod(1 - prob, dim=0).clamp(eps, 1.0 - eps)
    bg_score = (bg_p / (1.0 - bg_p)).log()
    all_scores = torch.cat((bg_score.unsqueeze(0), scores), dim=0)
    out = [1.0 / (all_scores - s.unsqueeze(0)).exp().sum(dim=0) for s in all_scores]
    agg = torch.stack(out, dim=0)
    labels = agg.argmax(dim=0).to(torch.uint8)
    return agg, labels, torch.stack([target_state(agg[i + 1]) for i in range(scores.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_readout_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "crop": list(CROP), "merge_image": list(MERGE_HW),
           "stock_kind": "this project's restatement of the reference's sequence, stock torch operators on the same GPU", "cases": {}}
    crop = torch.from_numpy(SC.blob_scores(4600, *CROP)).to(DEV)[None, None]
    cases = {}
    for name, (hw, scale, pos) in READOUTS.items():
        scale = float(torch.tensor(scale, dtype=torch.float32))
        fused = lambda hw=hw, scale=scale, pos=pos: SR.crop_to_image(crop, hw, scale, pos)  # noqa: E731
        stock = lambda hw=hw, scale=scale, pos=pos: stock_readout(crop, hw, scale, pos)  # noqa: E731
        diff = lambda f, s: max(float((f.scores_im - s[0]).abs().max()), float((f.prob_im - s[1]).abs().max()))  # noqa: E731
        cases[name] = (fused, stock, diff, 4 * (CROP[0] * CROP[1] + 3 * hw[0] * hw[1]))
    for name, n in MERGES.items():
        s = torch.from_numpy(SC.blob_scores(4700 + n, n * MERGE_HW[0], MERGE_HW[1]).reshape(n, *MERGE_HW)).to(DEV)
        s[0, :MERGE_HW[0] // 3] = SC.FILL
        fused = lambda s=s: SR.merge(s)  # noqa: E731
        stock = lambda s=s: stock_merge(s)  # noqa: E731
        diff = lambda f, t: float((f.prob - t[0]).abs().max())  # noqa: E731
        cases[name] = (fused, stock, diff, MERGE_HW[0] * MERGE_HW[1] * (4 * n + 4 * (n + 1) + 1))
    with torch.no_grad():
        for name, (fused, stock, diff, nbytes) in cases.items():
            variants = {"fused": fused, "stock": stock}
            d = diff(fused(), stock())
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
            out = {"max_abs_fused_minus_stock": d, "bytes": nbytes}
            for k in variants:
                out[k] = {"device_us": statistics.median(dev_t[k]), "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k])}
            out["fused_GBps"] = nbytes / out["fused"]["device_us"] * 1e-3
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
