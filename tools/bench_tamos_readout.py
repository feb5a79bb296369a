"""TaMOs per-frame multi-object read-out and training targets on one MI355X, per frame, at the deployed sizes (24 x 36 raw scores ->
48 x 72 decision map, stride 8):
    python -B tools/bench_tamos_readout.py [--rounds N] [--out profiles/tamos_readout_bench.json]
  readout_t1 / readout_t3 / readout_t10   pytracking_amd.tamos_readout.MotReadout.run: upsample, sigmoid, localize_advanced,
                                          direct_bbox_regression and the clip of T objects -- one launch, one polled wait
                                                                                     vs  the reference's per-object sequence in stock torch
  targets_nf2                             encode_bbox of 2 memory frames x 10 objects and 10 Gaussian labels, one launch
                                                                                     vs  the reference's sequence in stock torch
  track_t3                                the unmodified TaMOs.track on the stub net of tests/tamos_tracker.py (3 objects, 12 x 18 maps), wall
                                          time per call with install(tamos=True, tamos_readout=True) and with install(tamos=True) alone; only
                                          where the reference bundle is present
`stock` restates what TaMOs.track runs per object (pytracking/tracker/tamos/tamos.py:181-185, 248-280, 319-320, 366-429: the bicubic
upsample and the sigmoid once, then per object two max2d's, a clone, a masked fill, the .item() / .cpu() round trips, the copy of the object's
ltrb map to the host and two coordinate grids on the CPU; encode_bbox per memory frame, the Gaussian label on the CPU and its upload) with
stock PyTorch-ROCm operators on the SAME GPU.  It is this project's own restatement: it reads no reference file.  Both variants of a case are
interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.  Two figures per variant, because the
gain is host time: `host_us` = one call until its results are on the host, host clock; `device_us` = event-timed batch of 20 back-to-back
calls / 20 (for `stock` that includes the gaps its synchronisations leave).  Medians over the rounds, with the minimum and the quartiles."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pytracking_amd import _lib_mot as M  # noqa: E402
from pytracking_amd import tamos_readout as TR  # noqa: E402

DEV = "cuda:0"
BATCH = 20
HS, WS, H, W, STRIDE = 24, 36, 48, 72, 8
IMAGE_HW = (480, 854)


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def get(self, name, default=None):
        return self.__dict__.get(name, default)


class Tracker:
    """the attributes the read-out reads from a TaMOs object (tamos.py:60-86, 432-454, 601-610)"""

    def __init__(self, T, seed=0):
        rng = np.random.default_rng(seed)
        self.params = Params(target_not_found_threshold=0.25, distractor_threshold=0.8, hard_negative_threshold=0.5, target_neighborhood_scale=2.2,
                             dispalcement_scale=0.8, advanced_localization=True, normalize_scores=True, device=DEV,
                             image_sample_size=(H * STRIDE, W * STRIDE), feature_stride=16)
        self.object_ids = list(range(1, T + 1))
        self.img_sample_sz = torch.Tensor([H * STRIDE, W * STRIDE])
        self.img_support_sz = self.img_sample_sz
        self.train_img_sample_sz = torch.Tensor([HS * 16, WS * 16])
        self.kernel_size = torch.Tensor([1, 1])
        self.scale_factor = float(self.img_sample_sz[1]) / IMAGE_HW[1]
        self.image_sz = torch.Tensor(list(IMAGE_HW))
        self.frame_num = 2
        self.cells = {o: (float(rng.integers(4, H - 4)), float(rng.integers(4, W - 4))) for o in self.object_ids}
        ratio = STRIDE / self.scale_factor
        self.pos = {o: torch.Tensor([r * ratio, c * ratio]) for o, (r, c) in self.cells.items()}
        self.pos_prev = {o: p.clone() for o, p in self.pos.items()}
        self.target_sz = {o: torch.Tensor([60.0, 80.0]) for o in self.object_ids}
        self.feature_sz = torch.Tensor([HS, WS])
        self.sigma = 1 / 4 / 4.0 * math.sqrt(HS * WS) * torch.ones(2)

    def maps(self, T_tokens=10, seed=1):
        rng = np.random.default_rng(seed)
        s = -3.0 + rng.uniform(0, 0.02, (T_tokens, HS, WS))
        rr, cc = np.mgrid[0:HS, 0:WS]
        for o, (r, c) in self.cells.items():
            for (dr, dc, a) in ((0, 0, 5.0), (9, -11, 3.4)):
                y, x = ((r + dr) % H + 0.5) * HS / H - 0.5, ((c + dc) % W + 0.5) * WS / W - 0.5
                s[o - 1] += a * np.exp(-((rr - y) ** 2 + (cc - x) ** 2) / (2 * 0.7 ** 2))
        ltrb = rng.uniform(0.05, 0.3, (T_tokens, 4, H, W))
        return (torch.from_numpy(s.astype(np.float32)).to(DEV)[None, None], torch.from_numpy(ltrb.astype(np.float32)).to(DEV)[None, None])


def max2d(a):
    mv, ar = torch.max(a, dim=-2)
    mv, ac = torch.max(mv, dim=-1)
    ar = ar.gather(-1, ac.unsqueeze(-1)).squeeze(-1)
    return mv, torch.stack((ar, ac), -1)


def stock_localize(trk, scores, oid):
    """the operator sequence of localize_advanced (tamos.py:366-429) on a (1, H, W) device map"""
    prm = trk.params
    sz = scores.shape[-2:]
    output_sz = torch.Tensor(list(sz)) - (trk.kernel_size + 1) % 2
    ratio = (trk.img_support_sz / output_sz) / trk.scale_factor
    score_center = trk.pos[oid] / ratio
    m1, d1 = max2d(scores)
    _, scale_ind = torch.max(m1, dim=0)
    m1 = m1[scale_ind]
    d1 = d1[scale_ind, ...].float().cpu().view(-1)
    t1 = d1 - score_center
    if m1.item() < prm.target_not_found_threshold:
        return "not_found", d1
    if m1.item() < prm.get("uncertain_threshold", -float("inf")) or m1.item() < prm.get("hard_sample_threshold", -float("inf")):
        return "uncertain", d1
    neigh = trk.target_sz[oid] / ratio * prm.target_neighborhood_scale
    top = max(round(d1[0].item() - neigh[0].item() / 2), 0)
    bottom = min(round(d1[0].item() + neigh[0].item() / 2 + 1), sz[0])
    left = max(round(d1[1].item() - neigh[1].item() / 2), 0)
    right = min(round(d1[1].item() + neigh[1].item() / 2 + 1), sz[1])
    masked = scores[scale_ind:scale_ind + 1, ...].clone()
    masked[..., top:bottom, left:right] = 0
    m2, d2 = max2d(masked)
    d2 = d2.float().cpu().view(-1)
    t2 = d2 - score_center
    prev = (trk.pos[oid] - trk.pos_prev[oid]) / ratio
    if m2 > prm.distractor_threshold * m1:
        n1, n2 = torch.sqrt(torch.sum((t1 - prev) ** 2)), torch.sqrt(torch.sum((t2 - prev) ** 2))
        th = prm.dispalcement_scale * math.sqrt(sz[0] * sz[1]) / 2
        if n2 > th and n1 < th:
            return "hard_negative", d1
        if n2 < th and n1 > th:
            return "hard_negative", d2
        return "uncertain", d1
    if m2 > prm.hard_negative_threshold * m1 and m2 > prm.target_not_found_threshold:
        return "hard_negative", d1
    return "normal", d1


def stock_box(trk, bbox_preds, coords, loc, stride):
    """the operator sequence of direct_bbox_regression and clip_bbox_to_image_area (tamos.py:248-280, 106-112)"""
    sx = torch.arange(0, trk.img_sample_sz[1], step=stride, dtype=torch.float32)
    sy = torch.arange(0, trk.img_sample_sz[0], step=stride, dtype=torch.float32)
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    xs, ys = xx + stride // 2, yy + stride // 2
    ltrb = bbox_preds.permute(0, 1, 3, 4, 2)[0, 0].cpu() * trk.train_img_sample_sz[[1, 0, 1, 0]]
    xs1, xs2, ys1, ys2 = xs - ltrb[:, :, 0], xs + ltrb[:, :, 2], ys - ltrb[:, :, 1], ys + ltrb[:, :, 3]
    r, c = loc.int().tolist()
    sw, sh = trk.img_sample_sz[1], trk.img_sample_sz[0]
    x1 = xs1[r, c] / sw * (coords[0, 3] - coords[0, 1]) + coords[0, 1]
    y1 = ys1[r, c] / sh * (coords[0, 2] - coords[0, 0]) + coords[0, 0]
    x2 = xs2[r, c] / sw * (coords[0, 3] - coords[0, 1]) + coords[0, 1]
    y2 = ys2[r, c] / sh * (coords[0, 2] - coords[0, 0]) + coords[0, 0]
    b = torch.Tensor([x1, y1, x2 - x1, y2 - y1])
    Hi, Wi = IMAGE_HW
    cx1, cy1 = max(0, min(b[0], Wi - 10)), max(0, min(b[1], Hi - 10))
    cx2, cy2 = max(cx1 + 10, min(b[0] + b[2], Wi)), max(cy1 + 10, min(b[1] + b[3], Hi))
    return b, torch.Tensor([cx1, cy1, cx2 - cx1, cy2 - cy1])


def stock_readout(trk, target_scores, bbox_preds, coords):
    s = F.interpolate(target_scores[0], bbox_preds.shape[-2:], mode="bicubic").unsqueeze(0)
    s = torch.sigmoid(s)
    out = {}
    for oid in trk.object_ids:
        flag, loc = stock_localize(trk, s[:, :, oid - 1].squeeze(1), oid)
        raw, box = stock_box(trk, bbox_preds[:, :, oid - 1], coords, loc, STRIDE)
        out[oid] = (flag, loc, raw, box)
    return out


def stock_targets(trk, boxes, positions):
    """encode_bbox per memory frame (tamos.py:114-153, 299) and get_label_function per object with its upload (tamos.py:204, 582-592)"""
    stride, (oh, ow) = 16, trk.params.image_sample_size
    outs = []
    for bb in boxes:
        mask = (bb[:, 2] > 0) & (bb[:, 3] > 0)
        b = bb[mask]
        sx = torch.arange(0, ow, step=stride, dtype=torch.float32, device=b.device)
        sy = torch.arange(0, oh, step=stride, dtype=torch.float32, device=b.device)
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        xs, ys = xx.reshape(-1) + stride // 2, yy.reshape(-1) + stride // 2
        xyxy = torch.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], dim=1)
        reg = torch.stack([xs[:, None] - xyxy[:, 0][None], ys[:, None] - xyxy[:, 1][None], xyxy[:, 2][None] - xs[:, None], xyxy[:, 3][None] - ys[:, None]], dim=2)
        reg = reg.reshape(-1, 4) / torch.tensor([ow, oh, ow, oh]).reshape(1, 4).to(b.device)
        reg = reg.reshape(oh // stride, ow // stride, b.shape[0], 4).permute(2, 3, 0, 1)
        full = torch.zeros(bb.shape[0], 4, oh // stride, ow // stride, device=b.device)
        full[mask] = reg
        outs.append(full.unsqueeze(0))
    labels = []
    for pos in positions:
        norm = (pos * trk.scale_factor - trk.img_support_sz / 2) / trk.img_support_sz
        center = trk.feature_sz * norm
        g = []
        for d in range(2):
            sz, sg = trk.feature_sz[d].item(), trk.sigma[d].item()
            k = torch.arange(-(sz - 1) / 2, (sz + 1) / 2)
            g.append(torch.exp(-1.0 / (2 * sg ** 2) * (k - center[d]) ** 2))
        labels.append((g[0].reshape(1, 1, -1, 1) * g[1].reshape(1, 1, 1, -1)).to(DEV))
    return torch.cat(outs, dim=0), labels


def fused_targets(trk, boxes, positions):
    ltrb = torch.empty(*boxes.shape[:2], 4, HS, WS, device=DEV)
    centres = [(trk.feature_sz * ((p * trk.scale_factor - trk.img_support_sz / 2) / trk.img_support_sz)).tolist() for p in positions]
    lab = TR.label_block(trk.feature_sz.tolist(), trk.sigma.tolist(), (0.0, 0.0))
    n = len(centres)
    out = torch.empty(n, HS, WS, device=DEV)
    flat = (ctypes.c_float * (2 * n))(*[v for c in centres for v in c])
    b = boxes.reshape(-1, 4)
    M.check(M.lib().pt_mot_targets_f32(b.data_ptr(), b.shape[0], HS * 16, WS * 16, 16, ltrb.data_ptr(), ctypes.byref(lab), flat, n, out.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pt_mot_targets_f32")
    return ltrb, out


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "q1": q[0], "q3": q[2]}


def time_variants(variants, rounds, waits):
    """variants {name: fn}; waits {name: True when fn returns with its results on the host already}"""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    dev_t, host_t = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(rounds):
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
            if not waits[k]:
                torch.cuda.synchronize()
            host_t[k].append((time.perf_counter() - t0) * 1e6)
    return {k: {"host_us": quartiles(host_t[k]), "device_us": quartiles(dev_t[k])} for k in variants}


def bench_track(rounds):
    """wall time per TaMOs.track call on the stub net, tamos_readout on / off, interleaved run by run"""
    from oracle import ref_harness
    if not ref_harness.available():
        return {"skipped": "no reference bundle"}
    ref_harness.install()
    import tamos_tracker as TT
    from pytracking.tracker.tamos.tamos import TaMOs
    from pytracking_amd import install as amd
    times = {"readout_on": [], "readout_off": []}
    orig = TaMOs.track
    sink = []

    def track(self, image, info=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = orig(self, image, info)
        torch.cuda.synchronize()
        sink.append((time.perf_counter() - t0) * 1e6)
        return out
    TaMOs.track = track
    try:
        for r in range(rounds + 1):
            for key, flag in (("readout_on", True), ("readout_off", False)):
                amd.uninstall()
                amd.install(tamos=True, tamos_readout=flag)
                del sink[:]
                TT.run(device="cuda", **TT.RUN)
                if r:                                                # round 0 warms both variants up
                    times[key] += sink
    finally:
        TaMOs.track = orig
        amd.uninstall()
    out = {k: dict(quartiles(v), calls=len(v)) for k, v in times.items()}
    out["off_over_on"] = out["readout_off"]["median"] / out["readout_on"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--track-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tamos_readout_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "maps": [HS, WS, H, W],
           "stock_kind": "this project's restatement of the reference's sequence, stock torch operators on the same GPU", "cases": {}}
    with torch.no_grad():
        for T in (1, 3, 10):
            trk = Tracker(T)
            scores, ltrb = trk.maps()
            coords = torch.Tensor([[0, 0, trk.img_sample_sz[0] / trk.scale_factor, trk.img_sample_sz[1] / trk.scale_factor]])
            ro = TR.MotReadout(trk)
            fused = lambda: ro.run(scores, ltrb, coords, IMAGE_HW, STRIDE)  # noqa: E731
            stock = lambda: stock_readout(trk, scores, ltrb, coords)  # noqa: E731
            f, s = fused(), stock()
            agree = all(f[o].flag == s[o][0] and f[o].score_loc.int().tolist() == s[o][1].int().tolist() for o in trk.object_ids)
            diff = max(float((f[o].bbox - s[o][3]).abs().max()) for o in trk.object_ids)
            out = time_variants({"fused": fused, "stock": stock}, a.rounds, {"fused": True, "stock": True})
            out.update(objects=T, flags_and_cells_agree=agree, max_abs_box_fused_minus_stock=diff, flags=[f[o].flag for o in trk.object_ids])
            out["stock_over_fused_host"] = out["stock"]["host_us"]["median"] / out["fused"]["host_us"]["median"]
            out["stock_over_fused_device"] = out["stock"]["device_us"]["median"] / out["fused"]["device_us"]["median"]
            res["cases"][f"readout_t{T}"] = out
            print(f"readout_t{T}", json.dumps(out), flush=True)
        trk = Tracker(10)
        rng = np.random.default_rng(5)
        boxes = torch.from_numpy(np.concatenate([rng.uniform(0, 300, (2, 10, 2)), rng.uniform(10, 90, (2, 10, 2))], -1).astype(np.float32)).to(DEV)
        positions = [trk.pos[o] for o in trk.object_ids]
        fused = lambda: fused_targets(trk, boxes, positions)  # noqa: E731
        stock = lambda: stock_targets(trk, boxes, positions)  # noqa: E731
        (fl, fy), (sl, sy) = fused(), stock()
        diff = max(float((fl - sl).abs().max()), max(float((fy[i] - sy[i][0, 0]).abs().max()) for i in range(10)))
        out = time_variants({"fused": fused, "stock": stock}, a.rounds, {"fused": False, "stock": False})
        out.update(memory_frames=2, objects=10, max_abs_fused_minus_stock=diff)
        out["stock_over_fused_host"] = out["stock"]["host_us"]["median"] / out["fused"]["host_us"]["median"]
        out["stock_over_fused_device"] = out["stock"]["device_us"]["median"] / out["fused"]["device_us"]["median"]
        res["cases"]["targets_nf2"] = out
        print("targets_nf2", json.dumps(out), flush=True)
        res["cases"]["track_t3"] = bench_track(a.track_rounds)
        print("track_t3", json.dumps(res["cases"]["track_t3"]), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
