"""Measurement of the per-frame sample-memory update on the MI355X (needs a GPU; the track() part needs oracle/_ref):

    python -B tools/bench_mem_update.py [--reps 200] [--batch 50] [--frames 60] [--rounds 3] [--out profiles/mem_update_bench.json]

One process, variants interleaved call by call, medians with quartiles.  Per workload (DiMP-50, ToMP, ATOM, LWL memory shapes) and phase
(`fill`: the index is a host value, the fused call does not wait; `full`: the arg-min runs on the device, one wait):
  fused   pytracking_amd.memory_update.run(blocks, rows)
  stock   the reference's statement sequence (dimp.py:445-484 / atom.py:603-639 / lwl.py:474-516 and the stores of `update_memory`) restated
          in stock PyTorch-ROCm on the same GPU, with its `.item()` and its truth test of a device tensor
  host_us    host clock from the call to the Python ints of `replace_ind` being on the host (stream idle at the start, no synchronise at the end)
  event_us   device events around a batch of calls, per call: what the stream is busy for, launch gaps included
Then `track()` of the installed unmodified DiMP (the method of tests/profile_installed_track.py: stub backbone outputs and frames cached on
the device), install() against install(memory=True), three interleaved rounds of 60 frames each, wall ms per call with the device
synchronised.  A frame is an update frame when `DiMP.update_memory` was called in it (a counter on the class, the same for both variants),
split by whether the filter optimiser ran in it as well (every second update frame with the harness's train_skipping of 2);
`target_not_found_threshold` is lowered to 0.1 as in the closed-loop harness, because on the stub's scores the parameter file's 0.25 calls
most frames 'not_found', and those do not update.
Nothing here promises a speed-up: rows that lose are reported as they are."""
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

from pytracking_amd import memory_update as MU  # noqa: E402

DEV = "cuda:0"
# name: rule, n, num_init, floor, lr, slot shapes of the rows
WORKLOADS = {
    "dimp50": ("A", 50, 13, 0.25, 0.01, [(512, 18, 18), (4,)]),
    "tomp": ("A", 2, 1, 0.0, 0.01, [(256, 18, 18), (1, 18, 18), (4,)]),
    "atom": ("B", 250, 13, 0.25, 0.01, [(64, 18, 18), (1, 18, 18)]),
    "lwl": ("C", 32, 1, 0.0, 0.1, [(512, 30, 52), (1, 480, 832)]),
}


def stock_update(sw, prev_ind, num_samp, num_init, lr, floor, always_argmin):
    """the reference's statements on stock PyTorch (rule A; always_argmin: rule B)"""
    s_ind = 0 if not floor else num_init
    if num_samp == 0 or lr == 1:
        sw[:] = 0
        sw[0] = 1
        r_ind = 0
    else:
        if num_samp < sw.shape[0] and not always_argmin:
            r_ind = num_samp
        else:
            _, r_ind = torch.min(sw[s_ind:], 0)
            r_ind = r_ind.item() + s_ind
        if prev_ind is None:
            sw /= 1 - lr
            sw[r_ind] = lr
        else:
            sw[r_ind] = sw[prev_ind] / (1 - lr)
    sw /= sw.sum()
    if floor and sw[:num_init].sum() < floor:
        sw /= floor + sw[num_init:].sum()
        sw[:num_init] = floor / num_init
    return r_ind


class State:
    def __init__(self, name, phase):
        rule, n, num_init, floor, lr, shapes = WORKLOADS[name]
        g = torch.Generator(device="cpu").manual_seed(5)
        w = torch.rand(n, generator=g) + 0.5
        self.rule, self.n, self.num_init, self.floor, self.lr = rule, n, num_init, floor, lr
        self.stored = n if phase == "full" else max(num_init, n // 2) if n > 2 else 1
        if phase == "fill":
            w[self.stored:] = 0
        self.w = {v: (w / w.sum()).to(DEV) for v in ("fused", "stock")}
        self.mem = [torch.zeros(n, *s, device=DEV) for s in shapes]
        self.src = [torch.randn(3, *s, device=DEV)[1:2] for s in shapes]           # test_x[scale_ind:scale_ind+1]
        self.prev = {"fused": 0, "stock": 0}

    def fused(self):
        blk = MU.Block(self.w["fused"], self.num_init, self.stored, self.prev["fused"], self.lr, self.floor, self.rule)
        r = MU.run([blk], [MU.Row(s, m) for s, m in zip(self.src, self.mem)])
        self.prev["fused"] = r[0]
        return r

    def stock(self):
        r = stock_update(self.w["stock"], self.prev["stock"], self.stored, self.num_init, self.lr, self.floor, self.rule == "B")
        for s, m in zip(self.src, self.mem):
            m[r:r + 1, ...] = s
        self.prev["stock"] = r
        return [r]


def quartiles(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"q1": round(float(q[0]), 2), "median": round(float(q[1]), 2), "q3": round(float(q[2]), 2)}


def bench_calls(reps, batch):
    out = {}
    for name in WORKLOADS:
        for phase in ("fill", "full"):
            st = State(name, phase)
            calls = {"fused": st.fused, "stock": st.stock}
            for fn in calls.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            host = {v: [] for v in calls}
            for _ in range(reps):
                for v, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    host[v].append((time.perf_counter() - t0) * 1e6)
            ev = {v: [] for v in calls}
            for _ in range(max(4, reps // batch)):
                for v, fn in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for _ in range(batch):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    ev[v].append(a.elapsed_time(b) * 1e3 / batch)
            row = {v: {"host_us": quartiles(host[v]), "event_us": quartiles(ev[v])} for v in calls}
            row["payload_bytes"] = int(sum(4 * s.numel() for s in st.src))
            # both variants made the same number of carried calls: where they end up (not a test: tests/test_gpu_mem_update.py is)
            row["same_last_index"] = st.prev["fused"] == st.prev["stock"]
            row["max_weight_difference"] = float((st.w["fused"] - st.w["stock"]).abs().max())
            out[f"{name}.{phase}"] = row
            print(f"{name:7s} {phase:4s} host us fused {row['fused']['host_us']['median']:8.2f} stock {row['stock']['host_us']['median']:8.2f}   "
                  f"event us fused {row['fused']['event_us']['median']:8.2f} stock {row['stock']['event_us']['median']:8.2f}", flush=True)
    return out


def bench_track(frames, rounds, threshold, device="cuda"):
    """wall ms of the installed DiMP's track() per kind of frame, install() against install(memory=True).  A frame is an update frame when
    `DiMP.update_memory` was called in it (counted on the class, whichever function is bound there)."""
    import profile_installed_track as PT
    from oracle import tracker_harness as TH
    TH.ref_harness.install()
    from pytracking.tracker.dimp.dimp import DiMP
    from pytracking_amd import install as amd
    sync = torch.cuda.synchronize if device == "cuda" else (lambda: None)
    cache, imgs = {}, []
    box = {"init_bbox": [200.0, 140.0, 70.0, 90.0]}
    kinds = ("update", "update.memory-only", "update.with-optimiser", "classify-only")   # `update` holds both kinds of update frame
    walls = {(sw, kind): [] for sw in (False, True) for kind in kinds}
    fast = 0
    for rnd in range(1 + 2 * rounds):                                # round 0 fills the caches and warms every path
        sw = bool(rnd % 2 == 0) if rnd else False
        amd.uninstall()
        amd.install(memory=sw)
        amd.stats.clear()
        bound, calls = vars(DiMP)["update_memory"], []

        def update_memory(self, *args, **kw):
            calls.append(1)
            return bound(self, *args, **kw)
        DiMP.update_memory = update_memory
        try:
            tracker = PT.build(frames, cache, imgs, device=device)
            tracker.params.target_not_found_threshold = threshold
            tracker.initialize(imgs[0], dict(box))
            for f in range(frames):
                n0, o0 = len(calls), amd.stats.get("DiMPSteepestDescentGN.fast", 0)
                sync()
                t0 = time.perf_counter()
                tracker.track(imgs[1 + f])
                sync()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd and len(calls) > n0:
                    walls[(sw, "update")].append(dt)
                    walls[(sw, "update.with-optimiser" if amd.stats.get("DiMPSteepestDescentGN.fast", 0) > o0 else "update.memory-only")].append(dt)
                elif rnd:
                    walls[(sw, "classify-only")].append(dt)
        finally:
            DiMP.update_memory = bound
        if sw and device == "cuda":
            fast += amd.stats.get("DiMP.update_memory.fast", 0)
            assert "DiMP.update_memory.reference" not in amd.stats and amd.stats.get("DiMP.update_memory.fast", 0) == len(calls)
        amd.uninstall()
    out = {f"{'memory' if sw else 'default'}.{kind}": dict(quartiles(v), calls=len(v)) if v else "not measured: no such frame in the sequence"
           for (sw, kind), v in walls.items()}
    out.update(update_memory_fast_calls=fast, frames=frames, rounds_per_variant=rounds, target_not_found_threshold=threshold)
    for k, v in out.items():
        print("track() ms", k, v, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3, help="track() rounds per variant, interleaved")
    ap.add_argument("--not-found-threshold", type=float, default=0.1,
                    help="params.target_not_found_threshold of the track() part (oracle.tracker_harness.DIMP_RUN's value: on the stub's scores the "
                         "0.25 of the parameter file calls most frames 'not_found', and those frames do not update)")
    ap.add_argument("--track-only", action="store_true")
    ap.add_argument("--device", default="cuda", help="cpu: control-flow dry run of the track() part (with --track-only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_update_bench.json"))
    a = ap.parse_args()
    dry = a.track_only and a.device == "cpu"
    if not dry and not torch.cuda.is_available():
        raise SystemExit("bench_mem_update.py needs a GPU")
    result = {"device": "CPU (dry run)" if dry else torch.cuda.get_device_name(0), "reps": a.reps, "batch": a.batch}
    if not a.track_only:
        result["calls"] = bench_calls(a.reps, a.batch)
    from oracle import ref_harness
    result["track_ms"] = (bench_track(a.frames, a.rounds, a.not_found_threshold, a.device) if ref_harness.available()
                          else "not measured: no reference bundle")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
