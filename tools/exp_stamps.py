"""Experiment: phase time stamps of the two solver passes (library built with -DPT_STAMPS, selected via PT_HOT_LIB).
   PT_HOT_LIB=.../libpt_hot_stamps.so python tools/exp_stamps.py [n ...]"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from pytracking_amd import _lib, bench_frame, synth  # noqa: E402

if os.environ.get("PT_STAMP_SET") == "2":
    ADJ = ["entry", "small loads requested", "feature loads requested", "maps zeroed", "table written", "barrier 1", "update stage done", "end"]
else:
    ADJ = None
NAMES = {0: ["entry", "loads issued", "filter reduced+staged", "barrier 1", "MFMA loop done", "T written", "barrier 2", "end"],
         1: ["entry", "update inputs requested", "table built", "argument block held", "barrier 1", "update stage done", "barrier 2",
             "first feature group arrived", "MFMA loop done", "red written + barrier 3", "partial gradient stored", "end"]}
SLOTS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]            # buffer slot of stamp k (slot 8 is HW_ID)


def main():
    ns = [int(a) for a in sys.argv[1:]] or [32, 50]
    cfg = synth.DIMP50
    dev = torch.device("cuda:0")
    L = _lib.lib()
    L.pt_debug_set_stamps.argtypes = [ctypes.c_void_p]
    stream = torch.cuda.Stream()
    pool = bench.make_pool(cfg, 99, dev)
    with torch.cuda.stream(stream):
        for n in ns:
            st = bench_frame.TrackState(cfg, n, seed=1234, device=dev)
            bench.run_frames(st, pool, 0, 10)
            stream.synchronize()
            c = st.cfg
            for which in (0, 1):
                args = (ctypes.byref(st.params), st.filter.data_ptr(), st.mem_feat.data_ptr(), st.mem_bb.data_ptr(),
                        st.sample_weight.data_ptr(), st.n, c["C"], c["H"], c["W"], c["K"], bench.NUM_ITER, st.ws.data_ptr(),
                        st.ws.numel(), which)
                sp = ctypes.c_void_p(stream.cuda_stream)
                nwg = 8 * n if which == 0 else 256 * 2
                buf = torch.zeros(nwg * 16 * 16, dtype=torch.int64, device=dev)
                L.pt_track_frame_replay_pass_f32(*args, 20, sp)                # warm
                acc, acc_hw = [], []
                for rep in range(5):
                    buf.zero_()
                    stream.synchronize()
                    L.pt_debug_set_stamps(ctypes.c_void_p(buf.data_ptr()))
                    L.pt_track_frame_replay_pass_f32(*args, 1, sp)
                    stream.synchronize()
                    L.pt_debug_set_stamps(None)
                    raw = buf.cpu().numpy().reshape(nwg, 16, 16)
                    hw = raw[:, :, 8]                                               # HW_ID | 1 << 32 (0: wave slot unused)
                    t = raw[:, :, SLOTS].astype(np.float64)
                    t[t == 0] = np.nan
                    t = (t - np.nanmin(t[:, :, 0])) * 0.01                      # 100 MHz -> us
                    acc.append(t)
                    acc_hw.append(hw)
                t = np.nanmean(np.stack(acc), axis=0)
                print(f"n={n} {'k_corr2 (fused)' if which == 0 else 'k_adj2 (sd)'}: per-stamp over all waves [us since first wave entry]: min / mean / max"
                      f" | per-WORKGROUP last wave: mean")
                last = len(NAMES[which]) - 1
                for k in range(last + 1):
                    col = t[:, :, k]
                    if np.all(np.isnan(col)):
                        continue
                    wgmax = np.nanmax(col, axis=1)
                    print(f"   {k} {NAMES[which][k]:34s} {np.nanmin(col):6.2f} {np.nanmean(col):6.2f} {np.nanmax(col):6.2f}   | {np.nanmean(wgmax):6.2f}")
                if which == 0:
                    simd_table(np.concatenate(acc), np.concatenate(acc_hw))       # placement differs from launch to launch
                elif last == 11:
                    adj_table(np.concatenate(acc), np.concatenate(acc_hw), n, c, nwg)
                dur = np.nanmax(t[:, :, last], axis=1) - np.nanmin(t[:, :, 0], axis=1)
                print(f"   workgroup duration (entry of first wave -> end of last): min {np.nanmin(dur):.2f} mean {np.nanmean(dur):.2f} max {np.nanmax(dur):.2f}")


def simd_table(t, hw):
    """k_corr2: where the waves of a workgroup sit (SIMD of HW_ID; every repeat is a set of workgroups of its own) and how long 'barrier 1 -> MFMA loop done' takes by the
    number of waves that share the SIMD."""
    live = (hw != 0).any(axis=1)                                                    # the buffer has room for 8 n workgroups; pairs launch 4 n
    t, hw = t[live], hw[live]
    used = hw != 0
    simd = (hw >> 4) & 3
    cu = (hw >> 8) & 0xFF                                                           # CU | SH << 4 | SE << 5
    nw = int(used[0].sum())
    per = np.stack([((simd == s) & used).sum(axis=1) for s in range(4)], axis=1)    # [workgroup][SIMD] -> waves
    pat, cnt = np.unique(np.sort(per, axis=1)[:, ::-1], axis=0, return_counts=True)
    print(f"   waves per workgroup {nw}; waves per SIMD (sorted) : workgroups  " + "  ".join(f"{'/'.join(map(str, p))}: {c}" for p, c in zip(pat, cnt)))
    one_cu = sum(len(set(cu[b][used[b]])) == 1 for b in range(hw.shape[0]))
    print(f"   workgroups whose waves share one CU id: {one_cu} of {hw.shape[0]}")
    order = [int(s) for s in simd[0][used[0]]]
    print(f"   workgroup 0: SIMD of wave 0.. = {order}")
    loop = t[:, :, 4] - t[:, :, 3]
    share = np.take_along_axis(per, simd, axis=1).astype(np.float64)                 # waves on this wave's SIMD
    share[~used] = np.nan
    for k in sorted(set(share[used].astype(int))):
        sel = share == k
        print(f"   waves on a SIMD holding {k}: {int(sel.sum()):5d} waves, barrier 1 -> MFMA loop done {np.nanmean(loop[sel]):5.2f} us mean, "
              f"{np.nanmax(loop[sel]):5.2f} max; loop done at {np.nanmean(t[:, :, 4][sel]):5.2f} us")
    for w in range(nw):
        print(f"   wave {w:2d}: loop {np.nanmean(loop[:, w]):5.2f} us, done at {np.nanmean(t[:, w, 4]):5.2f}, shares its SIMD with "
              f"{np.nanmean(share[:, w]) - 1:4.2f} others")
    kind_table(t, nw)
    wg_last = np.nanmax(t[:, :, 4], axis=1) - np.nanmin(t[:, :, 3], axis=1)
    wg_first = np.nanmin(t[:, :, 4], axis=1) - np.nanmin(t[:, :, 3], axis=1)
    print(f"   per workgroup, first barrier-1 exit -> MFMA loop done: first wave {np.mean(wg_first):5.2f} us, last wave {np.mean(wg_last):5.2f} us")


def kind_table(t, nw):
    """k_corr2, mixed pairs (2 tiles + 2 waves, csrc/fast_passes.hip: waves 0..3 = (sample, position half) of tile 0, then the full tiles
    of sample 0 and of sample 1): MFMA loop, wait at barrier 2 and the epilogue (shift-and-add: barrier 2 -> end) per wave kind."""
    if nw < 6 or nw % 2:
        return
    full = (nw - 4) // 2
    kinds = (("half 0 + leftover quads", [0, 2]), ("half 1", [1, 3]), ("full tiles of sample 0", list(range(4, 4 + full))),
             ("full tiles of sample 1", list(range(4 + full, nw))))
    seg = lambda k0, k1, ws: np.nanmean((t[:, :, k1] - t[:, :, k0])[:, ws])
    print("   per wave kind (mixed pair):          barrier 1 -> loop done | loop done -> T written | at barrier 2 | barrier 2 -> end | end at")
    for name, ws in kinds:
        print(f"   {name:24s} (waves {','.join(map(str, ws)):9s})   {seg(3, 4, ws):5.2f}   {seg(4, 5, ws):5.2f}   {seg(5, 6, ws):5.2f}   "
              f"{seg(6, 7, ws):5.2f}   {np.nanmean(t[:, ws, 7]):5.2f}")
    ep = t[:, :, 7] - t[:, :, 6]
    print("   epilogue per wave (barrier 2 -> end): " + " ".join(f"w{w}:{np.nanmean(ep[:, w]):4.2f}" for w in range(nw)))
    print(f"   per workgroup: last barrier-2 exit -> last wave's end {np.mean(np.nanmax(t[:, :, 7], axis=1) - np.nanmax(t[:, :, 6], axis=1)):5.2f} us")


def adj_table(t, hw, n, c, nwg):
    """k_adj2 (stamp set A): waves per SIMD, the update stage (wave w < ns carries sample w of the slice) and the wait behind it at
    barrier 2, the MFMA loop per wave, the last wave at each barrier.  Every repeat is a set of `nwg` buffer rows of its own.
    Which samples a workgroup's slice holds is restated here from pt_fast_plan / k_adj2 (csrc/fast_passes.hip: 8 or 16 position
    slices, ks = (b >> 3) / bpx, >= 8 channel blocks); the workgroup count is checked against it, change the two together."""
    reps = t.shape[0] // nwg
    b = np.tile(np.arange(nwg), reps)
    live = (hw != 0).any(axis=1)
    t, hw, b = t[live], hw[live], b[live]
    used = hw != 0
    nw = int(used[0].sum())
    t, hw, used = t[:, :nw], hw[:, :nw], used[:, :nw]
    simd = (hw >> 4) & 3
    cu = (hw >> 8) & 0xFF
    per = np.stack([((simd == s) & used).sum(axis=1) for s in range(4)], axis=1)
    pat, cnt = np.unique(np.sort(per, axis=1)[:, ::-1], axis=0, return_counts=True)
    print(f"   waves per workgroup {nw}; waves per SIMD (sorted) : workgroups  " + "  ".join(f"{'/'.join(map(str, p))}: {k}" for p, k in zip(pat, cnt)))
    print(f"   workgroups whose waves share one CU id: {sum(len(set(cu[k])) == 1 for k in range(hw.shape[0]))} of {hw.shape[0]}")
    print(f"   workgroup 0: SIMD of wave 0.. = {[int(v) for v in simd[0]]}")
    # samples of the workgroup's position slice (pt_fast_plan / k_adj2: ks = (b >> 3) / bpx with >= 8 channel blocks)
    HW = c["H"] * c["W"]
    NG = (n * HW + 15) // 16
    gper = next(g for g in (-(-NG // ks) for ks in (8, 16)) if -(-g // nw) <= 128 // nw)
    assert c["C"] // 16 >= 8 and hw.shape[0] == reps * (c["C"] // 16) * -(-NG // gper), "the restated slice plan does not match the launch"
    ks = (b >> 3) // (c["C"] // 16 // 8)
    gbeg, gend = ks * gper, np.minimum(NG, ks * gper + gper)
    ns = np.minimum(n - 1, (gend * 16 - 1) // HW) - (gbeg * 16) // HW + 1
    upd = np.arange(nw)[None, :] < ns[:, None]
    print(f"   samples per slice: {sorted(set(int(v) for v in ns))}; waves with an update stage {int(upd.sum())} of {upd.size}")
    share = np.take_along_axis(per, simd, axis=1).astype(np.float64)
    seg = lambda k0, k1: t[:, :, k1] - t[:, :, k0]
    for name, sel in (("with an update stage", upd), ("without", ~upd)):
        if sel.any():
            print(f"   waves {name:21s}: barrier 1 -> update stage done {np.nanmean(seg(4, 5)[sel]):5.2f} us mean {np.nanmax(seg(4, 5)[sel]):5.2f} max, "
                  f"then at barrier 2 for {np.nanmean(seg(5, 6)[sel]):5.2f} us; barrier 2 -> first features {np.nanmean(seg(6, 7)[sel]):5.2f}; "
                  f"barrier 2 -> MFMA loop done {np.nanmean(seg(6, 8)[sel]):5.2f} us; at barrier 3 for {np.nanmean(seg(8, 9)[sel]):5.2f} us")
    for k in sorted(set(share.astype(int).ravel())):
        sel = share == k
        print(f"   waves on a SIMD holding {k}: {int(sel.sum()):5d} waves, barrier 2 -> MFMA loop done {np.nanmean(seg(6, 8)[sel]):5.2f} us mean, "
              f"{np.nanmax(seg(6, 8)[sel]):5.2f} max")
    for w in range(nw):
        print(f"   wave {w:2d}: entry {np.nanmean(t[:, w, 0]):5.2f}, args held {np.nanmean(t[:, w, 3]):5.2f}, update {np.nanmean(seg(4, 5)[:, w]):5.2f}, at barrier 2 "
              f"{np.nanmean(seg(5, 6)[:, w]):5.2f}, first features +{np.nanmean(seg(6, 7)[:, w]):5.2f}, loop {np.nanmean(seg(6, 8)[:, w]):5.2f}, done at "
              f"{np.nanmean(t[:, w, 8]):5.2f}, at barrier 3 {np.nanmean(seg(8, 9)[:, w]):5.2f}; shares its SIMD with {np.nanmean(share[:, w]) - 1:4.2f} others")
    for name, k in (("barrier 1", 3), ("barrier 2", 5), ("barrier 3", 8)):
        lastw = np.nanargmax(t[:, :, k], axis=1)
        spread = np.nanmax(t[:, :, k], axis=1) - np.nanmin(t[:, :, k], axis=1)
        print(f"   last wave to reach {name}: " + " ".join(f"w{w}:{int((lastw == w).sum())}" for w in range(nw)) +
              f"; first -> last arrival {np.mean(spread):5.2f} us mean")
    ent = np.nanmin(t[:, :, 0], axis=1)
    print("   per workgroup since its first wave's entry: " + ", ".join(
        f"{nm} {np.mean(np.nanmax(t[:, :, k], axis=1) - ent):5.2f}" for nm, k in (("barrier 1", 4), ("barrier 2", 6), ("loop done (last wave)", 8),
                                                                                 ("barrier 3", 9), ("end", 11))))


if ADJ:
    NAMES[1] = ADJ

if __name__ == "__main__":
    main()
