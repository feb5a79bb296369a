"""k_corr2 keeps its bits with the feature stream requested in front of barrier 1 and held D k-steps ahead in one straight-line MFMA
loop per wave kind (csrc/fast_passes.hip, PT_C2_D; profiles/r10a_corr2_feature_stream.txt).

Only WHEN a feature k-step is requested changed, and which copy of the loop a wave runs: every element still runs through one
accumulator with the k-steps in order, the tap planes, the shift-and-add and the slice sums are the same.  So every route of the
correlation pass must produce the bits it produced before.  The reference is what the library computed before the change
(tests/golden/corr2_stream_*.npz, recorded from the parent build on the same seeded inputs by this file's `--record`, with PT_HOT_LIB naming that build), at the
smallest shapes that reach each loop body; the plan of each shape is asserted, so that a case cannot drift onto another body:

  pass_mix128 / pass_mix512  mixed sample pairs (half 0 + leftover quads, half 1, full tiles), 4 and 16 k-steps
  pass_pair                  plain sample pairs (16 x 16: four full tiles, no leftover quads)
  pass_halves                one sample per workgroup, two k-step halves per tile
  pass_wide                  one wave per tile with all k-steps (22 x 22)
  pass_c64                   64-channel samples: one channel range, k-step halves of 8 k-steps (the arms under the 80-VGPR cap)
  pass_1x1                   a filter of another size than 4 x 4 (K16 false)
  frame_slot0 / frame_last   the DiMP-50 frame at n = 34: the plain pass with the memory insert riding on it (first and last slot; the
                             slot's stored features are bit-equal to the source) and the passes with the fused reduction of 8 gradient
                             partials, through a 3-iteration solve
  chain                      four chained frames with the last update deferred into the next frame's first pass, then the flush"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

FIELDS = ("ok", "tiles", "nh", "spw", "mix", "threads", "NK", "KSC", "lds", "left")
# case -> ((n, C, H, W, K), the plan fields that select the kernel instantiation and its loop bodies)
PASS_CASES = {
    "pass_mix128": ((34, 128, 18, 18, 4), dict(mix=1, spw=2, nh=1, NK=4, left=1)),
    "pass_mix512": ((34, 512, 18, 18, 4), dict(mix=1, spw=2, nh=1, NK=16, left=1)),
    "pass_pair": ((34, 128, 16, 16, 4), dict(mix=0, spw=2, nh=1, NK=4, left=0)),
    "pass_halves": ((3, 128, 18, 18, 4), dict(mix=0, spw=1, nh=2, NK=2, left=1)),
    "pass_wide": ((2, 128, 22, 22, 4), dict(mix=0, spw=1, nh=1, NK=4, left=0)),
    "pass_c64": ((2, 64, 18, 18, 4), dict(mix=0, spw=1, nh=2, NK=8, KSC=1, left=1)),
    "pass_1x1": ((2, 256, 18, 18, 1), dict(mix=0, spw=1, nh=2, NK=4, left=1)),
}
FRAME_N = 34
FRAME_CASES = {"frame_slot0": 0, "frame_last": FRAME_N - 1}
DEV = "cuda:0"


def plan(n, C, H, W, K):
    from pytracking_amd import _lib
    out = (ctypes.c_int * 10)()
    assert _lib.lib().pt_corr_pass_plan(n, C, H, W, K, K, H + 1 - K % 2, W + 1 - K % 2, out) == 0
    return dict(zip(FIELDS, out))


def pass_outputs(case):
    import torch
    from pytracking_amd import filter as F, synth
    (n, C, H, W, K), want = PASS_CASES[case]
    p = plan(n, C, H, W, K)
    assert p["ok"] == 1 and {k: p[k] for k in want} == want, (case, p)
    rng = np.random.default_rng(10100 + sorted(PASS_CASES).index(case))
    feat = synth.clf_features(rng, n, C, H, W, 4)
    filt = rng.standard_normal((C, K, K), dtype=np.float32) * np.float32(0.5 / np.sqrt(C * K * K))
    ft = torch.from_numpy(feat).to(DEV)
    assert ft.data_ptr() % 16 == 0                                   # the fast route
    return {"scores": F.corr_raw(ft, torch.from_numpy(filt).to(DEV)).cpu().numpy()}


def _frame_state():
    from pytracking_amd import _lib, bench_frame, synth
    cfg = dict(synth.DIMP50)
    p = plan(FRAME_N, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    assert (p["ok"], p["mix"], p["NK"], p["left"]) == (1, 1, 16, 1), p
    adj = (ctypes.c_int * 11)()                                     # out[4]: position slices of the adjoint pass = gradient partials
    assert _lib.lib().pt_adj_pass_plan(FRAME_N, cfg["C"], cfg["H"], cfg["W"], cfg["K"], cfg["K"], cfg["H"] + 1, cfg["W"] + 1, adj) == 0
    assert (adj[0], adj[4]) == (1, 8), list(adj)                    # the solve's correlation passes sum 8 partials (FUSE = 8)
    return cfg, bench_frame.TrackState(cfg, FRAME_N, seed=10311, device=DEV)


def _state_arrays(st):
    return {k: getattr(st, k).cpu().numpy().copy() for k in ("scores", "filter", "peak", "mem_bb")}


def frame_outputs(case):
    import torch
    from pytracking_amd import synth
    slot = FRAME_CASES[case]
    cfg, st = _frame_state()
    x = synth.clf_features(np.random.default_rng(10312 + slot), 1, cfg["C"], cfg["H"], cfg["W"], cfg["K"])[0]
    st.step(torch.from_numpy(x).to(DEV), slot=slot, num_iter=3)
    torch.cuda.synchronize()
    out = _state_arrays(st)
    stored = st.mem_feat[slot].cpu().numpy()
    assert np.array_equal(stored.view(np.int32), x.view(np.int32)), "memory insert: the slot's features differ from the source"
    return out


def chain_outputs():
    import torch
    from pytracking_amd import synth
    cfg, st = _frame_state()
    xs = synth.clf_features(np.random.default_rng(10400), 4, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    out = {}
    for f in range(4):
        st.step(torch.from_numpy(xs[f]).to(DEV), slot=(5 + f) % FRAME_N, num_iter=3, defer=True)
        torch.cuda.synchronize()
        assert st.pending.iters > 0, "the frame did not take the chain's path"
        out["scores%d" % f] = st.scores.cpu().numpy().copy()
        out["peak%d" % f] = st.peak.cpu().numpy().copy()
    st.flush()
    torch.cuda.synchronize()
    out.update(_state_arrays(st))
    return out


def outputs(case):
    if case in PASS_CASES:
        return pass_outputs(case)
    return chain_outputs() if case == "chain" else frame_outputs(case)


ALL_CASES = sorted(PASS_CASES) + sorted(FRAME_CASES) + ["chain"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES)
def test_correlation_pass_keeps_its_bits(case):
    want = np.load(os.path.join(GOLDEN, "corr2_stream_" + case + ".npz"))
    got = outputs(case)
    assert sorted(got) == sorted(want.files), (sorted(got), sorted(want.files))
    bad = {}
    for k in sorted(got):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (case, k)
        assert np.isfinite(a).all() and np.abs(b).max() > 0, (case, k)
        diff = a.view(np.int32) != b.view(np.int32)
        print(f"{case}.{k}: {int(diff.sum())} of {diff.size} elements differ in bits from the recorded result of the parent "
              f"(max abs difference {float(np.abs(a - b).max()):.3e})")
        if diff.any():
            bad[k] = int(diff.sum())
    assert not bad, (case, bad)


if __name__ == "__main__":                                          # --record [DIR]: write the golden files from the library in use
    assert sys.argv[1:2] == ["--record"], "usage: python tests/test_gpu_corr2_feature_stream.py --record [DIR]"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    for case in ALL_CASES:
        arrays = outputs(case)
        path = os.path.join(out_dir, "corr2_stream_" + case + ".npz")
        np.savez_compressed(path, **arrays)
        print(case, {k: v.shape for k, v in arrays.items()}, os.path.getsize(path), "bytes")
