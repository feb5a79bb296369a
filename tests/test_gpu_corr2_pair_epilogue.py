"""k_corr2 keeps its bits with the one-round shift-and-add of the mixed sample pairs (csrc/fast_passes.hip, PT_C2_SA1;
profiles/r12a_pass_wave_arbitration.txt).

A mixed-pair workgroup whose thread count covers 2 * roundup64(OH * OW) outputs runs the shift-and-add of both samples at once, the
first half of its waves on the pair's first sample and the second half on the second; otherwise it keeps one round per sample.  Inside
an output nothing is reordered, so every score must keep the bits it had.  The reference is what the library computed before the change
(tests/golden/corr2_epilogue_*.npz, recorded from the parent build on the same seeded inputs by this file's `--record`, with
PT_HOT_LIB naming that build), at the smallest shapes that reach each route of the epilogue; the plan of every case is asserted:

  one_round        34 x 128 x 16 x 20, K = 4   mixed pair, five full tiles, OO = 357: 2 * 384 <= 768 threads
  one_round_part   34 x 128 x 16 x 18, K = 4   mixed pair with a partial fifth tile, OO = 323
  two_rounds       34 x 128 x 8 x 42, K = 4    mixed pair with leftover quads, OO = 387: 2 * 448 > 768, the two rounds stay (the plan takes no
                                              6 x 54 map; of the mixed pairs it takes with more than 384 outputs this is the smallest)
  plain_pair       34 x 128 x 18 x 18, K = 3   no mixed pair (9 taps): code the change does not touch"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

FIELDS = ("ok", "tiles", "nh", "spw", "mix", "threads", "NK", "KSC", "lds", "left")
# case -> ((n, C, H, W, K), plan fields, does the workgroup run both samples in one round)
CASES = {
    "one_round": ((34, 128, 16, 20, 4), dict(mix=1, spw=2, nh=1, tiles=5, threads=768, left=0), True),
    "one_round_part": ((34, 128, 16, 18, 4), dict(mix=1, spw=2, nh=1, tiles=5, threads=768, left=0), True),
    "two_rounds": ((34, 128, 8, 42, 4), dict(mix=1, spw=2, nh=1, tiles=5, threads=768, left=1), False),
    "plain_pair": ((34, 128, 18, 18, 3), dict(mix=0, spw=2), None),
}
DEV = "cuda:0"


def plan(n, C, H, W, K):
    from pytracking_amd import _lib
    out = (ctypes.c_int * 10)()
    assert _lib.lib().pt_corr_pass_plan(n, C, H, W, K, K, H + 1 - K % 2, W + 1 - K % 2, out) == 0
    return dict(zip(FIELDS, out))


def check_plan(case):
    (n, C, H, W, K), want, one_round = CASES[case]
    p = plan(n, C, H, W, K)
    assert p["ok"] == 1 and {k: p[k] for k in want} == want, (case, p)
    if one_round is not None:
        oo = (H + 1) * (W + 1)
        assert (2 * ((oo + 63) // 64 * 64) <= p["threads"]) == one_round, (case, oo, p["threads"])


def outputs(case):
    import torch
    from pytracking_amd import filter as F, synth
    (n, C, H, W, K), _, _ = CASES[case]
    check_plan(case)
    rng = np.random.default_rng(12100 + sorted(CASES).index(case))
    feat = synth.clf_features(rng, n, C, H, W, 4)
    filt = rng.standard_normal((C, K, K), dtype=np.float32) * np.float32(0.5 / np.sqrt(C * K * K))
    ft = torch.from_numpy(feat).to(DEV)
    assert ft.data_ptr() % 16 == 0                                   # the fast route
    return F.corr_raw(ft, torch.from_numpy(filt).to(DEV)).cpu().numpy()


def _differ(a, b):
    return int((a.view(np.int32) != b.view(np.int32)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_pair_epilogue_keeps_its_bits(case):
    (n, C, H, W, K), _, _ = CASES[case]
    want = np.load(os.path.join(GOLDEN, "corr2_epilogue_" + case + ".npz"))["scores"]
    got = outputs(case)
    assert got.shape == want.shape == (n, H + 1 - K % 2, W + 1 - K % 2) and got.dtype == want.dtype == np.float32, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    # every sample must carry a map of its own: a round that wrote the wrong sample's slot would still be "some recorded map"
    assert len({want[i].tobytes() for i in range(n)}) == n
    first, last, every = _differ(got[0], want[0]), _differ(got[n - 1], want[n - 1]), _differ(got, want)
    print(f"{case}: elements that differ in bits from the recorded result of the parent: first sample {first}, last sample {last}, "
          f"all {every} of {got.size} (max abs difference {float(np.abs(got - want).max()):.3e})")
    assert first == 0, (case, "scores[0]", first)
    assert last == 0, (case, "scores[%d]" % (n - 1), last)
    assert every == 0, (case, every)


if __name__ == "__main__":                                          # --record [DIR]: write the golden files from the library in use
    assert sys.argv[1:2] == ["--record"], "usage: python tests/test_gpu_corr2_pair_epilogue.py --record [DIR]"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    for case in sorted(CASES):
        scores = outputs(case)
        path = os.path.join(out_dir, "corr2_epilogue_" + case + ".npz")
        np.savez_compressed(path, scores=scores)
        print(case, scores.shape, os.path.getsize(path), "bytes")
