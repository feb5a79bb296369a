"""k_adj2 keeps its bits with the feature loads of its MFMA loop pinned five groups ahead (csrc/fast_passes.hip, PT_ADJ_AHEAD;
profiles/r09a_adj2_wave_anatomy.txt).

Only WHEN a feature group is requested changed: every G[c][tap] still runs through the same two accumulators in the same group order,
the partials of the waves and of the position slices are summed in the same order.  So the adjoint pass and the whole steepest-descent
solve must produce the bits they produced before, at the sizes the trackers run:

  * the plain adjoint (pt_feat_transpose_f32: k_adj2<0, ..>) at the DiMP-50, PrDiMP-50 and ATOM shapes;
  * the solve (pt_sd_solve_f32: k_adj2<1, 6, 16> for DiMP-50, k_adj2<4, 9, ..> for PrDiMP-50).

The reference is what the library computed before the change (tests/golden/adj2_prefetch_*.npz, recorded from the parent build on the
same seeded inputs).  The generic k_adj route cannot serve: it sums the positions in another order and was not bit-equal to the fast
route before the change either (7393 of 8192 elements differ at the DiMP-50 shape, profiles/r09a_adj2_wave_anatomy.txt).  Each case
also runs the generic route (a feature pointer that is not 16-byte aligned takes it) and asserts that it differs in bits and agrees
to rounding: the aligned call really took the fast route, and the two routes compute the same thing."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

# case -> (n, C, H, W); K = 4 everywhere
ADJ_CASES = {"adj_dimp50": (50, 512, 18, 18), "adj_prdimp50": (50, 512, 22, 22), "adj_atom": (250, 64, 18, 18)}
SOLVE_CASES = {"solve_dimp50": "dimp", "solve_prdimp50": "prdimp"}


def _views(feat, dev):
    """The same features twice: 16-byte aligned (fast route) and 4 bytes off (generic route)."""
    import torch
    src = torch.from_numpy(feat)
    out = []
    for off in (0, 1):
        buf = torch.zeros(feat.size + 4, device=dev)
        v = buf[off:off + feat.size].view(feat.shape)
        v.copy_(src)
        assert v.data_ptr() % 16 == 4 * off
        out.append(v)
    return out


def adj_outputs(case):
    """(fast, generic) gradient of the plain adjoint pass, (C, 4, 4) each."""
    import torch
    from pytracking_amd import filter as F, synth
    n, C, H, W = ADJ_CASES[case]
    rng = np.random.default_rng(9100 + sorted(ADJ_CASES).index(case))
    feat = synth.clf_features(rng, n, C, H, W, 4)
    r = rng.standard_normal((n, H + 1, W + 1), dtype=np.float32)
    dev = "cuda:0"
    al, mis = _views(feat, dev)
    rt = torch.from_numpy(r).to(dev)
    return F.adj_raw(al, rt, (4, 4)).cpu().numpy(), F.adj_raw(mis, rt, (4, 4)).cpu().numpy()


def solve_outputs(case):
    """(fast, generic) filter iterates of a 5-iteration solve, (6, 512, 4, 4) each."""
    import torch
    from pytracking_amd import optimizer, synth
    dev = "cuda:0"
    if SOLVE_CASES[case] == "dimp":
        c = synth.DIMP50
        mod = optimizer.DiMPSteepestDescentGN(
            num_iter=c["num_iter"], feat_stride=c["feat_stride"], init_step_length=c["init_step_length"],
            init_filter_reg=c["init_filter_reg"], init_gauss_sigma=c["init_gauss_sigma"], num_dist_bins=c["num_dist_bins"],
            bin_displacement=c["bin_displacement"], mask_init_factor=c["mask_init_factor"], score_act=c["score_act"],
            mask_act=c["mask_act"], min_filter_reg=c["min_filter_reg"], alpha_eps=c["alpha_eps"])
        w0, feat, bb, sw = synth.dimp_problem(9201, 50)
    else:
        c = synth.PRDIMP50
        mod = optimizer.PrDiMPSteepestDescentNewton(
            num_iter=c["num_iter"], feat_stride=c["feat_stride"], init_step_length=c["init_step_length"],
            init_filter_reg=c["init_filter_reg"], gauss_sigma=c["gauss_sigma"], min_filter_reg=c["min_filter_reg"],
            alpha_eps=c["alpha_eps"], init_uni_weight=c["init_uni_weight"], normalize_label=c["normalize_label"],
            label_shrink=c["label_shrink"], softmax_reg=c["softmax_reg"], label_threshold=c["label_threshold"])
        w0, feat, bb, sw = synth.dimp_problem(9202, 50, synth.PRDIMP50)
        w0 = w0 * 0
    mod = mod.to(dev).eval()
    assert feat.shape[1:] == (512, c["H"], c["W"]) and feat.shape[0] == 50
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    res = []
    for v in _views(np.ascontiguousarray(feat, dtype=np.float32), dev):
        with torch.no_grad():
            _, its, _ = mod(T(w0)[None], v, T(bb), sample_weight=T(sw), num_iter=5, compute_losses=False)
        res.append(torch.stack([i[0] for i in its]).cpu().numpy())
    return res


def _check(case, fast, generic):
    want = np.load(os.path.join(GOLDEN, "adj2_prefetch_" + case + ".npz"))["fast"]
    assert fast.shape == want.shape and fast.dtype == want.dtype == np.float32
    diff = fast.view(np.int32) != want.view(np.int32)
    gdiff = fast.view(np.int32) != generic.view(np.int32)
    gerr = float(np.abs(fast - generic).max())
    print(f"{case}: {int(diff.sum())} of {diff.size} elements differ in bits from the recorded result of the parent (max abs difference "
          f"{float(np.abs(fast - want).max()):.3e}); {int(gdiff.sum())} differ from the generic route (max abs difference {gerr:.3e})")
    assert np.abs(want).max() > 0 and np.isfinite(fast).all()
    assert not diff.any(), (case, int(diff.sum()))
    # another summation order, the same sums: float32 rounding of sums of ~n*H*W terms, far inside the project's 1e-4 parity bound
    assert gdiff.any() and gerr < 1e-4 * max(1.0, float(np.abs(want).max())), (case, int(gdiff.sum()), gerr)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ADJ_CASES))
def test_plain_adjoint_keeps_its_bits(case):
    _check(case, *adj_outputs(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SOLVE_CASES))
def test_solve_keeps_its_bits(case):
    _check(case, *solve_outputs(case))
