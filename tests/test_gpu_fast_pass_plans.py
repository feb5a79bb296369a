"""Every plan cell of the XCD-aligned feature passes (k_corr2 / k_adj2, csrc/fast_passes.hip) and of the steepest-descent solve on them, on
the MI355X: the cases of tests/fast_pass_cases.py through pytracking_amd.filter (pt_apply_filter_f32, pt_feat_transpose_f32) and the
optimizer modules (pt_sd_solve_f32) against the same operation in float64 on the CPU.

  (a) random data: scores within 2e-5, the adjoint within 2e-5 * max(1, |ref|max) -- the project's flat bounds -- and both within
      FACTOR x max(the fp32 CPU evaluation's own distance from float64 on the case, one fp32 ulp of the output's range), the bound of
      tests/f64_bound.py with its spacing_of_max floor; two calls
      bit-identical; <F w, r> = <w, F^T r>.
  (b) structured data: one-hot channels against power-of-two taps and small-integer residual maps.  The float64 reference is integral and
      below 2^24, so every summation order is exact and the device result must be EQUAL.
  (c) the solver cases against oracle.np_oracle in float64: iterates within 2e-5, losses within 2e-5 absolute + 1e-4 relative, with the
      same oracle's fp32 distance from float64 printed beside every case.

Every test prints its figures before it asserts (run with -s); with FAST_PASSES_F64_OUT set the table is written to that file
(profiles/fast_passes_f64.txt).  Needs no reference tree."""
import numpy as np
import pytest
import torch

import fast_pass_cases as FP
import f64_bound
from pytracking_amd import _lib, filter as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = ["-".join(str(v) for v in c[0]) for c in FP.CASES]
TABLE = f64_bound.Table("FAST_PASSES_F64_OUT",
                        "XCD-aligned feature passes and the steepest-descent solve on gfx950 against float64 (tests/test_gpu_fast_pass_plans.py -s).\n"
                        "passes: max |out - float64| per case (n-C-H-W-K-out-sf) and output, ref_err = the fp32 CPU evaluation's own distance from\n"
                        f"float64 (torch conv2d, {FP.THREADS} threads), floor = one fp32 ulp of the output's range, ratio = err / max(ref_err, floor);\n"
                        f"bound {f64_bound.FACTOR}, and the worst ratio is that of the passes.\n"
                        "solver: max |iterates - float64 oracle| (bound 2e-5), max |losses - float64 oracle|, and the fp32 oracle's own distances.")


def _dev_problem(case, feat, filt, r):
    """Device operands, 16-byte aligned; sf == 2: the features are sequence 1 of a (n, 2, C, H, W) tensor whose sequence 0 holds 1e3."""
    n, C, H, W, K, out, sf = case
    if sf == 1:
        fd = torch.tensor(feat, device=DEV)
    else:
        f5 = torch.full((n, sf, C, H, W), 1e3, device=DEV)
        f5[:, 1] = torch.tensor(feat, device=DEV)
        fd = f5[:, 1]
    wd, rd = torch.tensor(filt, device=DEV), torch.tensor(r, device=DEV)
    # the predicate of the fast route (pt_fast_usable): the plan covers the shape, 16-byte aligned operands, sample stride % 4, 31 bits
    assert fd.stride() == (sf * C * H * W, H * W, W, 1) and fd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    assert fd.stride(0) % 4 == 0 and n * fd.stride(0) * 4 < 2 ** 31
    return fd, wd, rd


def _on_its_cell(idx):
    case, corr, adj = FP.CASES[idx]
    assert FP.cells(_lib.lib(), *case) == (corr, adj), (case, FP.cells(_lib.lib(), *case))
    return case


def _where_corr(case, got, ref):
    """The worst score, located in the plan: sample (and member of the pair), and for the feature position under the filter's centre
    tap its 64-position tile, quad and lane of the quad."""
    n, C, H, W, K, out, sf = case
    g = FP.geometry(_lib.lib(), *case)
    d = np.abs(got - ref)
    i, y, x = (int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))
    p = min(y, H - 1) * W + min(x, W - 1)
    return (f"scores: max |gpu - float64| = {float(d.max()):.3e} at (sample {i}{f' = member {i % 2} of pair {i // 2}' if g['spw'] == 2 else ''}, "
            f"row {y}, col {x}) gpu {got[i, y, x]!r} float64 {ref[i, y, x]!r}; position {p}: tile {p // 64} of {g['tiles']} "
            f"({'leftover quads' if g['tail'] == 'left' and p >= 64 * g['TF'] else 'partial tile' if p >= 64 * g['TF'] else 'full tile'}), "
            f"quad {(p % 64) // 4}, lane {p % 4} of the quad; nh {g['nh']} mix {g['mix']}; {int((d > 0).sum())} of {d.size} elements differ")


def _where_adj(case, got, ref, hot=None):
    """The worst gradient element: channel, its 16-channel block and XCD, the tap; with one-hot features also the position slices that
    hold that channel's hot position of every sample."""
    n, C, H, W, K, out, sf = case
    g = FP.geometry(_lib.lib(), *case)
    d = np.abs(got - ref)
    c, u, v = (int(q) for q in np.unravel_index(int(np.argmax(d)), d.shape))
    cb = c // 16
    msg = (f"adjoint: max |gpu - float64| = {float(d.max()):.3e} at (channel {c}, tap ({u}, {v})) gpu {got[c, u, v]!r} float64 {ref[c, u, v]!r}; "
           f"channel block {cb} of {g['CB']} (XCD {cb // g['bpx'] if g['bpx'] else cb % 8}), {g['KSPL']} slices of {g['gper']} groups; "
           f"{int((d > 0).sum())} of {d.size} elements differ")
    if hot is not None:
        sl = sorted({(i * H * W + hot[(c + 3 * i) % len(hot)]) // (g["gper"] * 16) for i in range(n)})
        msg += f"; slices that hold channel {c}'s hot positions: {sl[:12]}{' ...' if len(sl) > 12 else ''}"
    return msg


@pytest.mark.parametrize("idx", range(len(FP.CASES)), ids=IDS)
def test_random_data_matches_float64(idx):
    case = _on_its_cell(idx)
    n, C, H, W, K, out, sf = case
    feat, filt, r = FP.random_problem(idx)
    (s64, g64), (s_err, g_err) = FP.reference(idx, feat, filt, r, "rand")
    fd, wd, rd = _dev_problem(case, feat, filt, r)
    ohw = FP.out_size(H, W, K, out)
    s, s2 = F.corr_raw(fd, wd, out_hw=ohw), F.corr_raw(fd, wd, out_hw=ohw)
    a, a2 = F.adj_raw(fd, rd, (K, K)), F.adj_raw(fd, rd, (K, K))
    sg, ag = s.double().cpu().numpy(), a.double().cpu().numpy()
    assert sg.shape == s64.shape and ag.shape == g64.shape
    tag = IDS[idx]
    flat_a = 2e-5 * max(1.0, float(np.abs(g64).max()))
    msg = f"{FP.CASES[idx]}\n{_where_corr(case, sg, s64)}\n{_where_adj(case, ag, g64)}"
    assert np.isfinite(sg).all() and np.isfinite(ag).all(), msg
    f64_bound.held(tag + " corr", sg, s64, s_err, floor=f64_bound.spacing_of_max, flat=2e-5, table=TABLE, msg=msg)
    f64_bound.held(tag + " adj", ag, g64, g_err, floor=f64_bound.spacing_of_max, flat=flat_a, table=TABLE, msg=msg)
    assert torch.equal(s, s2) and torch.equal(a, a2), f"{tag}: two calls differ"           # fixed-order sums: bit-identical
    lhs, rhs = float((sg * r.astype(np.float64)).sum()), float((ag * filt.astype(np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs)), (tag, lhs, rhs)                     # <F w, r> = <w, F^T r>


@pytest.mark.parametrize("idx", range(len(FP.CASES)), ids=IDS)
def test_structured_data_is_exact(idx):
    """A shifted tile, a swapped tap, a lost channel range or k-step half, the wrong sample of a pair or a mis-cut position slice is a
    whole-number error here."""
    case = _on_its_cell(idx)
    n, C, H, W, K, out, sf = case
    feat, filt, r, hot = FP.structured_problem(_lib.lib(), idx)
    assert len(hot) <= C and all(0 <= p < H * W for p in hot)                              # every sample meets every hot spot
    ohw = FP.out_size(H, W, K, out)
    s64, g64 = FP.corr_cpu(feat, filt, ohw, torch.float64), FP.adj_cpu(feat, r, K, torch.float64)
    for ref in (s64, g64):
        assert np.array_equal(ref, np.round(ref)) and 0 < float(np.abs(ref).max()) < 2 ** 24, float(np.abs(ref).max())
    fd, wd, rd = _dev_problem(case, feat, filt, r)
    sg = F.corr_raw(fd, wd, out_hw=ohw).double().cpu().numpy()
    ag = F.adj_raw(fd, rd, (K, K)).double().cpu().numpy()
    msg = f"{FP.CASES[idx]}, {len(hot)} hot spots {hot}\n{_where_corr(case, sg, s64)}\n{_where_adj(case, ag, g64, hot)}"
    print(f"\nstructured {IDS[idx]}: scores up to {float(s64.max()):.0f}, gradient up to {float(g64.max()):.0f}; "
          f"{int((sg != s64).sum())} + {int((ag != g64).sum())} elements differ (exact expected)")
    assert np.array_equal(sg, s64), msg
    assert np.array_equal(ag, g64), msg


# ---- solver ------------------------------------------------------------------------------------------------------------------------
def _module(v):
    from pytracking_amd import optimizer
    if v in (FP.V_RELU, FP.V_BENT):
        return optimizer.DiMPSteepestDescentGN(num_iter=3, feat_stride=16, init_step_length=0.9, init_filter_reg=0.1, init_gauss_sigma=0.9,
                                               num_dist_bins=100, bin_displacement=0.1, mask_init_factor=3.0,
                                               score_act="bentpar" if v == FP.V_BENT else "relu", act_param=2.0 if v == FP.V_BENT else None,
                                               min_filter_reg=1e-3).to(DEV).eval()
    if v == FP.V_L2:
        return optimizer.DiMPL2SteepestDescentGN(num_iter=3, feat_stride=16, init_step_length=1.0, gauss_sigma=1.0, hinge_threshold=0.05,
                                                 init_filter_reg=0.1, min_filter_reg=1e-3).to(DEV).eval()
    return optimizer.PrDiMPSteepestDescentNewton(num_iter=3, feat_stride=16, init_step_length=1.0, init_filter_reg=0.05, gauss_sigma=0.9,
                                                 min_filter_reg=0.05, alpha_eps=0.05, normalize_label=True, softmax_reg=0.1).to(DEV).eval()


@pytest.mark.parametrize("case", FP.SOLVER_CASES, ids=lambda c: f"{FP.V_NAMES[c[0]]}-{c[1]}")
def test_solver_case_matches_float64_oracle(case):
    v, tag, has_sw, iters, seed = case
    (n, C, H, W, K), want = FP.SOLVER_SHAPES[tag]
    L = _lib.lib()
    w0, feat, bb, sw = FP.solver_problem(case)
    T = f64_bound.dev
    wd, fd = T(w0)[None], T(feat)
    mod = _module(v)
    outs = {}
    for compute_losses in (True, False):
        # the route of exactly this call: the solve's own predicate on the pointers it gets (the iterate buffer comes from the allocator: aligned)
        rc, route = FP.solve_route(L, v, n, C, H, W, K, compute_losses, ptr=fd.data_ptr())
        assert rc == 0 and route == [1, v, want[1], int(compute_losses)] and wd.data_ptr() % 16 == 0, (rc, route)
        with torch.no_grad():
            w, its, losses = mod(wd, fd, T(bb), sample_weight=T(sw), num_iter=iters, compute_losses=compute_losses)
        outs[compute_losses] = (torch.stack([i[0] for i in its]), torch.cat(losses) if losses else None)
    its, losses = outs[True]
    assert outs[False][1] is None and torch.equal(its, outs[False][0])                     # the loss flag is side-effect free
    i64, l64 = FP.solver_oracle(case, np.float64)
    i32, l32 = FP.solver_oracle(case, np.float32)
    ig, lg = its.double().cpu().numpy(), losses.double().cpu().numpy()
    e_i, e_l = float(np.abs(ig - i64).max()), float(np.abs(lg - l64).max())
    o_i, o_l = float(np.abs(i32 - i64).max()), float(np.abs(l32 - l64).max())
    name = f"solve {FP.V_NAMES[v]}-{tag}{'-sw' if has_sw else ''}"
    TABLE.row(name + " iterates", e_i, o_i, f64_bound.spacing_of_max(i64), e_i / max(o_i, 1e-30), bounded=False)
    TABLE.row(name + " losses", e_l, o_l, f64_bound.spacing_of_max(l64), e_l / max(o_l, 1e-30), bounded=False)
    print(f"\n{name} {(n, C, H, W, K)} x {iters} iterations, route {want}: max |iterates - float64| {e_i:.3e} (fp32 oracle {o_i:.3e}, bound 2e-5), "
          f"max |losses - float64| {e_l:.3e} (fp32 oracle {o_l:.3e}); losses {l64[0]:.4f} -> {l64[-1]:.4f}")
    assert np.isfinite(ig).all() and np.isfinite(lg).all()
    assert o_i <= 2e-5 and np.all(np.abs(l32 - l64) <= 2e-5 + 1e-4 * np.abs(l64)), "the seed: the fp32 oracle itself misses the bound"
    assert e_i <= 2e-5, (name, e_i)
    np.testing.assert_allclose(lg, l64, atol=2e-5, rtol=1e-4)
