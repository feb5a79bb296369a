"""GPU parity: the HIP path (through the C ABI) against the numpy oracle and the reference-generated golden
vectors on identical seeded inputs.  Tolerance: BASELINE.json north_star asks for 1e-4 abs on score maps /
filters; 2e-5 is asserted where the arithmetic is smooth, 1e-4 where a sign(s) flip of a near-zero score can
move an iterate discontinuously (LeakyReluParDeriv, activation.py:43-44)."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import np_oracle as O
from pytracking_amd import synth
from tomp_cases import build_tomp_modules               # shared with tests/test_gpu_tomp_routes.py

pytestmark = pytest.mark.gpu

DEV = "cuda"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, b, atol, rtol=0.0):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    np.testing.assert_allclose(a.astype(np.float64), np.asarray(b, dtype=np.float64), atol=atol, rtol=rtol)


# ------------------------------------------------------------------------------------------------------
# filter layer
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["k4", "k3", "k1"])
def test_apply_filter_and_transpose_golden(tag):
    from pytracking_amd import filter as F
    g = load_golden("filter_ops")
    feat, filt = T(g[f"{tag}_feat"]), T(g[f"{tag}_filt"][None])
    s = F.apply_filter(feat, filt)
    assert s.shape == (feat.shape[0], 1) + g[f"{tag}_scores"].shape[1:]
    close(s[:, 0], g[f"{tag}_scores"], atol=2e-5)
    K = filt.shape[-1]
    adj = F.apply_feat_transpose(feat, T(g[f"{tag}_inp"])[:, None], (K, K), training=False)
    close(adj[0], g[f"{tag}_adj_v2"], atol=1e-4)


def test_apply_filter_two_sequences_and_errors():
    from pytracking_amd import filter as F
    g = load_golden("filter_ops")
    s = F.apply_filter(T(g["s2_feat"]), T(g["s2_filt"]))
    close(s, g["s2_scores"], atol=2e-5)
    adj = F.apply_feat_transpose(T(g["s2_feat"]), T(g["s2_inp"]), 4, training=False)
    close(adj, g["s2_adj"], atol=1e-4)
    with pytest.raises(RuntimeError, match="not covered"):
        F.apply_filter(T(g["k5_feat"]), T(g["k5_filt"][None]))          # 25 taps > 16
    # multi-filter (LWL) branch: feat (n,1,C,H,W), filter (1,F,C,K,K)
    s = F.apply_filter(T(g["mf_feat"])[:, None], T(g["mf_filt"])[None])
    close(s[:, 0], g["mf_scores"], atol=2e-5)
    adj = F.apply_feat_transpose(T(g["mf_feat"])[:, None], T(g["mf_inp"])[:, None], 3, training=False)
    close(adj[0], g["mf_adj"], atol=1e-4)


@pytest.mark.parametrize("n,C,H,W,K", [(1, 512, 18, 18, 4), (50, 512, 18, 18, 4), (7, 64, 22, 22, 4),
                                       (3, 20, 9, 7, 3), (2, 33, 5, 6, 2), (5, 256, 18, 18, 1),
                                       # XCD-aligned fast path: trailing-quad trick (rem 1 and 4), no remainder,
                                       # regular partial tile (22x22: rem 9), every channel count, odd/even K.  A sample of
                                       # its plan space: tests/fast_pass_cases.py holds one case per reachable plan cell of
                                       # both passes (tests/test_gpu_fast_pass_plans.py, tests/test_fast_pass_plans_cpu.py)
                                       (3, 128, 18, 18, 4), (5, 256, 22, 22, 4), (2, 128, 10, 8, 4),
                                       (2, 128, 16, 16, 4), (3, 256, 12, 12, 3), (2, 128, 20, 20, 4),
                                       (1, 1024, 18, 18, 4), (4, 128, 14, 14, 2), (9, 128, 18, 16, 4),
                                       (50, 512, 22, 22, 4), (33, 128, 8, 8, 4)])
def test_filter_ops_vs_oracle(n, C, H, W, K):
    from pytracking_amd import filter as F
    rng = np.random.default_rng(n * 1000 + C)
    feat = synth.clf_features(rng, n, C, H, W, max(K, 1))
    filt = rng.standard_normal((C, K, K), dtype=np.float32) * 0.05
    s = F.apply_filter(T(feat), T(filt[None]))[:, 0]
    ref = O.apply_filter(feat.astype(np.float64), filt.astype(np.float64))
    close(s, ref, atol=2e-5)
    inp = rng.standard_normal(ref.shape).astype(np.float32)
    adj = F.apply_feat_transpose(T(feat), T(inp)[:, None], (K, K))[0]
    refa = O.apply_feat_transpose(feat.astype(np.float64), inp.astype(np.float64), K)
    close(adj, refa, atol=2e-5 * max(1.0, np.abs(refa).max()))
    # adjointness <F w, r> == <w, F^T r>  (size-independent property)
    lhs = float((s.double().cpu() * torch.from_numpy(inp).double()).sum())
    rhs = float((adj.double().cpu() * torch.from_numpy(filt).double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs))


def test_apply_filter_same_crop_and_autograd_pair():
    from pytracking_amd import filter as F
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((4, 16, 18, 18), dtype=np.float32)
    filt = rng.standard_normal((16, 4, 4), dtype=np.float32)
    s = F.corr_raw(T(feat), T(filt), out_hw=(18, 18))                     # operation.conv2d(mode='same')
    close(s, O.apply_filter(feat.astype(np.float64), filt.astype(np.float64), out_hw=(18, 18)), atol=1e-4)
    # ATOM's per-frame classification shape (atom.py:300-302): 64 compressed channels, 4x4 filter, 'same' crop; equals
    # stock F.conv2d(padding=2)[..., :-1, :-1] (operation.py:17-32)
    x = T(rng.standard_normal((1, 64, 18, 18), dtype=np.float32))
    w = T(rng.standard_normal((1, 64, 4, 4), dtype=np.float32) * 0.05)
    want = torch.nn.functional.conv2d(x, w, padding=2)[:, :, :-1, :-1]
    close(F.corr_raw(x, w[0], out_hw=(18, 18)).unsqueeze(1), want.cpu().numpy(), atol=2e-5)
    # autograd: d/dfilter <apply_filter(feat, filter), r> = apply_feat_transpose(feat, r)
    w = T(filt[None]).requires_grad_(True)
    r = T(rng.standard_normal((4, 1, 19, 19), dtype=np.float32))
    (F.apply_filter(T(feat), w) * r).sum().backward()
    close(w.grad[0], O.apply_feat_transpose(feat.astype(np.float64), r[:, 0].cpu().numpy().astype(np.float64), 4),
          atol=1e-3)


# ------------------------------------------------------------------------------------------------------
# steepest-descent solvers
# ------------------------------------------------------------------------------------------------------
def _dimp_module(cfg=synth.DIMP50, **over):
    from pytracking_amd import optimizer
    c = dict(cfg, **over)
    return optimizer.DiMPSteepestDescentGN(
        num_iter=c["num_iter"], feat_stride=c["feat_stride"], init_step_length=c["init_step_length"],
        init_filter_reg=c["init_filter_reg"], init_gauss_sigma=c["init_gauss_sigma"], num_dist_bins=c["num_dist_bins"],
        bin_displacement=c["bin_displacement"], mask_init_factor=c["mask_init_factor"], score_act=c["score_act"],
        mask_act=c["mask_act"], min_filter_reg=c["min_filter_reg"], alpha_eps=c["alpha_eps"]).to(DEV).eval()


def _run(mod, w0, feat, bb, sw, num_iter, compute_losses=True):
    with torch.no_grad():
        w, its, losses = mod(T(w0)[None], T(feat), T(bb), sample_weight=None if sw is None else T(sw),
                             num_iter=num_iter, compute_losses=compute_losses)
    assert len(its) == num_iter + 1 and w is its[-1]
    return torch.stack([i[0] for i in its]), (torch.cat(losses) if losses else None)   # (1,)-shaped losses, dimp.py:583


@pytest.mark.parametrize("name", ["dimp_sd_small_w", "dimp_sd_small_now", "dimp_sd_mid"])
def test_dimp_sd_golden_small(name):
    g = load_golden(name)
    mod = _dimp_module()
    if "filter_reg" in g:     # run-time mutated attributes (dimp.py:589-602)
        mod.filter_reg.data[0] = float(g["filter_reg"])
        mod.min_filter_reg = float(g["min_filter_reg"])
        mod.alpha_eps = float(g["alpha_eps"])
    its, losses = _run(mod, g["w0"], g["feat"], g["bb"], g.get("sw"), int(g["num_iter"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses, g["losses"], atol=2e-5, rtol=1e-4)
    its2, l2 = _run(mod, g["w0"], g["feat"], g["bb"], g.get("sw"), int(g["num_iter"]), compute_losses=False)
    assert l2 is None and torch.equal(its, its2)                          # deterministic, loss flag is side-effect free


@pytest.mark.parametrize("name", ["dimp_sd_cfg2_n50", "dimp_sd_cfg2_n15"])
def test_dimp_sd_golden_baseline_size(name):
    """BASELINE.json configs[1]: DiMP-50, 512x18x18, K=4, 5 iterations, n=50 / n=15 memory samples."""
    from pytracking_amd import filter as F
    g = load_golden(name)
    w0, feat, bb, sw = synth.dimp_problem(int(g["seed"]), int(g["n"]))
    its, losses = _run(_dimp_module(), w0, feat, bb, sw, 5)
    close(its, g["iterates"], atol=1e-4)
    close(losses, g["losses"], atol=1e-4, rtol=1e-4)
    scores = F.apply_filter(T(feat), its[-1][None])[:, 0]
    close(scores, g["scores"], atol=1e-4)
    assert np.all(np.diff(losses.cpu().numpy()) < 0)                      # monotone decrease


def test_dimp_sd_wide_adjoint_plan_22x22():
    """Round 4: 22x22 maps with n = 50 samples run the adjoint as EIGHT position slices of 24 groups per wave
    (k_adj2<V, 9, 24>; the PrDiMP goldens cover V = PrDiMP).  The same plan for the DiMP residual (V = relu) and the plain
    adjoint, against the float64 oracle: 128 channels keep the oracle in seconds."""
    from pytracking_amd import filter as F
    cfg = dict(synth.DIMP50, C=128, H=22, W=22)
    w0, feat, bb, sw = synth.dimp_problem(8122, 50, cfg)
    its, losses = _run(_dimp_module(cfg), w0, feat, bb, sw, 2)
    f64 = lambda a: np.asarray(a, np.float64)
    want, wl = O.dimp_sd(f64(w0), f64(feat), f64(bb), f64(sw), num_iter=2, step_length=cfg["init_step_length"],
                         filter_reg=cfg["init_filter_reg"], min_filter_reg=cfg["min_filter_reg"], feat_stride=cfg["feat_stride"],
                         label_w=synth.gauss_lut(cfg["num_dist_bins"], cfg["bin_displacement"], cfg["init_gauss_sigma"]),
                         mask_w=synth.mask_lut(cfg["num_dist_bins"], cfg["bin_displacement"], cfg["mask_init_factor"]),
                         spatial_w=np.ones(cfg["num_dist_bins"], np.float32), bin_displacement=cfg["bin_displacement"],
                         alpha_eps=cfg["alpha_eps"])
    close(its, want, atol=2e-5)
    close(losses, np.array(wl), atol=2e-5, rtol=1e-4)
    rng = np.random.default_rng(8123)
    r = rng.standard_normal((50, 23, 23)).astype(np.float32)
    adj = F.apply_feat_transpose(T(feat), T(r)[:, None], (4, 4), training=False)
    close(adj[0], O.apply_feat_transpose(f64(feat), f64(r), 4), atol=1e-4)


def test_dimp_more_bins_than_the_init_stage_stages_vs_oracle():
    """Look-up tables of more than 4096 bins (3 x 4100 x 4 bytes > 48 KB) do not fit the LDS of the fast route's init stage: the
    solve AND the frame take the generic route end to end (pt_sd_route_fast) -- on a shape (C = 128, 18x18) that otherwise runs
    the fast route.  Against the float64 oracle at the neighbouring tests' tolerances; the 4100-bin tables are finer than the
    100-bin ones of every other test (iterates differ by 7e-4 between the two), so a solve that ignored them would not pass."""
    from pytracking_amd import bench_frame
    from oracle import frame_port
    cfg = dict(synth.DIMP50, C=128, H=18, W=18, num_dist_bins=4100, bin_displacement=0.005)
    w0, feat, bb, sw = synth.dimp_problem(4100, 7, cfg)
    its, losses = _run(_dimp_module(cfg), w0, feat, bb, sw, 4)
    f64 = lambda a: np.asarray(a, np.float64)
    want, wl = O.dimp_sd(f64(w0), f64(feat), f64(bb), f64(sw), num_iter=4, step_length=cfg["init_step_length"],
                         filter_reg=cfg["init_filter_reg"], min_filter_reg=cfg["min_filter_reg"], feat_stride=cfg["feat_stride"],
                         label_w=synth.gauss_lut(cfg["num_dist_bins"], cfg["bin_displacement"], cfg["init_gauss_sigma"]),
                         mask_w=synth.mask_lut(cfg["num_dist_bins"], cfg["bin_displacement"], cfg["mask_init_factor"]),
                         spatial_w=np.ones(cfg["num_dist_bins"], np.float32), bin_displacement=cfg["bin_displacement"],
                         alpha_eps=cfg["alpha_eps"])
    assert np.isfinite(np.asarray(want)).all() and np.all(np.diff(wl) < 0)
    close(its, want, atol=2e-5)
    close(losses, np.array(wl), atol=2e-5, rtol=1e-4)
    # the frame (pt_track_frame_f32), as test_track_frame_matches_oracle_composition checks it
    st = bench_frame.TrackState(cfg, 6, seed=77, device=DEV)
    x = synth.clf_features(np.random.default_rng(78), 1, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    mem0, bb0, f0 = st.mem_feat.cpu().numpy().copy(), st.mem_bb.cpu().numpy().copy(), st.filter.cpu().numpy().copy()
    st.step(T(x)[0], slot=2, num_iter=3)
    torch.cuda.synchronize()
    ref = frame_port.oracle_step(cfg, mem0, bb0, st.sample_weight.cpu().numpy(), f0, x[0], slot=2, num_iter=3)
    close(st.scores, ref["scores"], atol=2e-5)
    assert tuple(st.peak.cpu().numpy().astype(int)) == tuple(ref["peak"])
    close(st.mem_bb, ref["bb"], atol=1e-4)
    close(st.filter, ref["filter"], atol=2e-5)


def test_dimp_l2_golden():
    from pytracking_amd import optimizer
    g = load_golden("dimp_l2_small")
    mod = optimizer.DiMPL2SteepestDescentGN(num_iter=3, feat_stride=16, init_step_length=float(g["step_length"]),
                                            gauss_sigma=float(g["gauss_sigma"]),
                                            hinge_threshold=float(g["hinge_threshold"]),
                                            init_filter_reg=float(g["filter_reg"]),
                                            min_filter_reg=float(g["min_filter_reg"])).to(DEV).eval()
    its, losses = _run(mod, g["w0"], g["feat"], g["bb"], g["sw"], int(g["num_iter"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses, g["losses"], atol=2e-5, rtol=1e-4)


def _prdimp_module(cfg=synth.PRDIMP50, **over):
    from pytracking_amd import optimizer
    c = dict(cfg, **over)
    return optimizer.PrDiMPSteepestDescentNewton(
        num_iter=c["num_iter"], feat_stride=c["feat_stride"], init_step_length=c["init_step_length"],
        init_filter_reg=c["init_filter_reg"], gauss_sigma=c["gauss_sigma"], min_filter_reg=c["min_filter_reg"],
        alpha_eps=c["alpha_eps"], init_uni_weight=c["init_uni_weight"], normalize_label=c["normalize_label"],
        label_shrink=c["label_shrink"], softmax_reg=c["softmax_reg"], label_threshold=c["label_threshold"]).to(DEV).eval()


def test_prdimp_golden_small_and_options():
    g = load_golden("prdimp_sd_small")
    its, losses = _run(_prdimp_module(), g["w0"], g["feat"], g["bb"], g["sw"], int(g["num_iter"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses, g["losses"], atol=2e-5, rtol=1e-4)
    g = load_golden("prdimp_sd_opts")
    mod = _prdimp_module(softmax_reg=float(g["softmax_reg"]), init_uni_weight=float(g["uni_weight"]),
                         label_shrink=float(g["label_shrink"]), label_threshold=float(g["label_threshold"]))
    its, losses = _run(mod, g["w0"], g["feat"], g["bb"], None, int(g["num_iter"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses, g["losses"], atol=2e-5, rtol=1e-4)


def test_prdimp_golden_baseline_size():
    """BASELINE.json configs[2] shape: PrDiMP-50, 512x22x22, n=50, 5 iterations."""
    g = load_golden("prdimp_sd_cfg3_n50")
    w0, feat, bb, sw = synth.dimp_problem(int(g["seed"]), int(g["n"]), synth.PRDIMP50)
    its, losses = _run(_prdimp_module(), w0 * 0, feat, bb, sw, 5)
    close(its, g["iterates"], atol=1e-4)
    close(losses, g["losses"], atol=1e-4, rtol=1e-4)


def test_sd_zero_iterations_and_single_sample():
    mod = _dimp_module()
    w0, feat, bb, sw = synth.dimp_problem(3, 1, small=dict(C=16, H=10, W=10))
    its, losses = _run(mod, w0, feat, bb, sw, 0)
    assert its.shape[0] == 1 and losses.shape[0] == 1
    ref_its, ref_l = O.dimp_sd(w0.astype(np.float64), feat.astype(np.float64), bb.astype(np.float64),
                               sw.astype(np.float64), num_iter=2, step_length=0.9, filter_reg=0.1, min_filter_reg=1e-3,
                               feat_stride=16, label_w=synth.gauss_lut(100, 0.1, 0.9), mask_w=synth.mask_lut(100, 0.1, 3.0),
                               spatial_w=np.ones(100, np.float32), bin_displacement=0.1)
    close(losses[0], ref_l[0], atol=1e-5, rtol=1e-4)
    its, losses = _run(mod, w0, feat, bb, sw, 2)
    close(its, ref_its, atol=2e-5)


@pytest.mark.parametrize("n,C,H,W", [(7, 128, 18, 18), (3, 256, 22, 22), (20, 128, 16, 16), (2, 128, 10, 8)])
def test_sd_fast_path_shapes_vs_oracle(n, C, H, W):
    """XCD-aligned solver path (C in {128,256,512,1024}, H*W % 4 == 0) against the float64 oracle: DiMP, DiMP-L2, PrDiMP."""
    from pytracking_amd import optimizer
    w0, feat, bb, sw = synth.dimp_problem(100 + n, n, small=dict(C=C, H=H, W=W))
    f64 = lambda a: None if a is None else a.astype(np.float64)
    for weights in (sw, None):
        ref_its, ref_l = O.dimp_sd(f64(w0), f64(feat), f64(bb), f64(weights), num_iter=4, step_length=0.9, filter_reg=0.1,
                                   min_filter_reg=1e-3, feat_stride=16, label_w=synth.gauss_lut(100, 0.1, 0.9),
                                   mask_w=synth.mask_lut(100, 0.1, 3.0), spatial_w=np.ones(100, np.float32),
                                   bin_displacement=0.1)
        its, losses = _run(_dimp_module(), w0, feat, bb, weights, 4)
        close(its, ref_its, atol=2e-5)
        close(losses, np.array(ref_l), atol=2e-5, rtol=1e-4)
    its0, l0 = _run(_dimp_module(), w0, feat, bb, sw, 0)
    close(l0[0], ref_l[0] if False else O.dimp_sd(f64(w0), f64(feat), f64(bb), f64(sw), num_iter=0, step_length=0.9,
          filter_reg=0.1, min_filter_reg=1e-3, feat_stride=16, label_w=synth.gauss_lut(100, 0.1, 0.9),
          mask_w=synth.mask_lut(100, 0.1, 3.0), spatial_w=np.ones(100, np.float32), bin_displacement=0.1)[1][0],
          atol=2e-5, rtol=1e-4)
    ref_its, ref_l = O.prdimp_sd(f64(w0) * 0, f64(feat), f64(bb), f64(sw), num_iter=4, step_length=1.0, filter_reg=0.05,
                                 min_filter_reg=0.05, feat_stride=16, gauss_sigma=0.9, alpha_eps=0.05,
                                 normalize_label=True, softmax_reg_val=0.1)
    its, losses = _run(_prdimp_module(softmax_reg=0.1), w0 * 0, feat, bb, sw, 4)
    close(its, ref_its, atol=2e-5)
    close(losses, np.array(ref_l), atol=2e-5, rtol=1e-4)
    ref_its, ref_l = O.dimp_l2_sd(f64(w0), f64(feat), f64(bb), f64(sw), num_iter=3, step_length=1.0, filter_reg=0.1,
                                  min_filter_reg=1e-3, feat_stride=16, gauss_sigma=1.0, hinge_threshold=0.05)
    mod = optimizer.DiMPL2SteepestDescentGN(num_iter=3, feat_stride=16, init_step_length=1.0, gauss_sigma=1.0,
                                            hinge_threshold=0.05, init_filter_reg=0.1, min_filter_reg=1e-3).to(DEV).eval()
    its, losses = _run(mod, w0, feat, bb, sw, 3)
    close(its, ref_its, atol=2e-5)
    close(losses, np.array(ref_l), atol=2e-5, rtol=1e-4)


# ------------------------------------------------------------------------------------------------------
# multi-filter filter layer + LWL few-shot learner
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F,C,H,W,K", [(3, 16, 64, 30, 52, 3), (2, 16, 512, 30, 52, 3), (5, 7, 40, 9, 11, 3),
                                         (2, 16, 32, 30, 52, 1), (4, 3, 20, 17, 120, 3), (1, 1, 16, 5, 5, 3),
                                         # two samples per adjoint workgroup, short last band, few filters
                                         (35, 5, 48, 9, 16, 3),
                                         # 1x1: re-rowed float4 path with a ragged channel count / odd map (banded kernel)
                                         (2, 16, 24, 18, 18, 1), (3, 9, 33, 7, 9, 1),
                                         # several full bands per sample; one-row bands (3 staged rows of 168 floats: the widest map a 3x3 pass stages)
                                         (2, 16, 16, 64, 64, 3), (1, 16, 20, 3, 168, 3),
                                         # even width that is not a multiple of 4 (480x854 frames: 30x54 maps): float2 staging
                                         (2, 16, 32, 30, 54, 3), (3, 6, 24, 18, 18, 3)])
def test_multifilter_ops_vs_oracle(n, F, C, H, W, K):
    from pytracking_amd import filter as FL
    rng = np.random.default_rng(7 * n + C)
    feat = synth.clf_features(rng, n, C, H, W, K)
    filt = rng.standard_normal((F, C, K, K), dtype=np.float32) * 0.05
    s = FL.apply_filter(T(feat)[:, None], T(filt)[None])[:, 0]
    ref = O.apply_filter(feat.astype(np.float64), filt.astype(np.float64))
    assert s.shape == ref.shape
    close(s, ref, atol=2e-5)
    inp = rng.standard_normal(ref.shape).astype(np.float32)
    adj = FL.apply_feat_transpose(T(feat)[:, None], T(inp)[:, None], K)[0]
    refa = O.apply_feat_transpose(feat.astype(np.float64), inp.astype(np.float64), K)
    close(adj, refa, atol=2e-5 * max(1.0, np.abs(refa).max()))
    lhs = float((s.double().cpu() * torch.from_numpy(inp).double()).sum())          # <F w, r> == <w, F^T r>
    rhs = float((adj.double().cpu() * torch.from_numpy(filt).double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs))


def _lwl_run(g_w0, feat, label, sw, num_iter, reg, slreg):
    from pytracking_amd.steepestdescent import GNSteepestDescent, LWTLResidual
    res = LWTLResidual(init_filter_reg=reg).to(DEV)
    opt = GNSteepestDescent(residual_module=res, num_iter=num_iter, compute_losses=True, steplength_reg=slreg,
                            residual_batch_dim=1)
    swt = None if sw is None else (T(sw)[:, None] if sw.ndim == 4 else T(sw))
    with torch.no_grad():
        w, its, losses = opt([T(g_w0)[None]], feat=T(feat)[:, None], label=T(label)[:, None], sample_weight=swt)
    assert len(its) == num_iter + 1 and w[0] is its[-1][0]
    return torch.stack([i[0][0] for i in its]), torch.stack(losses)


@pytest.mark.parametrize("name", ["lwl_gn_small_full", "lwl_gn_small_img", "lwl_gn_small_none", "lwl_gn_mid"])
def test_lwl_gn_golden(name):
    g = load_golden(name)
    sw = g["sw"] if g["sw"].size else None
    its, losses = _lwl_run(g["w0"], g["feat"], g["label"], sw, int(g["num_iter"]), float(g["filter_reg"]),
                           float(g["steplength_reg"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses, g["losses"], atol=1e-7, rtol=1e-4)


def test_lwl_edge_cases():
    """zero iterations (loss only), one filter, one sample, unsupported filter counts raise."""
    from pytracking_amd import filter as FL
    rng = np.random.default_rng(91)
    feat = synth.clf_features(rng, 1, 24, 6, 8, 3)
    label = rng.uniform(0, 1, (1, 1, 6, 8)).astype(np.float32)
    w0 = rng.standard_normal((1, 24, 3, 3), dtype=np.float32) * 0.05
    f64 = lambda a: a.astype(np.float64)
    its, losses = _lwl_run(w0, feat, label, None, 0, 0.1, 0.0)
    assert its.shape[0] == 1 and losses.shape[0] == 1
    ref_its, ref_l = O.lwl_gn_sd(f64(w0), f64(feat), f64(label), None, num_iter=2, filter_reg=0.1)
    close(losses[0], ref_l[0], atol=1e-7, rtol=1e-4)
    its, losses = _lwl_run(w0, feat, label, None, 2, 0.1, 0.0)
    close(its, ref_its, atol=2e-5)
    with pytest.raises(RuntimeError, match="not covered"):
        FL.apply_filter(T(feat)[:, None], T(np.zeros((1, 17, 24, 3, 3), np.float32)))   # 17 filters


def test_lwl_gn_config5_geometry_vs_oracle():
    """BASELINE configs[4] geometry (16 filters, 3x3, 30x52 maps) at reduced n and C; 3 iterations."""
    rng = np.random.default_rng(55)
    n, F, C, H, W, K = 3, 16, 128, 30, 52, 3
    feat = synth.clf_features(rng, n, C, H, W, K)
    label = rng.uniform(0, 1, (n, F, H, W)).astype(np.float32)
    sw = rng.uniform(0.2, 1.0, (n, F, H, W)).astype(np.float32)
    w0 = np.zeros((F, C, K, K), np.float32)
    its, losses = _lwl_run(w0, feat, label, sw, 3, 0.05, 0.0)
    f64 = lambda a: a.astype(np.float64)
    ref_its, ref_l = O.lwl_gn_sd(f64(w0), f64(feat), f64(label), f64(sw), num_iter=3, filter_reg=0.05)
    close(its, ref_its, atol=2e-5)
    close(losses, np.array(ref_l), atol=1e-7, rtol=1e-4)
    assert np.all(np.diff(losses.cpu().numpy()) < 0)


# ------------------------------------------------------------------------------------------------------
# ATOM conjugate gradient
# ------------------------------------------------------------------------------------------------------
def _atom_run(x0, samples, y, sw, iters, fr, calls):
    from pytracking_amd.optimization import ConjugateGradient, ConvProblem, MLU
    x = [T(x0.copy())[None].clone()]
    prob = ConvProblem([T(samples)], [T(y)[:, None]], [synth.ATOM18["filter_reg"]], [T(sw)],
                       MLU(synth.ATOM18["act_min_val"]))
    opt = ConjugateGradient(prob, x, fletcher_reeves=fr, direction_forget_factor=0)
    outs = []
    for _ in range(calls):
        opt.run(iters)
        outs.append(x[0][0].clone())
    return torch.stack(outs)


@pytest.mark.parametrize("name", ["atom_cg_small_pr", "atom_cg_small_fr"])
def test_atom_cg_golden_small(name):
    g = load_golden(name)
    out = _atom_run(g["x0"], g["samples"], g["y"], g["sw"], int(g["num_iter"]), bool(g["fletcher_reeves"]),
                    g["x_out"].shape[0])
    close(out, g["x_out"], atol=5e-6)                    # measured on gfx950: 1.3e-7 (round 5, |x| <= 0.29)


def test_atom_cg_golden_config1_size():
    """BASELINE.json configs[0] solver shape: ATOM, 250 x 64 x 18 x 18 memory, PR-CG 5 iterations."""
    g = load_golden("atom_cg_cfg1_n250")
    x0, samples, y, sw = synth.atom_problem(int(g["seed"]), int(g["n"]))
    out = _atom_run(x0, samples, y, sw, 5, False, 1)
    close(out, g["x_out"], atol=5e-6)                    # measured on gfx950: 2.3e-7 (round 5, |x| <= 0.065); was 1e-4 + rtol 1e-3


def _atom_gn_run(f0, P0, samples, y, sw, cg_iters, fr, filter_reg, projection_reg, act_min_val):
    import torch.nn.functional as F
    from pytracking_amd.optimization import FactorizedConvProblem, GaussNewtonCG
    # the activations arrive exactly as the reference tracker builds them (atom.py:444-466): plain lambdas
    prob = FactorizedConvProblem([T(samples)], [T(y)[:, None]], [filter_reg], [projection_reg], None, [T(sw)],
                                 lambda x: x, lambda x: F.elu(F.leaky_relu(x, 1 / act_min_val), act_min_val))
    filt = T(f0.copy())[None].clone()
    proj = T(P0.copy())[:, :, None, None].clone()
    opt = GaussNewtonCG(prob, [filt, proj], fletcher_reeves=fr)
    opt.run(list(cg_iters))
    return filt[0], proj[:, :, 0, 0]


@pytest.mark.parametrize("name", ["atom_gn_small_fr", "atom_gn_small_pr", "atom_gn_mid"])
def test_atom_joint_gn_golden(name):
    """ATOM first-frame GaussNewtonCG over (filter, projection matrix): optimization.py:328-421, atom/optim.py:6-68."""
    g = load_golden(name)
    f, P = _atom_gn_run(g["f0"], g["P0"], g["samples"], g["y"], g["sw"], [int(v) for v in g["cg_iters"]],
                        bool(int(g["fletcher_reeves"])), float(g["filter_reg"]), float(g["projection_reg"]),
                        float(g["act_min_val"]))
    close(f, g["f_out"], atol=5e-6)                      # measured on gfx950: 3e-8 (filter), 9.5e-7 (projection, |P| <= 3.1); no rtol
    close(P, g["P_out"], atol=1e-5)


def test_atom_joint_gn_first_frame_size_vs_oracle():
    """ATOM default first frame (parameter/atom/default.py): 30 augmented samples of 256 x 18 x 18 backbone features,
    64 compressed channels, 4 x 4 filter, init_CG_iter 60 / init_GN_iter 6 -> 6 x 10 CG iterations (shortened to
    3 x 4 so the float64 oracle finishes in seconds)."""
    rng = np.random.default_rng(77)
    n, M, Kc, H, W, K = 30, 256, 64, 18, 18, 4
    samples = rng.standard_normal((n, M, H, W), dtype=np.float32) * np.float32(0.1)
    _, _, y, sw = synth.atom_problem(77, n)
    f0 = np.zeros((Kc, K, K), np.float32)                               # filter_init_method 'zeros' (atom.py:140-143)
    P0 = rng.standard_normal((Kc, M), dtype=np.float32) * np.float32(1.0 / np.sqrt(M))
    cfg = synth.ATOM18
    f, P = _atom_gn_run(f0, P0, samples, y, sw, [4, 4, 4], True, cfg["filter_reg"], 1e-4, cfg["act_min_val"])
    f64 = lambda a: a.astype(np.float64)
    rf, rP = O.atom_gn_cg(f64(f0), f64(P0), f64(samples), f64(y), f64(sw), filter_reg=cfg["filter_reg"],
                          projection_reg=1e-4, act_min_val=cfg["act_min_val"], cg_iters=[4, 4, 4], fletcher_reeves=True)
    close(f, rf, atol=1e-4, rtol=2e-3)
    close(P, rP, atol=1e-4, rtol=2e-3)
    assert float(np.abs(rf).max()) > 1e-3                               # the solve moved the filter off zero


# ------------------------------------------------------------------------------------------------------
# Precise RoI pooling (oracle self-pinned; see oracle/prroi_torch.py)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW,scale,H,W", [(4, 4, 1 / 16, 18, 18), (5, 5, 1 / 8, 36, 36), (3, 3, 1 / 16, 18, 18),
                                             (1, 1, 1 / 16, 18, 18), (2, 3, 0.5, 7, 9)])
def test_prroi_forward_backward_vs_oracle(PH, PW, scale, H, W):
    from pytracking_amd.prroi_pool import PrRoIPool2D
    rng = np.random.default_rng(PH * 10 + PW)
    N, C, R = 2, 24, 11
    feat = rng.standard_normal((N, C, H, W), dtype=np.float32)
    ext = np.array([W, H], dtype=np.float64) / scale
    xy0 = rng.uniform(-0.1, 0.6, (R, 2)) * ext
    wh = rng.uniform(0.05, 0.6, (R, 2)) * ext
    rois = np.concatenate((rng.integers(0, N, (R, 1)).astype(np.float64), xy0, xy0 + wh), 1).astype(np.float32)
    rois[-1, 3] = rois[-1, 1]                                   # zero-area RoI -> zeros, zero gradients
    rois[-2, 1:] = [4 * ext[0], 4 * ext[1], 5 * ext[0], 5 * ext[1]]   # fully outside the map
    f = T(feat).requires_grad_(True)
    r = T(rois).requires_grad_(True)
    out = PrRoIPool2D(PH, PW, scale)(f, r)
    ref = O.prroi_forward(feat.astype(np.float64), rois.astype(np.float64), PH, PW, scale)
    close(out, ref, atol=2e-5)
    gout = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(T(gout))
    close(f.grad, O.prroi_backward_feat(gout.astype(np.float64), feat.shape, rois.astype(np.float64), PH, PW, scale),
          atol=1e-4)
    refc = O.prroi_backward_coor(gout.astype(np.float64), feat.astype(np.float64), rois.astype(np.float64), PH, PW, scale)
    close(r.grad, refc, atol=2e-4 * max(1.0, np.abs(refc).max()))
    assert float(r.grad[:, 0].abs().max()) == 0.0
    g1 = f.grad.clone()                                          # the feature gradient is a fixed-order gather: bit-reproducible
    f.grad = None
    r.grad = None
    PrRoIPool2D(PH, PW, scale)(f, r).backward(T(gout))
    assert torch.equal(f.grad, g1)


@pytest.mark.parametrize("PH,PW,scale,H,W", [(5, 5, 1 / 8, 36, 36), (3, 3, 1 / 16, 18, 18), (4, 4, 1 / 16, 18, 18)])
def test_prroi_rois_at_negative_coordinates(PH, PW, scale, H, W):
    """RoIs that drift above / left of the search crop (IoU refinement, jittered proposals): bins more than one pixel
    outside the map touch no pixel (j1 < 0 or i1 < 0) -- outputs and gradients must be the oracle's finite values
    (zeros where nothing is touched), not reads in front of the tensor."""
    from pytracking_amd.prroi_pool import PrRoIPool2D
    rng = np.random.default_rng(77 + PH)
    N, C = 1, 16
    # b = 0, c = 0 is the tensor base: a negative index there reads in front of the allocation
    feat = rng.standard_normal((N, C, H, W), dtype=np.float32)
    ex, ey = W / scale, H / scale
    rois = np.array([
        [0, -0.9 * ex, -0.9 * ey, -0.2 * ex, -0.2 * ey],       # fully above-left, far outside
        [0, -0.6 * ex, 0.1 * ey, 0.3 * ex, 0.5 * ey],          # left part outside: the first bins' i1 < 0
        [0, 0.2 * ex, -0.7 * ey, 0.6 * ex, 0.2 * ey],          # top part outside: the first bins' j1 < 0
        [0, -0.4 * ex, -0.4 * ey, 1.3 * ex, 1.3 * ey],         # covers the map and sticks out on every side (wide bins)
        [0, -3.0 / scale, -3.0 / scale, 2.0 / scale, 2.0 / scale],   # a few pixels over the corner
        [0, 0.9 * ex, 0.9 * ey, 1.8 * ex, 1.8 * ey],           # bottom-right overhang
    ], dtype=np.float32)
    f = T(feat).requires_grad_(True)
    r = T(rois).requires_grad_(True)
    out = PrRoIPool2D(PH, PW, scale)(f, r)
    ref = O.prroi_forward(feat.astype(np.float64), rois.astype(np.float64), PH, PW, scale)
    assert torch.isfinite(out).all()
    close(out, ref, atol=2e-5)
    assert float(out[0].abs().max()) == 0.0
    gout = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(T(gout))
    assert torch.isfinite(f.grad).all() and torch.isfinite(r.grad).all()
    close(f.grad, O.prroi_backward_feat(gout.astype(np.float64), feat.shape, rois.astype(np.float64), PH, PW, scale),
          atol=1e-4)
    refc = O.prroi_backward_coor(gout.astype(np.float64), feat.astype(np.float64), rois.astype(np.float64), PH, PW, scale)
    close(r.grad, refc, atol=2e-4 * max(1.0, np.abs(refc).max()))
    assert float(r.grad[0].abs().max()) == 0.0


def test_prroi_consumers_golden():
    """Reference FilterInitializerLinear pooling and the IoU-predictor proposal gradient (golden produced by the
    reference modules with the PrRoIPool restatement plugged in)."""
    from pytracking_amd.prroi_pool import PrRoIPool2D
    g = load_golden("filter_init_linear")
    bb = g["bb"]
    n = bb.shape[0]
    rois = np.concatenate((np.arange(n, dtype=np.float32)[:, None], bb[:, :2], bb[:, :2] + bb[:, 2:]), 1)
    pooled = PrRoIPool2D(4, 4, 1 / 16)(T(g["conv_out"]), T(rois))
    close(pooled.mean(0), g["weights"][0], atol=2e-5)
    g = load_golden("iou_predict")
    sd = {k[3:].replace("__", "."): T(v) for k, v in g.items() if k.startswith("sd_")}
    c3 = T(g["c3"]) * T(g["mod3"]).reshape(1, -1, 1, 1)
    c4 = T(g["c4"]) * T(g["mod4"]).reshape(1, -1, 1, 1)
    props = T(g["proposals"]).requires_grad_(True)
    xyxy = torch.cat((props[0, :, :2], props[0, :, :2] + props[0, :, 2:]), 1)
    roi = torch.cat((torch.zeros(xyxy.shape[0], 1, device=DEV), xyxy), 1)
    r3 = PrRoIPool2D(5, 5, 1 / 8)(c3, roi)
    r4 = PrRoIPool2D(3, 3, 1 / 16)(c4, roi)

    def block(x, pre):
        z = torch.nn.functional.linear(x.reshape(x.shape[0], -1), sd[pre + ".linear.weight"], sd[pre + ".linear.bias"])
        z = (z - sd[pre + ".bn.running_mean"]) / torch.sqrt(sd[pre + ".bn.running_var"] + 1e-5)
        return torch.relu(z * sd[pre + ".bn.weight"] + sd[pre + ".bn.bias"])
    iou = torch.nn.functional.linear(torch.cat((block(r3, "fc3_rt"), block(r4, "fc4_rt")), 1),
                                     sd["iou_predictor.weight"], sd["iou_predictor.bias"]).reshape(1, -1)
    close(iou, g["iou"], atol=5e-5)
    iou.backward(gradient=torch.ones_like(iou))                            # dimp.py:737-745
    close(props.grad, g["grad"], atol=5e-5, rtol=1e-3)


# ------------------------------------------------------------------------------------------------------
# benchmark frame (C ABI pt_track_frame_f32) against a composition of the oracle pieces
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,n", [(32, 6), (128, 6), (512, 9)])
def test_track_frame_matches_oracle_composition(C, n):
    from pytracking_amd import bench_frame
    from oracle import frame_port
    cfg = dict(synth.DIMP50, C=C, H=18, W=18)
    st = bench_frame.TrackState(cfg, n, seed=77, device=DEV)
    rng = np.random.default_rng(78)
    x = synth.clf_features(rng, 1, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    mem0, bb0, w0 = st.mem_feat.cpu().numpy().copy(), st.mem_bb.cpu().numpy().copy(), st.filter.cpu().numpy().copy()
    st.step(T(x)[0], slot=2, num_iter=3)
    torch.cuda.synchronize()
    ref = frame_port.oracle_step(cfg, mem0, bb0, st.sample_weight.cpu().numpy(), w0, x[0], slot=2, num_iter=3)
    close(st.scores, ref["scores"], atol=2e-5)
    assert tuple(st.peak.cpu().numpy().astype(int)) == tuple(ref["peak"])
    close(st.mem_bb, ref["bb"], atol=1e-4)
    close(st.filter, ref["filter"], atol=2e-5)


def test_bench_trajectory_closed_loop_60_frames():
    """The benchmark's own trajectory (bench.py: n = 50, C = 512, 5 iterations, graph-replayed) checked closed-loop: 60
    consecutive `pt_track_frame_f32` frames -- each classifies with the filter the previous frame produced, re-centres
    a box on its own arg-max and overwrites a memory slot -- against the float64 CPU restatement of the reference's op
    sequence stepping through the same inputs on its own state (oracle/frame_port.TorchCpuTracker, pinned against the
    reference goldens in tests/test_oracle_golden.py).  Classification scores, filter, peak and boxes within 1e-4 at
    EVERY frame; then the same 60 frames as three replays of one 20-frame hipGraph (the launch mode of
    `bench.py --steps 20 --warmup 5`) must reproduce the eager states bit for bit."""
    import os
    from pytracking_amd import bench_frame
    from oracle.frame_port import TorchCpuTracker
    cfg, n, G, start = synth.DIMP50, 50, 20, 5
    st = bench_frame.TrackState(cfg, n, seed=1234, device=DEV)
    ref = TorchCpuTracker(cfg, n, seed=1234, threads=min(16, os.cpu_count() or 1), dtype=torch.float64, gemm=True)
    pool_np = synth.clf_features(np.random.default_rng(4321), 50, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    pool, pool64 = T(pool_np), torch.from_numpy(pool_np).double()
    f0, m0, b0 = st.filter.clone(), st.mem_feat.clone(), st.mem_bb.clone()
    snaps, worst = {}, dict(scores=0.0, filter=0.0, bb=0.0)
    for f in range(60):
        k = start + f % G                                               # memory slot = pool entry, as bench.run_frames
        st.step(pool[k], slot=k, num_iter=5)
        s_ref = ref.step(pool64[k], k, 5)
        e_s = float((st.scores.double().cpu() - s_ref).abs().max())
        e_w = float((st.filter.double().cpu() - ref.filter[0]).abs().max())
        e_b = float((st.mem_bb.double().cpu() - ref.mem_bb).abs().max())
        flat = int(torch.argmax(s_ref))
        assert tuple(st.peak.cpu().numpy().astype(int)) == divmod(flat, s_ref.shape[1]), f
        assert e_s <= 1e-4 and e_w <= 1e-4 and e_b <= 1e-4, (f, e_s, e_w, e_b)
        worst = dict(scores=max(worst["scores"], e_s), filter=max(worst["filter"], e_w), bb=max(worst["bb"], e_b))
        if (f + 1) % G == 0:
            snaps[f + 1] = (st.filter.clone(), st.scores.clone(), st.mem_bb.clone(), st.mem_feat[start:start + G].clone())
    assert float((st.filter - f0).abs().max()) > 1e-3                  # the trajectory moved
    # the graph-replayed launch mode of the benchmark, from the same start state
    st.filter.copy_(f0); st.mem_feat.copy_(m0); st.mem_bb.copy_(b0)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for f in range(G):
                st.step(pool[start + f], slot=start + f, num_iter=5)
        for rep in (1, 2, 3):
            g.replay()
            stream.synchronize()
            w, s, b, m = snaps[rep * G]
            assert torch.equal(st.filter, w) and torch.equal(st.scores, s) and torch.equal(st.mem_bb, b), rep
            assert torch.equal(st.mem_feat[start:start + G], m)
    torch.cuda.current_stream().wait_stream(stream)
    print("closed-loop worst errors over 60 frames:", worst)


@pytest.mark.parametrize("kind,n,C", [("dimp", 50, 512), ("dimp", 16, 128), ("prdimp", 50, 512), ("dimp", 70, 256)])
def test_frame_chain_deferred_last_update_is_bit_identical(kind, n, C):
    """Frame chains (pt_track_frame_chain_f32, round 6): the solve's last filter update rides on the NEXT frame's first correlation
    instead of being its own dependent launch.  Two identical sequences, one through pt_track_frame_f32, one through the chain with
    every update deferred: classification scores, peak, re-centred boxes and memory BIT-EQUAL at every frame (the deferred update is
    evaluated by the same expressions on the same operands), the filter bit-equal whenever the chain is flushed -- with frames of 5,
    2, 1 (never deferred) and 0 iterations (classification-only frames consume a pending update as well) in the schedule; then the
    chain captured into a hipGraph (the launch mode of bench.py) and replayed."""
    from pytracking_amd import bench_frame
    cfg = dict(synth.DIMP50 if kind == "dimp" else synth.PRDIMP50, C=C)
    a = bench_frame.TrackState(cfg, n, seed=77, device=DEV, kind=kind)
    b = bench_frame.TrackState(cfg, n, seed=77, device=DEV, kind=kind)
    pool = T(synth.clf_features(np.random.default_rng(78), 24, C, cfg["H"], cfg["W"], cfg["K"]))
    sched = [5, 5, 2, 0, 5, 1, 5, 0, 0, 3, 5, 5]
    for f, nit in enumerate(sched):
        a.step(pool[f], slot=(3 * f) % n, num_iter=nit)
        b.step(pool[f], slot=(3 * f) % n, num_iter=nit, defer=True)
        assert b.pending.iters == (nit if nit >= 2 else 0), (f, nit, b.pending.iters)
        torch.cuda.synchronize()
        assert torch.equal(a.scores, b.scores) and torch.equal(a.peak, b.peak) and torch.equal(a.mem_bb, b.mem_bb), f
        assert torch.equal(a.mem_feat, b.mem_feat), f
        if f % 4 == 3 or nit < 2:
            b.flush()
            assert b.pending.iters == 0
            torch.cuda.synchronize()
            assert torch.equal(a.filter, b.filter), f
        elif nit >= 2:
            assert not torch.equal(a.filter, b.filter), f        # the update really is pending: `filter` still holds w_0 of the solve
    b.flush()
    torch.cuda.synchronize()
    assert torch.equal(a.filter, b.filter)
    # graph replay of a deferred chain: 6 frames + the flush captured once, replayed twice from the same start state
    f0, m0, b0 = a.filter.clone(), a.mem_feat.clone(), a.mem_bb.clone()
    for f in range(6):
        a.step(pool[12 + f], slot=f, num_iter=5)
    torch.cuda.synchronize()
    want = (a.filter.clone(), a.scores.clone(), a.mem_bb.clone())
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for f in range(6):
                b.step(pool[12 + f], slot=f, num_iter=5, defer=True)
            b.flush()
        for _ in range(2):
            b.filter.copy_(f0); b.mem_feat.copy_(m0); b.mem_bb.copy_(b0)
            g.replay()
            stream.synchronize()
            assert torch.equal(b.filter, want[0]) and torch.equal(b.scores, want[1]) and torch.equal(b.mem_bb, want[2])
    torch.cuda.current_stream().wait_stream(stream)


class _FuseInit:
    """PT_SD_FUSE_INIT=1 for the calls inside (opt-in experiment; the library reads the switch per solve)."""
    def __enter__(self):
        import os
        self.old = os.environ.get("PT_SD_FUSE_INIT")
        os.environ["PT_SD_FUSE_INIT"] = "1"

    def __exit__(self, *a):
        import os
        if self.old is None:
            os.environ.pop("PT_SD_FUSE_INIT", None)
        else:
            os.environ["PT_SD_FUSE_INIT"] = self.old


@pytest.mark.parametrize("variant", ["relu", "bentpar", "linmask", "l2", "relu_22x22", "relu_8x8_many", "relu_nosw", "relu_c512_n50"])
def test_fused_init_stage_is_bit_identical_solver(variant):
    """Round 6, experiment O (opt-in, PT_SD_FUSE_INIT=1: measured slower, profiles/r06o_fused_init_stage.txt): the first adjoint pass of a
    solve does the init stage itself (k_adj2<.., INIT>: slices -> s_0, maps, packed operands in registers) instead of a k_fast_init2
    launch in front of it.  Same expressions on the same operands: every iterate of the optimiser mirror BIT-EQUAL with the default path, for the relu / bentpar / L2 residuals, sigmoid and
    linear masks, 18x18 (E = 6) and 22x22 maps (E = 9, 24-group plan), slices holding more samples than the workgroup has waves
    (8x8 maps, n = 200), with and without sample weights -- and the fused iterates stay inside 2e-5 of the loss-returning call's
    (which never fuses: the loss read-out wants the raw maps)."""
    from pytracking_amd import optimizer
    cfg = dict(synth.DIMP50, C=128)
    n, nit = 15, 3
    if variant == "relu_22x22":
        cfg.update(H=22, W=22); n = 50; nit = 2
    elif variant == "relu_8x8_many":
        cfg.update(H=8, W=8); n = 200; nit = 2
    elif variant == "relu_c512_n50":
        cfg.update(C=512); n = 50; nit = 5
    w0, feat, bb, sw = synth.dimp_problem(6100 + len(variant), n, cfg)
    if variant == "relu_nosw":
        sw = None
    if variant == "l2":
        mod = optimizer.DiMPL2SteepestDescentGN(num_iter=nit, feat_stride=16, init_step_length=1.0, gauss_sigma=1.0, hinge_threshold=-999.0,
                                                init_filter_reg=0.1, min_filter_reg=1e-3).to(DEV).eval()
    else:
        over = {"bentpar": dict(score_act="bentpar"), "linmask": dict(mask_act="linear")}.get(variant, {})
        mod = _dimp_module(cfg, **over)
    with _FuseInit():
        fused, _ = _run(mod, w0, feat, bb, sw, nit, compute_losses=False)
    plain, _ = _run(mod, w0, feat, bb, sw, nit, compute_losses=False)
    assert torch.equal(fused, plain), float((fused - plain).abs().max())
    lossy, losses = _run(mod, w0, feat, bb, sw, nit, compute_losses=True)
    assert torch.equal(plain, lossy) and losses is not None
    assert float((fused[1:] - fused[:-1]).abs().max()) > 0                # the solve moved


@pytest.mark.parametrize("C,n", [(512, 50), (256, 16)])
def test_fused_init_stage_is_bit_identical_frames(C, n):
    """The same through the frame entry points (classification epilogue inside the init stage: scores of the inserted slot, first
    maximum, re-centred box): two identical sequences, one with PT_SD_FUSE_INIT=1; scores, peak, boxes, memory, filter AND the whole
    solver workspace (s_0 ... s_T, label / mask / weight maps, packed operands, gradient partials) bit-equal at every frame, plain
    frames and deferred chains, 5 / 2 / 1 / 0 iterations; then a graph-captured fused chain against the eager unfused one."""
    from pytracking_amd import bench_frame
    cfg = dict(synth.DIMP50, C=C)
    a = bench_frame.TrackState(cfg, n, seed=91, device=DEV, kind="dimp")
    b = bench_frame.TrackState(cfg, n, seed=91, device=DEV, kind="dimp")
    a.ws.zero_(); b.ws.zero_()
    pool = T(synth.clf_features(np.random.default_rng(92), 20, C, cfg["H"], cfg["W"], cfg["K"]))
    sched = [5, 5, 2, 0, 5, 1, 5, 3]
    for defer in (False, True):
        for f, nit in enumerate(sched):
            a.step(pool[f], slot=(5 * f) % n, num_iter=nit, defer=defer)
            with _FuseInit():
                b.step(pool[f], slot=(5 * f) % n, num_iter=nit, defer=defer)
            torch.cuda.synchronize()
            assert torch.equal(a.scores, b.scores) and torch.equal(a.peak, b.peak) and torch.equal(a.mem_bb, b.mem_bb), (defer, f)
            assert torch.equal(a.mem_feat, b.mem_feat) and torch.equal(a.filter, b.filter), (defer, f)
            assert torch.equal(a.ws, b.ws), (defer, f)
        if defer:
            a.flush(); b.flush()
            torch.cuda.synchronize()
            assert torch.equal(a.filter, b.filter)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), _FuseInit():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for f in range(4):
                b.step(pool[8 + f], slot=f, num_iter=5, defer=True)
            b.flush()
        g.replay()
        stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for f in range(4):
        a.step(pool[8 + f], slot=f, num_iter=5)
    torch.cuda.synchronize()
    assert torch.equal(a.filter, b.filter) and torch.equal(a.scores, b.scores) and torch.equal(a.mem_bb, b.mem_bb)


def test_frame_chain_argument_checks():
    import ctypes
    from pytracking_amd import _lib, bench_frame
    L = _lib.lib()
    pend = _lib.FramePending()
    assert L.pt_track_frame_flush_f32(None, None, 1, 1, 1, 1, 1, None, 0, None) == _lib.PT_ERR_NULL
    st = bench_frame.TrackState(dict(synth.DIMP50, C=128), 8, seed=1, device=DEV)
    assert L.pt_track_frame_flush_f32(ctypes.byref(pend), st.filter.data_ptr(), 8, 128, 18, 18, 4, st.ws.data_ptr(), st.ws.numel(), None) == 0
    pend.iters = -1
    x = T(synth.clf_features(np.random.default_rng(2), 1, 128, 18, 18, 4))[0]
    rc = L.pt_track_frame_chain_f32(ctypes.byref(st.params), st.filter.data_ptr(), st.mem_feat.data_ptr(), st.mem_bb.data_ptr(),
                                    st.sample_weight.data_ptr(), x.data_ptr(), 0, 8, 128, 18, 18, 4, 2, st.scores.data_ptr(),
                                    st.peak.data_ptr(), st.ws.data_ptr(), st.ws.numel(), ctypes.byref(pend), 1, None)
    assert rc == _lib.PT_ERR_SHAPE
    pend.iters = 1                                                 # a one-iteration solve is never pending
    rc = L.pt_track_frame_chain_f32(ctypes.byref(st.params), st.filter.data_ptr(), st.mem_feat.data_ptr(), st.mem_bb.data_ptr(),
                                    st.sample_weight.data_ptr(), x.data_ptr(), 0, 8, 128, 18, 18, 4, 2, st.scores.data_ptr(),
                                    st.peak.data_ptr(), st.ws.data_ptr(), st.ws.numel(), ctypes.byref(pend), 1, None)
    assert rc == _lib.PT_ERR_SHAPE
    # a 3x3 filter is outside the chain's path: refused, and TrackState.step(defer=True) falls back to the plain frame
    st3 = bench_frame.TrackState(dict(synth.DIMP50, C=64, K=3), 8, seed=1, device=DEV)
    x3 = T(synth.clf_features(np.random.default_rng(2), 1, 64, 18, 18, 3))[0]
    st3.step(x3, slot=1, num_iter=2, defer=True)
    assert st3.pending.iters == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,C", [(34, 128), (64, 256), (35, 128), (40, 512)])
def test_apply_filter_sample_pair_workgroups(n, C):
    """Round 4: with more than 32 samples (even count) the XCD-aligned correlation runs two samples per workgroup
    (csrc/fast_passes.hip: pt_fast_plan, spw = 2); an odd count keeps one.  Scores of every sample against the float64
    oracle, and the adjoint of the same maps (unchanged kernel, same plan object) for good measure."""
    from pytracking_amd import filter as F
    rng = np.random.default_rng(4000 + n + C)
    feat = synth.clf_features(rng, n, C, 18, 18, 4)
    filt = (rng.standard_normal((C, 4, 4), dtype=np.float32) * np.float32(0.5 / np.sqrt(C * 16)))
    s = F.apply_filter(T(feat), T(filt[None]))
    want = O.apply_filter(feat.astype(np.float64), filt.astype(np.float64))
    assert s.shape == (n, 1) + want.shape[1:]
    close(s[:, 0], want, atol=2e-5)
    r = rng.standard_normal(want.shape).astype(np.float32)
    adj = F.apply_feat_transpose(T(feat), T(r)[:, None], (4, 4), training=False)
    close(adj[0], O.apply_feat_transpose(feat.astype(np.float64), r.astype(np.float64), 4), atol=1e-4)


@pytest.mark.parametrize("slot", [6, 7, 33])
def test_track_frame_pair_workgroup_slot_parity(slot):
    """The memory insert rides on the first correlation: the inserted sample may be the first or the second member of a
    sample pair (even / odd slot), or the last sample.  n = 34, C = 128 runs pairs; against the float64 oracle composition."""
    from pytracking_amd import bench_frame
    from oracle import frame_port
    cfg = dict(synth.DIMP50, C=128)
    n = 34
    st = bench_frame.TrackState(cfg, n, seed=91, device=DEV)
    rng = np.random.default_rng(92 + slot)
    x = synth.clf_features(rng, 1, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    mem0, bb0, w0 = st.mem_feat.cpu().numpy().copy(), st.mem_bb.cpu().numpy().copy(), st.filter.cpu().numpy().copy()
    st.step(T(x)[0], slot=slot, num_iter=3)
    torch.cuda.synchronize()
    ref = frame_port.oracle_step(cfg, mem0, bb0, st.sample_weight.cpu().numpy(), w0, x[0], slot=slot, num_iter=3)
    close(st.scores, ref["scores"], atol=2e-5)
    assert tuple(st.peak.cpu().numpy().astype(int)) == tuple(ref["peak"])
    close(st.mem_feat, ref["mem"], atol=0)
    close(st.mem_bb, ref["bb"], atol=1e-4)
    close(st.filter, ref["filter"], atol=2e-5)


@pytest.mark.parametrize("C,n", [(32, 5), (128, 6), (512, 7)])
def test_track_frame_prdimp_matches_oracle_composition(C, n):
    """`pt_track_frame_f32(PT_SD_PRDIMP)` -- classification read off the solve's first correlation, first arg-max, box
    re-centring, memory insert, softmax-Newton solve (optimizer.py:355-439; dimp.py:190-194,605-648) -- against the
    float64 composition of the oracle pieces, from a NON-zero filter (so the classification map is not trivially 0)
    and from the zero start filter of the benchmark state."""
    from pytracking_amd import bench_frame
    from oracle import frame_port
    cfg = dict(synth.PRDIMP50, C=C)
    for zero_start in (False, True):
        st = bench_frame.TrackState(cfg, n, seed=177, device=DEV, kind="prdimp")
        if not zero_start:
            w_np = synth.dimp_problem(177, n, cfg)[0]
            st.filter.copy_(T(w_np))
        rng = np.random.default_rng(178)
        x = synth.clf_features(rng, 1, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
        mem0, bb0, w0 = st.mem_feat.cpu().numpy().copy(), st.mem_bb.cpu().numpy().copy(), st.filter.cpu().numpy().copy()
        st.step(T(x)[0], slot=3, num_iter=3)
        torch.cuda.synchronize()
        ref = frame_port.oracle_step(cfg, mem0, bb0, st.sample_weight.cpu().numpy(), w0, x[0], slot=3, num_iter=3, kind="prdimp")
        close(st.scores, ref["scores"], atol=2e-5)
        assert tuple(st.peak.cpu().numpy().astype(int)) == tuple(ref["peak"])
        close(st.mem_bb, ref["bb"], atol=1e-4)
        close(st.mem_feat, ref["mem"], atol=0)
        close(st.filter, ref["filter"], atol=2e-5)


def test_bench_trajectory_prdimp_closed_loop_40_frames():
    """BENCH's `prdimp50_frame` workload / BASELINE configs[2]'s per-GPU workload on its exact call path: 40 consecutive
    `pt_track_frame_f32(PT_SD_PRDIMP)` frames at n = 50, C = 512, 22x22 features (23x23 score maps), 5 iterations, zero
    start filter -- each frame classifies with the filter the previous frame left, re-centres a box on its own arg-max and
    overwrites a memory slot -- against the float64 restatement of the reference's op sequence
    (oracle/frame_port.TorchCpuTracker(kind="prdimp"), pinned to the reference golden `prdimp_sd_cfg3_n50` in
    tests/test_oracle_golden.py::test_torch_port_prdimp_matches_reference).  Scores, filter and boxes within 1e-4 at EVERY
    frame, peaks equal; then the same frames as two replays of one 20-frame hipGraph bit-equal to the eager states."""
    import os
    from pytracking_amd import bench_frame
    from oracle.frame_port import TorchCpuTracker
    cfg, n, G, start, frames = synth.PRDIMP50, 50, 20, 5, 40
    st = bench_frame.TrackState(cfg, n, seed=2234, device=DEV, kind="prdimp")
    ref = TorchCpuTracker(cfg, n, seed=2234, threads=min(16, os.cpu_count() or 1), dtype=torch.float64, gemm=True, kind="prdimp")
    pool_np = synth.clf_features(np.random.default_rng(4322), 50, cfg["C"], cfg["H"], cfg["W"], cfg["K"])
    pool, pool64 = T(pool_np), torch.from_numpy(pool_np).double()
    f0, m0, b0 = st.filter.clone(), st.mem_feat.clone(), st.mem_bb.clone()
    snaps, worst = {}, dict(scores=0.0, filter=0.0, bb=0.0)
    for f in range(frames):
        k = start + f % G
        st.step(pool[k], slot=k, num_iter=5)
        s_ref = ref.step(pool64[k], k, 5)
        e_s = float((st.scores.double().cpu() - s_ref).abs().max())
        e_w = float((st.filter.double().cpu() - ref.filter[0]).abs().max())
        e_b = float((st.mem_bb.double().cpu() - ref.mem_bb).abs().max())
        flat = int(torch.argmax(s_ref))
        assert tuple(st.peak.cpu().numpy().astype(int)) == divmod(flat, s_ref.shape[1]), f
        assert e_s <= 1e-4 and e_w <= 1e-4 and e_b <= 1e-4, (f, e_s, e_w, e_b)
        worst = dict(scores=max(worst["scores"], e_s), filter=max(worst["filter"], e_w), bb=max(worst["bb"], e_b))
        if (f + 1) % G == 0:
            snaps[f + 1] = (st.filter.clone(), st.scores.clone(), st.mem_bb.clone(), st.mem_feat[start:start + G].clone())
    assert float(st.filter.abs().max()) > 1e-2                        # the filter left its zero start
    assert float(st.scores.abs().max()) > 1e-2                        # and the classification map is a real one
    st.filter.copy_(f0); st.mem_feat.copy_(m0); st.mem_bb.copy_(b0)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for f in range(G):
                st.step(pool[start + f], slot=start + f, num_iter=5)
        for rep in range(1, frames // G + 1):
            g.replay()
            stream.synchronize()
            w, s, b, m = snaps[rep * G]
            assert torch.equal(st.filter, w) and torch.equal(st.scores, s) and torch.equal(st.mem_bb, b), rep
            assert torch.equal(st.mem_feat[start:start + G], m)
    torch.cuda.current_stream().wait_stream(stream)
    print("PrDiMP closed-loop worst errors over %d frames:" % frames, worst)


# ------------------------------------------------------------------------------------------------------
# ToMP transformer model predictor
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [("tomp_small", "TOMP_SMALL"), ("tomp_full", "TOMP")])
def test_tomp_predictor_golden(name, cfg):
    """predict_cls_bbreg_filters_parallel + classifier + box regressor vs the reference run (tomp.py:282-303)."""
    g = load_golden(name)
    cfg = getattr(synth, cfg)
    pred, cls, reg = build_tomp_modules(cfg, synth.tomp_params(int(g["seed"]), cfg), DEV)
    train, test, lab, ltrb = [T(a) for a in synth.tomp_inputs(int(g["seed"]) + 1, cfg)]
    with torch.no_grad():
        close(pred.get_positional_encoding(test)[0, 0], g["pos"], atol=5e-6, rtol=0)
        cw, bw, cenc, benc = pred.predict_cls_bbreg_filters_parallel(train, test, lab, cfg["num_gth_frames"], ltrb)
        assert cw.shape == (1, cfg["D"], 1, 1) and cenc.shape == (1, 1, cfg["D"], cfg["H"], cfg["W"])
        close(cenc, g["cls_enc"], atol=1e-4, rtol=1e-4)
        close(benc, g["bbreg_enc"], atol=1e-4, rtol=1e-4)
        close(cw.reshape(-1), g["cls_filter"], atol=1e-4, rtol=1e-4)
        close(bw.reshape(-1), g["bbreg_filter"], atol=1e-4, rtol=1e-4)
        scores = cls(cenc, cw)
        close(scores, g["scores"], atol=1e-4, rtol=1e-4)
        boxes = reg(benc, bw)
        assert boxes.shape == g["ltrb"].shape
        close(boxes, g["ltrb"], atol=1e-4, rtol=1e-4)
        # heads alone on the reference's own encoder outputs (isolates them from the transformer's rounding)
        close(cls(T(g["cls_enc"]), T(g["cls_filter"]).reshape(1, -1, 1, 1)), g["scores"], atol=2e-5, rtol=1e-4)
        close(reg(T(g["bbreg_enc"]), T(g["bbreg_filter"]).reshape(1, -1, 1, 1)), g["ltrb"], atol=2e-5, rtol=1e-4)
        w1, enc1 = pred.predict_filter(train, test, lab, ltrb)
        close(w1.reshape(-1), g["single_filter"], atol=1e-4, rtol=1e-4)
        close(enc1, g["single_enc"], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("nhead", [4, 2, 8])
def test_tomp_encoder_blocks_vs_oracle(nhead):
    """Odd sizes against the float64 oracle: 3 memory frames, 5x7 maps (tokens not a multiple of any tile), two
    sequences through predict_filter, masked keys through the parallel entry point; head widths 32 / 64 / 16."""
    from oracle import tomp_oracle as TO
    cfg = dict(synth.TOMP_SMALL, H=5, W=7, n_train=3, feature_sz=7, num_gth_frames=2, nhead=nhead)
    params = synth.tomp_params(91, cfg)
    pred, cls, reg = build_tomp_modules(cfg, params, DEV)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    train, test, lab, ltrb = synth.tomp_inputs(92, cfg)
    train2, test2, lab2, ltrb2 = synth.tomp_inputs(93, cfg)
    f64 = lambda a: a.astype(np.float64)
    a = (cfg["nhead"], cfg["n_enc"], cfg["n_dec"], cfg["feature_sz"])
    with torch.no_grad():
        cw, bw, cenc, benc = pred.predict_cls_bbreg_filters_parallel(T(train), T(test), T(lab), 2, T(ltrb))
        rcw, rbw, rcenc, rbenc = TO.predict_cls_bbreg_filters_parallel(p64, f64(train), f64(test), f64(lab), 2, f64(ltrb), *a)
        close(cw.reshape(-1), rcw, atol=5e-5, rtol=1e-4)
        close(bw.reshape(-1), rbw, atol=5e-5, rtol=1e-4)
        close(cenc, rcenc, atol=5e-5, rtol=1e-4)
        close(benc, rbenc, atol=5e-5, rtol=1e-4)
        close(reg(benc, bw), TO.dense_box_regressor(p64, rbenc, rbw), atol=5e-5, rtol=2e-4)
        cat = lambda x, y: np.concatenate((x, y), axis=1)
        tr, te, lb, lt = cat(train, train2), cat(test, test2), cat(lab, lab2), cat(ltrb, ltrb2)
        w, enc = pred.predict_filter(T(tr), T(te), T(lb), T(lt))
        rw, renc = TO.predict_filter(p64, f64(tr), f64(te), f64(lb), f64(lt), *a)
        close(w.reshape(2, -1), rw, atol=5e-5, rtol=1e-4)
        close(enc, renc, atol=5e-5, rtol=1e-4)


# ------------------------------------------------------------------------------------------------------
# classification-feature head
# ------------------------------------------------------------------------------------------------------
def _clf_head(cin, cout, scale, w):
    from pytracking_amd import features as FM
    head = FM.residual_bottleneck(feature_dim=cin // 4, num_blocks=0, l2norm=True, final_conv=True, norm_scale=scale,
                                  out_dim=cout)
    head.load_state_dict({"0.weight": torch.from_numpy(w.copy())}, strict=True)
    return head.to(DEV).eval()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_clf_head_golden(tag):
    g = load_golden("clf_head")
    x, w = g[f"{tag}_x"], g[f"{tag}_w"]
    head = _clf_head(w.shape[1], w.shape[0], float(g[f"{tag}_scale"]), w)
    with torch.no_grad():
        close(head(T(x)), g[f"{tag}_y"], atol=2e-5, rtol=1e-4)
        close(head(T(x)[:, None])[:, 0], g[f"{tag}_y"], atol=2e-5, rtol=1e-4)      # leading dims are preserved


@pytest.mark.parametrize("n,cout", [(1, 512), (3, 256)])
def test_clf_head_tracker_sizes_vs_oracle(n, cout):
    """DiMP-50 (1024 -> 512, one frame) and ToMP (1024 -> 256, test + two memory frames) at 18x18."""
    rng = np.random.default_rng(33)
    x = rng.standard_normal((n, 1024, 18, 18), dtype=np.float32)
    w = rng.standard_normal((cout, 1024, 3, 3), dtype=np.float32) * np.float32(0.02)
    scale = float(np.sqrt(1.0 / (cout * 16)))
    head = _clf_head(1024, cout, scale, w)
    with torch.no_grad():
        y = head(T(x))
    ref = O.clf_head(x.astype(np.float64), w.astype(np.float64), scale)
    close(y, ref, atol=1e-6, rtol=1e-4)
    assert abs(float((y * y).sum(dim=(1, 2, 3)).mean()) - scale * scale * cout * 324) < 1e-3 * scale * scale * cout * 324


# ------------------------------------------------------------------------------------------------------
# target localisation on the device
# ------------------------------------------------------------------------------------------------------
def test_localize_advanced_golden():
    """pt_localize_decide_f32 (peaks AND outcome decided on the device) vs the reference's DiMP.localize_advanced on 48
    score maps (all four outcomes, the second-peak pick, two scales, exact ties): flag, scale and the float32 translation
    vector bit-exact; the 16 numbers the kernel leaves equal the oracle's restatement."""
    import ctypes
    from pytracking_amd import localization as LM
    from localize_cases import cases, constants
    for me, c in cases(load_golden("localize")):
        scores = T(c["scores"].copy())
        spos, sscl = torch.from_numpy(c["sample_pos"]), torch.from_numpy(c["sample_scales"])
        tv, scale_ind, s_out, flag = LM.localize_advanced(me, scores, spos, sscl)
        assert flag == str(c["flag"]) and int(scale_ind) == int(c["scale_ind"]) and s_out is scores
        assert not tv.is_cuda and tv.dtype == torch.float32
        np.testing.assert_array_equal(tv.numpy(), c["tv"])
        _, qd = constants(me, tuple(scores.shape), spos, sscl)
        want = O.localize_decide(c["scores"], c["scores"], qd)
        got = LM._host_out(scores.device)[1].astype(np.float64)
        np.testing.assert_array_equal(got[:15], want[:15])                  # [15]: the call's sequence number
        assert got[15] >= 1
        v = LM.two_peaks(scores, None, [np.array([3.3, 4.7], np.float32)] * scores.shape[0]).numpy().astype(np.float64)
        ref = O.two_peaks(c["scores"], c["scores"], [np.array([3.3, 4.7], np.float32)] * scores.shape[0])
        np.testing.assert_array_equal(v, ref)                               # bit-exact: values are copied, indices integral
        tv5 = LM.localize_advanced_tomp(me, scores, spos, sscl)
        assert len(tv5) == 5 and tv5[3] == flag and tv5[4].tolist() == want[2:4].tolist()


def test_localize_windowed_and_device_result_buffer():
    """`perform_hn_without_windowing` (dimp.py:247-250): the first peak is searched in the windowed map, the second in
    the raw one; and the kernel's result written to DEVICE memory equals the pinned-host result."""
    import ctypes
    from pytracking_amd import _lib, localization as LM
    from localize_cases import cases, constants
    rng = np.random.default_rng(3)
    for k, (me, c) in enumerate(cases(load_golden("localize"))):
        if k % 6:
            continue
        S, H, W = c["scores"].shape
        win = (0.2 + 0.8 * np.outer(np.hanning(H + 2)[1:-1], np.hanning(W + 2)[1:-1])).astype(np.float32)
        me.output_window = T(win)
        me.params.perform_hn_without_windowing = True
        raw = c["scores"].copy()
        scores = T(raw.copy())
        spos, sscl = torch.from_numpy(c["sample_pos"]), torch.from_numpy(c["sample_scales"])
        tv, scale_ind, s_hn, flag = LM.localize_advanced(me, scores, spos, sscl)
        np.testing.assert_array_equal(s_hn.cpu().numpy(), raw)              # the un-windowed clone is what is returned
        windowed = raw * win
        np.testing.assert_array_equal(scores.cpu().numpy(), windowed)       # `scores *= window` in place, as the reference
        q, qd = constants(me, (S, H, W), spos, sscl)
        want = O.localize_decide(windowed, raw, qd)
        np.testing.assert_array_equal(LM._host_out(scores.device)[1].astype(np.float64)[:15], want[:15])
        assert flag == O.LOC_FLAGS[int(want[0])]
        dev = torch.zeros(16, device=DEV)
        rc = _lib.lib().pt_localize_decide_f32(scores.data_ptr(), s_hn.data_ptr(), ctypes.byref(q), dev.data_ptr(), S, H, W,
                                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        np.testing.assert_array_equal(dev.cpu().numpy().astype(np.float64), want)


def test_max2d_vs_oracle_with_ties():
    from pytracking_amd import localization as LM
    rng = np.random.default_rng(8)
    a = rng.standard_normal((3, 2, 19, 23)).astype(np.float32)
    a[0, 0, 4, 7] = a[0, 0, 9, 7] = a[0, 0, 9, 2] = 9.0                      # ties: smallest column, then smallest row
    a[2, 1] = 0.0                                                            # a constant map -> [0, 0]
    mv, am = LM.max2d(T(a))
    assert mv.shape == (3, 2) and am.shape == (3, 2, 2) and am.dtype == torch.int64
    for i in range(3):
        for j in range(2):
            v, (r, c) = O.max2d(a[i, j])
            assert float(mv[i, j]) == float(v) and am[i, j].tolist() == [r, c]
    assert am[0, 0].tolist() == [9, 2]


# ------------------------------------------------------------------------------------------------------
# IoU-guided box refinement
# ------------------------------------------------------------------------------------------------------
class _IoUNetStandIn(torch.nn.Module):
    """The attributes of the reference's AtomIoUNet that the refinement reads (atom_iou_net.py:44-49), carrying the golden
    weights; the reference tree is not available on the GPU box."""

    def __init__(self, g):
        super().__init__()
        C, I = g["c3"].shape[1], g["w_fc3_rt.linear.bias"].shape[0]

        def block(k):
            m = torch.nn.Module()
            m.linear = torch.nn.Linear(C * k * k, I)
            m.bn = torch.nn.BatchNorm2d(I)
            m.relu = torch.nn.ReLU()
            return m
        self.fc3_rt, self.fc4_rt = block(5), block(3)
        self.iou_predictor = torch.nn.Linear(2 * I, 1)
        sd = {k[2:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("w_")}
        for blk in ("fc3_rt", "fc4_rt"):
            sd[f"{blk}.bn.num_batches_tracked"] = torch.tensor(0)
        self.load_state_dict(sd, strict=True)
        self.prroi_pool3t = types.SimpleNamespace(pooled_height=5, pooled_width=5, spatial_scale=1 / 8)
        self.prroi_pool4t = types.SimpleNamespace(pooled_height=3, pooled_width=3, spatial_scale=1 / 16)


def _iou_box_check(boxes, iou, g, tag, relative, atom=False):
    """north_star bound (1e-4 px / 1e-4 IoU) against the float64 restatement of the same refinement -- or, where the
    REFERENCE's own float32 run is further than that from float64 (|reference - float64|, measured here), twice the
    reference's rounding error: the step length amplifies float32 gradient noise (ATOM relative space, step 6e-2: the
    reference itself is 1.2e-3 px from float64, this path 6.9e-4; profiles/r02_iou_rounding_study.txt)."""
    from oracle import iou_oracle as IO
    t64 = lambda a: torch.from_numpy(a.astype(np.float64))
    p = {k[2:]: t64(v) for k, v in g.items() if k.startswith("w_")}
    iters, step, decay = g[f"{tag}_cfg"]
    fn = IO.refine_atom if atom else IO.refine
    out = fn(p, (t64(g["mod3"]), t64(g["mod4"])), (t64(g["c3"]), t64(g["c4"])), t64(g["boxes"]), int(iters), float(step),
             float(decay), relative)
    b64, i64 = out[0].numpy(), out[1].numpy()
    ref_err_b = float(np.abs(g[f"{tag}_boxes"] - b64).max())
    ref_err_i = float(np.abs(g[f"{tag}_iou"] - i64).max())
    # the relaxation cannot inflate itself: if the float64 restatement drifts from the reference golden (an oracle bug),
    # this fails instead of loosening the GPU bound (measured: 1.2e-3 px / 3e-5 IoU at worst)
    assert ref_err_b < 5e-3 and ref_err_i < 2e-4, (ref_err_b, ref_err_i)
    close(boxes, b64, atol=max(1e-4, 2 * ref_err_b))
    close(iou, i64, atol=max(1e-4, 2 * ref_err_i))
    close(boxes, g[f"{tag}_boxes"], atol=1e-4 + 2 * ref_err_b)
    close(iou, g[f"{tag}_iou"], atol=1e-4 + 2 * ref_err_i)


@pytest.mark.parametrize("tag,relative", [("default", False), ("default_decay", False), ("relative", True)])
def test_iou_refinement_golden(tag, relative):
    """optimize_boxes_default / optimize_boxes_relative (dimp.py:725-788) vs the reference run on CPU."""
    from pytracking_amd import iou_refine as IR
    g = load_golden("iou_refine")
    net = _IoUNetStandIn(g).to(DEV).eval()
    iters, step, decay = g[f"{tag}_cfg"]
    params = types.SimpleNamespace(box_refinement_iter=int(iters), box_refinement_step_length=float(step),
                                   box_refinement_step_decay=float(decay))
    me = types.SimpleNamespace(params=params, net=types.SimpleNamespace(bb_regressor=net),
                               iou_modulation=(T(g["mod3"]), T(g["mod4"])))
    fn = IR.optimize_boxes_relative if relative else IR.optimize_boxes_default
    boxes, iou = fn(me, (T(g["c3"]), T(g["c4"])), torch.from_numpy(g["boxes"].copy()))
    assert not boxes.is_cuda and boxes.shape == (10, 4) and iou.shape == (10,)
    _iou_box_check(boxes, iou, g, tag, relative)
    assert float(np.abs(g[f"{tag}_boxes"] - g["boxes"]).max()) > 2.0           # the boxes really moved
    b2, i2 = fn(me, (T(g["c3"]), T(g["c4"])), torch.from_numpy(g["boxes"].copy()))   # cached pack / prepared buffers
    assert torch.equal(b2, boxes) and torch.equal(i2, iou)
    if tag == "default":                                                       # tuple step length (dimp.py:737-738)
        params.box_refinement_step_length = (float(step), float(step))
        b3, _ = fn(me, (T(g["c3"]), T(g["c4"])), torch.from_numpy(g["boxes"].copy()))
        assert torch.equal(b3, boxes)


@pytest.mark.parametrize("tag,relative,backtrack", [("default", False, False), ("relative", True, False), ("atom_default", False, True)])
def test_iou_refinement_paths_agree(tag, relative, backtrack):
    """One refinement, three routes through the library: the per-frame call (proposals from host memory in a kernel argument block,
    results polled from pinned host memory: pt_iou_refine_sync_f32), device in / device out on the fused iteration
    (pt_iou_refine_f32, <= 16 proposals), and the unfused six-launch iteration that serves larger proposal sets -- the first two
    bit-identical, the third (other summation order; here on 20 proposals = the 10 golden ones twice: proposals are independent
    of each other in an eval-mode network) under the SAME rule as every other refinement test (`_iou_box_check`: the north_star
    bound against the float64 restatement and the reference golden)."""
    from pytracking_amd import iou_refine as IR
    g = load_golden("iou_refine")
    net = _IoUNetStandIn(g).to(DEV).eval()
    mod, feat = (T(g["mod3"]), T(g["mod4"])), (T(g["c3"]), T(g["c4"]))
    b0 = torch.from_numpy(g["boxes"].copy())
    iters, step, decay = g[f"{tag}_cfg"]
    iters, step, decay = int(iters), float(step), float(decay)
    host = IR.refine_boxes(net, mod, feat, b0, iters, step, decay, relative, backtrack=backtrack, to_host=True)
    dev = IR.refine_boxes(net, mod, feat, b0.to(DEV), iters, step, decay, relative, backtrack=backtrack)
    assert not host[0].is_cuda and dev[0].is_cuda
    assert torch.equal(host[0], dev[0].cpu()) and torch.equal(host[1], dev[1].cpu())
    _iou_box_check(host[0], host[1], g, tag, relative, atom=backtrack)
    big = IR.refine_boxes(net, mod, feat, torch.cat((b0, b0)).to(DEV), iters, step, decay, relative, backtrack=backtrack)
    assert big[0].shape == (20, 4)
    for half in (slice(0, 10), slice(10, 20)):
        _iou_box_check(big[0][half], big[1][half], g, tag, relative, atom=backtrack)
    assert torch.equal(big[0][:10], big[0][10:]) and torch.equal(big[1][:10], big[1][10:])


@pytest.mark.parametrize("tag,space", [("atom_default", "default"), ("atom_relative", "relative"), ("atom_nodecay", "default")])
def test_iou_refinement_atom_golden(tag, space):
    """ATOM.optimize_boxes (atom.py:758-836) with per-proposal backtracking vs the reference run on CPU.  Backtracking is
    a discontinuous decision on `iou > previous iou`; the golden cases keep a margin, the tolerance is the smooth one."""
    from pytracking_amd import iou_refine as IR
    g = load_golden("iou_refine")
    net = _IoUNetStandIn(g).to(DEV).eval()
    iters, step, decay = g[f"{tag}_cfg"]

    class P(types.SimpleNamespace):
        def get(self, name, default=None):
            return getattr(self, name, default)
    params = P(box_refinement_iter=int(iters), box_refinement_step_length=float(step), box_refinement_step_decay=float(decay),
               box_refinement_space=space)
    me = types.SimpleNamespace(params=params, iou_predictor=net, target_feat=(T(g["mod3"]), T(g["mod4"])))
    boxes, iou = IR.optimize_boxes_atom(me, (T(g["c3"]), T(g["c4"])), torch.from_numpy(g["boxes"].copy()))
    _iou_box_check(boxes, iou, g, tag, space == "relative", atom=True)


# ------------------------------------------------------------------------------------------------------
# round 2: full-size / deployed-size reference vectors and the branches that had no coverage
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dimp_sd_bentpar", "dimp_sd_linmask", "dimp_sd_bentpar_linmask", "dimp_sd_bentpar_c128"])
def test_dimp_sd_activation_branches_golden(name):
    """PT_ACT_BENTPAR (activation.py:47-66) and PT_MASK_LINEAR (optimizer.py:57-66) on the generic kernels (C=16) and
    on the XCD-aligned path (C=128, 18x18), against the reference."""
    g = load_golden(name)
    if "feat" in g:
        w0, feat, bb, sw = g["w0"], g["feat"], g["bb"], g["sw"]
        over = dict(score_act=str(g["score_act"]), mask_act=str(g["mask_act"]))
    else:
        w0, feat, bb, sw = synth.dimp_problem(int(g["seed"]), int(g["n"]), small=dict(C=128, H=18, W=18))
        over = dict(score_act="bentpar", mask_act="linear")
    from pytracking_amd import optimizer
    c = dict(synth.DIMP50, **over)
    mod = optimizer.DiMPSteepestDescentGN(
        num_iter=3, feat_stride=c["feat_stride"], init_step_length=c["init_step_length"],
        init_filter_reg=c["init_filter_reg"], init_gauss_sigma=c["init_gauss_sigma"], num_dist_bins=c["num_dist_bins"],
        bin_displacement=c["bin_displacement"], mask_init_factor=c["mask_init_factor"], score_act=c["score_act"],
        act_param=float(g["act_param"]) or None, mask_act=c["mask_act"], min_filter_reg=c["min_filter_reg"],
        alpha_eps=c["alpha_eps"]).to(DEV).eval()
    its, losses = _run(mod, w0, feat, bb, sw, int(g["num_iter"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses.reshape(-1), g["losses"], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("name", ["prdimp_sd_sigma0", "prdimp_sd_sigma0_c128"])
def test_prdimp_one_hot_label_golden(name):
    """gauss_sigma == 0 (optimizer.py:334-341; sd_common.h one-hot branch), generic and XCD-aligned path."""
    g = load_golden(name)
    if "feat" in g:
        w0, feat, bb, sw = g["w0"], g["feat"], g["bb"], g["sw"]
    else:
        w0, feat, bb, sw = synth.dimp_problem(int(g["seed"]), int(g["n"]), synth.PRDIMP50, small=dict(C=128, H=18, W=18))
        w0 = w0 * 0
    its, losses = _run(_prdimp_module(gauss_sigma=0.0), w0, feat, bb, sw, int(g["num_iter"]))
    close(its, g["iterates"], atol=2e-5)
    close(losses.reshape(-1), g["losses"], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("name", ["dimp_sd_two_sequences", "prdimp_sd_two_sequences"])
def test_sd_two_sequences_golden(name):
    """S = 2 through the optimiser mirror: feat (n,S,C,H,W), weights (S,C,K,K), bb (n,S,4), sample_weight (n,S); the
    losses keep the reference's shape (1,) so that `torch.cat(losses)` (dimp.py:583,641) works."""
    g = load_golden(name)
    mod = _dimp_module() if name.startswith("dimp") else _prdimp_module()
    with torch.no_grad():
        w, its, losses = mod(T(g["w0"]), T(g["feat"]), T(g["bb"]), sample_weight=T(g["sw"]), num_iter=int(g["num_iter"]),
                             compute_losses=True)
    assert w.shape == g["w0"].shape and len(its) == int(g["num_iter"]) + 1
    close(torch.stack(its), g["iterates"], atol=2e-5)
    assert losses[0].shape == (1,)
    close(torch.cat(losses), g["losses"][:, 0], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("tag", ["pr", "fr"])
def test_atom_cg_direction_forgetting_golden(tag):
    """direction_forget_factor != 0: the CG state (p, rho, r_prev) is carried across run() calls
    (optimization.py:82-85; atom_cg.hip cg_state)."""
    from pytracking_amd.optimization import ConjugateGradient, ConvProblem, MLU
    g = load_golden(f"atom_cg_forget_{tag}")
    x = [T(g["x0"].copy())[None].clone()]
    prob = ConvProblem([T(g["samples"])], [T(g["y"])[:, None]], [synth.ATOM18["filter_reg"]], [T(g["sw"])],
                       MLU(synth.ATOM18["act_min_val"]))
    opt = ConjugateGradient(prob, x, fletcher_reeves=bool(int(g["fletcher_reeves"])), direction_forget_factor=float(g["forget"]))
    for call, iters in enumerate(g["iters"]):
        opt.run(int(iters))
        close(x[0][0], g["x_out"][call], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("tag", ["pr", "fr", "pr0", "fr0"])
def test_atom_cg_compressed_channels_golden(tag):
    """C = 64, 4x4 filter -- the channel count and filter of ATOM's online update -- on a 12x12 map: two position tiles, so the GENERIC
    route of csrc/atom_cg.hip (the fused one needs 4 or 5 tiles; tests/test_gpu_atom_routes.py runs this golden's 16x16 twin and every
    other cell of it): Polak-Ribiere / Fletcher-Reeves, with / without direction forgetting, state carried over three run() calls,
    against the reference's autograd CG."""
    import ctypes
    from pytracking_amd import _lib
    from pytracking_amd.optimization import ConjugateGradient, ConvProblem, MLU
    g = load_golden("atom_cg_c64")
    x0, samples, y, sw = synth.atom_problem(int(g["seed"]), int(g["n"]), small=dict(C=64, H=int(g["H"]), W=int(g["W"])))
    x = [T(x0.copy())[None].clone()]
    route = (ctypes.c_int * 5)()
    assert _lib.lib().pt_atom_cg_route(x[0].data_ptr(), 256, 64 * 144, 256, int(g["n"]), 64, int(g["H"]), int(g["W"]), 4, route) == 0
    assert list(route) == [0, 1, 4, 4, 1]                               # generic, 16-byte loads, 4 k-steps per slice, 4 channel slices, 1 adjoint slice
    prob = ConvProblem([T(samples)], [T(y)[:, None]], [synth.ATOM18["filter_reg"]], [T(sw)], MLU(synth.ATOM18["act_min_val"]))
    opt = ConjugateGradient(prob, x, fletcher_reeves=bool(int(g[f"{tag}_fr"])), direction_forget_factor=float(g[f"{tag}_forget"]))
    for call, iters in enumerate(g["iters"]):
        opt.run(int(iters))
        close(x[0][0], g[f"{tag}_x_out"][call], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("tag,fr", [("pr", False), ("fr", True)])
def test_atom_joint_gn_first_frame_schedule_golden(tag, fr):
    """ATOM first frame at the deployed schedule: 6 Gauss-Newton x 10 CG iterations on 30 x 256 x 18 x 18 samples, 64
    compressed channels, 4x4 filter (parameter/atom/default.py:27-28,30), against the reference's autograd run."""
    g = load_golden("atom_gn_first_frame")
    f0, P0, samples, y, sw = synth.atom_gn_problem(int(g["seed"]))
    f, P = _atom_gn_run(f0, P0, samples, y, sw, [10] * 6, fr, float(g["filter_reg"]), float(g["projection_reg"]),
                        float(g["act_min_val"]))
    close(f, g[f"f_out_{tag}"], atol=1e-4)
    close(P, g[f"P_out_{tag}"], atol=1e-4)


@pytest.mark.parametrize("num_iter", [3, 4])
def test_lwl_gn_config5_full_size_golden(num_iter):
    """BASELINE configs[4] at full size: n = 32 samples of 512 x 30 x 52, 16 filters 3x3, 3 iterations (the reference's
    per-frame setting, lwl_ytvos.py:26) and 4 (BASELINE's wording), against the reference's autograd run on CPU."""
    from pytracking_amd import filter as FL
    g = load_golden("lwl_gn_cfg5_n32")
    w0, feat, label, sw = synth.lwl_problem(int(g["seed"]))
    its, losses = _lwl_run(w0, feat, label, sw, num_iter, float(g["filter_reg"]), 0.0)
    close(its[1], g["iterate1"], atol=2e-5)
    close(its[-1], g[f"final{num_iter}"], atol=1e-4)
    close(losses, g[f"losses{num_iter}"], atol=1e-7, rtol=1e-4)
    if num_iter == 4:
        s = FL.apply_filter(T(feat[:2])[:, None], its[-1][None])[:, 0]
        close(s, g["scores_first2"], atol=1e-4)


@pytest.mark.parametrize("n", [1, 32])
def test_lwl_gn_config5_twenty_iterations_golden(n):
    """LWL's first-frame setting `net_opt_iter = 20` (lwl_ytvos.py:30) at the configs[4] geometry, n = 1 (the first frame
    of every sequence) and n = 32: the fused solver carries the scores by recurrence -- final filter, iterate 10, all 21
    losses and the scores under the final filter against the reference's autograd run bound the drift."""
    from pytracking_amd import filter as FL
    g = load_golden(f"lwl_gn_cfg5_n{n}_it20")
    w0, feat, label, sw = synth.lwl_problem(int(g["seed"]), dict(synth.LWL, n=n))
    its, losses = _lwl_run(w0, feat, label, sw, 20, float(g["filter_reg"]), 0.0)
    close(its[-1], g["final"], atol=1e-4)
    close(its[10], g["iterate10"].astype(np.float64), atol=2e-3, rtol=2e-3)      # stored as float16
    close(losses, g["losses"], atol=1e-7, rtol=1e-4)
    s = FL.apply_filter(T(feat[:1])[:, None], its[-1][None])[:, 0]
    close(s, g["scores_first"], atol=1e-4)
    ls = losses.cpu().numpy()
    assert np.all(np.diff(ls) <= 1e-6 * ls[0]) and ls[-1] < ls[0]         # non-increasing up to float32 rounding at convergence


def test_dimp_sd_twenty_iterations_golden():
    """DiMP at 20 iterations (4x the tracker's setting; the ABI allows 64) at the configs[1] geometry, n = 15: iterates
    5 / 10 / 20, the 21 losses and the final scores against the reference -- no drift of s_t = s_{t-1} - a (F g)."""
    from pytracking_amd import filter as F
    g = load_golden("dimp_sd_cfg2_n15_it20")
    w0, feat, bb, sw = synth.dimp_problem(int(g["seed"]), int(g["n"]))
    its, losses = _run(_dimp_module(), w0, feat, bb, sw, 20)
    close(its[g["which"]], g["iterates"], atol=1e-4)
    close(losses, g["losses"], atol=1e-4, rtol=1e-4)
    close(F.apply_filter(T(feat), its[-1][None])[:, 0], g["scores"], atol=1e-4)


class _IoUNetFromParams(torch.nn.Module):
    """AtomIoUNet's test branch (atom_iou_net.py:44-49) carrying the seeded weights of synth.iou_net_params."""

    def __init__(self, p, C, I):
        super().__init__()

        def block(k):
            m = torch.nn.Module()
            m.linear = torch.nn.Linear(C * k * k, I)
            m.bn = torch.nn.BatchNorm2d(I)
            m.relu = torch.nn.ReLU()
            return m
        self.fc3_rt, self.fc4_rt = block(5), block(3)
        self.iou_predictor = torch.nn.Linear(2 * I, 1)
        sd = {k: torch.from_numpy(v.copy()) for k, v in p.items()}
        for blk in ("fc3_rt", "fc4_rt"):
            sd[f"{blk}.bn.num_batches_tracked"] = torch.tensor(0)
        self.load_state_dict(sd, strict=True)
        self.prroi_pool3t = types.SimpleNamespace(pooled_height=5, pooled_width=5, spatial_scale=1 / 8)
        self.prroi_pool4t = types.SimpleNamespace(pooled_height=3, pooled_width=3, spatial_scale=1 / 16)


@pytest.mark.parametrize("tag", ["default", "relative", "atom"])
def test_iou_refinement_deployed_size_golden(tag):
    """IoU-guided refinement at the deployed sizes (256-channel IoU features 36x36 / 18x18, 256-wide LinearBlocks, 10
    proposals): DiMP-50 default (5 it), PrDiMP-50 relative (10 it), ATOM backtracking, against the reference on CPU.
    north_star bound: 1e-4 on IoU and on the boxes (pixels)."""
    from pytracking_amd import iou_refine as IR
    g = load_golden("iou_refine_full")
    cfg = synth.IOU50
    net = _IoUNetFromParams(synth.iou_net_params(int(g["param_seed"])), cfg["C"], cfg["I"]).to(DEV).eval()
    c3, c4, m3, m4, boxes = synth.iou_inputs(int(g["input_seed"]))
    iters, step, decay = g[f"{tag}_cfg"]

    class P(types.SimpleNamespace):
        def get(self, name, default=None):
            return getattr(self, name, default)
    params = P(box_refinement_iter=int(iters), box_refinement_step_length=float(step), box_refinement_step_decay=float(decay),
               box_refinement_space="default")
    if tag == "atom":
        me = types.SimpleNamespace(params=params, iou_predictor=net, target_feat=(T(m3), T(m4)))
        b, iou = IR.optimize_boxes_atom(me, (T(c3), T(c4)), torch.from_numpy(boxes.copy()))
    else:
        me = types.SimpleNamespace(params=params, net=types.SimpleNamespace(bb_regressor=net), iou_modulation=(T(m3), T(m4)))
        fn = IR.optimize_boxes_relative if tag == "relative" else IR.optimize_boxes_default
        b, iou = fn(me, (T(c3), T(c4)), torch.from_numpy(boxes.copy()))
    close(iou, g[f"{tag}_iou"], atol=1e-4)
    close(b, g[f"{tag}_boxes"], atol=1e-4)
    assert float(np.abs(g[f"{tag}_boxes"] - boxes).max()) > 2.0


@pytest.mark.parametrize("tag", ["default", "relative", "atom"])
def test_iou_refinement_deployed_size_unfused_route(tag):
    """The unfused iteration (more than 16 proposals: `k_iou_setup` / `k_prroi_*2` / `k_gemm_pair` / `k_iou_head` /
    `k_iou_update`) at the DEPLOYED sizes (256-channel IoU features, 256-wide LinearBlocks): 20 proposals = the golden's 10
    twice (an eval-mode network treats proposals independently, atom_iou_net.py:96-136), each half against the reference run
    at the north_star bound 1e-4 (IoU and pixels) -- the same bar as the fused route in the test above."""
    from pytracking_amd import iou_refine as IR
    g = load_golden("iou_refine_full")
    cfg = synth.IOU50
    net = _IoUNetFromParams(synth.iou_net_params(int(g["param_seed"])), cfg["C"], cfg["I"]).to(DEV).eval()
    c3, c4, m3, m4, boxes = synth.iou_inputs(int(g["input_seed"]))
    iters, step, decay = g[f"{tag}_cfg"]
    b20 = torch.from_numpy(np.concatenate((boxes, boxes))).to(DEV)
    b, iou = IR.refine_boxes(net, (T(m3), T(m4)), (T(c3), T(c4)), b20, int(iters), float(step), float(decay),
                             tag == "relative", backtrack=(tag == "atom"))
    assert b.shape == (20, 4) and iou.shape == (20,)
    for half in (slice(0, 10), slice(10, 20)):
        close(iou[half], g[f"{tag}_iou"], atol=1e-4)
        close(b[half], g[f"{tag}_boxes"], atol=1e-4)


def test_track_frame_is_deterministic_under_repeated_launches():
    """Determinism under cache churn: every reduction of the frame (score-map slices, gradient partials, per-sample
    curvature terms) is summed in a fixed order by a fixed owner, and kernels hand data to each other only across launch
    boundaries (the in-launch hand-offs tried in round 2 were reverted, profiles/HISTORY.md section 8) -- so 300 frames from identical
    state must give bit-identical filters, scores and boxes every time, whatever ran in between."""
    from pytracking_amd import bench_frame
    cfg = synth.DIMP50
    st = bench_frame.TrackState(cfg, 50, seed=321, device=DEV)
    rng = np.random.default_rng(322)
    x = T(synth.clf_features(rng, 1, cfg["C"], cfg["H"], cfg["W"], cfg["K"])[0])
    f0, m0, b0 = st.filter.clone(), st.mem_feat.clone(), st.mem_bb.clone()
    ref = None
    junk = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    for rep in range(300):
        st.filter.copy_(f0); st.mem_feat.copy_(m0); st.mem_bb.copy_(b0)
        if rep % 3 == 0:
            junk.fill_(rep & 255)                                   # uneven load / cache churn between the frames
        st.step(x, slot=rep % 50 if rep % 2 else 7, num_iter=5)
        if rep % 2 == 0:                                            # same slot -> same result
            out = (st.filter.clone(), st.scores.clone(), st.mem_bb.clone())
            if ref is None:
                ref = out
            else:
                assert all(torch.equal(a, b) for a, b in zip(out, ref)), rep
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------
# image-patch sampling on the device
# ------------------------------------------------------------------------------------------------------
def test_sample_patch_golden():
    """pt_sample_patch_f32 behind the mirrored `sample_patch` / `sample_patch_multiscale` against 24 + 3 reference runs
    (preprocessing.py:33-148): border modes replicate / inside / inside_major, pre-downsampling strides 1..8, crops
    over every border.  Pixels are 0..255, bound 1e-4 (north_star): the source index is ONE fused multiply-add as in this
    image's ATen build (unfused it was 5e-4 off); the coordinates are exact."""
    from pytracking_amd import preprocessing as PP
    g = load_golden("sample_patch")
    im = T(g["im"])
    exact = 0
    for k in range(int(g["n"])):
        msc = float(g[f"c{k}_msc"])
        patch, coord = PP.sample_patch(im, torch.from_numpy(g[f"c{k}_pos"]), torch.from_numpy(g[f"c{k}_ssz"]),
                                       torch.from_numpy(g[f"c{k}_osz"]).float(), mode=str(g[f"c{k}_mode"]),
                                       max_scale_change=None if msc < 0 else msc)
        assert patch.shape == g[f"c{k}_patch"].shape
        np.testing.assert_array_equal(coord.numpy(), g[f"c{k}_coord"])
        close(patch, g[f"c{k}_patch"], atol=1e-4, rtol=0)
        exact += int(np.array_equal(patch.cpu().numpy(), g[f"c{k}_patch"]))
    assert exact >= 16                                                   # most cases are bit-identical
    ps, cs = PP.sample_patch_multiscale(im, torch.from_numpy(g["ms_pos"]), torch.from_numpy(g["ms_scales"]),
                                        torch.Tensor([32.0, 32.0]))
    np.testing.assert_array_equal(cs.numpy(), g["ms_coords"])
    close(ps, g["ms_patches"], atol=1e-4, rtol=0)
    ref = O.sample_patch_pixels(g["im"][0], 1, 0, 0, 5, 7, 20, 30, (20, 30))  # no resize: an exact copy of the crop
    geom = PP._lib.PatchGeom(1, 0, 0, 5, 7, 20, 30)
    out = torch.empty(1, 3, 20, 30, device=DEV)
    from pytracking_amd.filter import _ptr, _stream
    PP._lib.check(PP._lib.lib().pt_sample_patch_f32(_ptr(im), 3, 70, 90, (PP._lib.PatchGeom * 1)(geom), 1, _ptr(out), 20, 30,
                                                    _stream()), "pt_sample_patch_f32")
    assert np.array_equal(out[0].cpu().numpy(), ref) and np.array_equal(ref, g["im"][0][:, 5:25, 7:37])


@pytest.mark.parametrize("tag", ["s", "n", "d"])
def test_augmentation_set_golden(tag):
    """pt_augment_patches_f32 behind the mirrored `sample_patch_transformed` (preprocessing.py:13-30) against the reference's output
    for lists of its own transforms (augmentation.py: Identity, Translation, FlipHorizontal, FlipVertical, Blur, Scale; `d` = the
    DiMP-50 first-frame list, 576 -> 288 with random shifts, dimp.py:329-395).  The transform objects are stand-ins with the
    reference classes' names and attributes (tests/augment_cases.py).  Pixels 0..255 within 1e-4; flips / shifts / crops of the
    base patch must reproduce the device base patch bit for bit."""
    from pytracking_amd import preprocessing as PP
    from augment_cases import read_case
    c = read_case(load_golden("augment"), tag)
    im = T(c["im"])
    out = PP.sample_patch_transformed(im, torch.from_numpy(c["pos"]), c["scale"], torch.from_numpy(c["image_sz"]), c["objs"])
    assert tuple(out.shape) == c["shape"]
    st = c["stride"]
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:, :, ::st, ::st], c["out"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(got.astype(np.float64).sum(axis=(1, 2, 3)), c["sums"], rtol=1e-7)
    # against the oracle applied to the DEVICE base patch: the pure gathers are exact, blur / scale within an ulp or two
    base, _ = PP.sample_patch(im, torch.from_numpy(c["pos"]), c["scale"] * torch.from_numpy(c["image_sz"]), torch.from_numpy(c["image_sz"]))
    ref = O.augment_patch(base[0].cpu().numpy(), c["specs"])
    for k, sp in enumerate(c["specs"]):
        if sp["kind"] in ("identity", "fliplr", "flipud"):
            assert np.array_equal(got[k], ref[k]), (k, sp["kind"])
        else:
            np.testing.assert_allclose(got[k], ref[k], atol=1e-4, rtol=0)


def test_augmentation_rotate_unpinned_and_errors():
    """`Rotate` (augmentation.py:111-126, cv2.warpAffine) has no golden -- cv2 is not installed where goldens are made: the
    kernel is checked against the oracle's independent restatement of OpenCV's published arithmetic (PARITY UNPINNED), plus
    the properties any implementation must have: angle 0 is the identity, a constant image stays constant, 180 degrees about
    the centre reverses both axes.  Lists longer than one launch's argument block are split; unknown transforms are refused."""
    from pytracking_amd import preprocessing as PP
    from augment_cases import rotate_pair, Identity
    rng = np.random.default_rng(4)
    patch = rng.integers(0, 256, size=(1, 3, 64, 64)).astype(np.float32)
    dp = T(patch)
    specs, objs = zip(*[rotate_pair(a, [48, 48], (2, -3)) for a in (10, -10, 45, -45, 0, 180)])
    out = PP.augment_patch(dp, list(objs)).cpu().numpy()
    ref = O.augment_patch(patch[0], list(specs))
    np.testing.assert_allclose(out, ref, atol=1e-4, rtol=0)
    ident = O.augment_patch(patch[0], [{"kind": "identity", "output_sz": [48, 48], "shift": (2, -3)}])[0]
    assert np.array_equal(out[4], ident)
    full = PP.augment_patch(dp, [rotate_pair(180, None, (0, 0))[1]]).cpu().numpy()[0]
    np.testing.assert_allclose(full, patch[0][:, ::-1, ::-1], atol=1e-4, rtol=0)
    const = PP.augment_patch(torch.full((1, 1, 40, 40), 7.0, device=DEV), [rotate_pair(33, None, (0, 0))[1]])
    assert torch.all(const == 7.0)
    many = [Identity([48, 48], (k - 15, 15 - k)) for k in range(31)]                 # > PT_AUG_MAX_TRANSFORMS: two launches
    outm = PP.augment_patch(dp, many).cpu().numpy()
    refm = O.augment_patch(patch[0], [{"kind": "identity", "output_sz": [48, 48], "shift": m.shift} for m in many])
    assert np.array_equal(outm, refm)

    class RandomAffine:
        output_sz, shift = None, (0, 0)
    with pytest.raises(NotImplementedError):
        PP.augment_patch(dp, [RandomAffine()])
    with pytest.raises(NotImplementedError):
        PP.sample_patch_transformed(dp, torch.Tensor([30.0, 30.0]), 1.0, torch.Tensor([32.0, 32.0]), [Identity(None, (0, 0))], is_mask=True)


def test_track_frame_with_head_writes_the_memory_slot():
    """pt_track_frame_head_f32 (second half): head output lands in the memory slot and the frame is
    bit-identical to head -> pt_track_frame_f32 on the separately materialised test feature."""
    from pytracking_amd import bench_frame, features as FM
    cfg = dict(synth.DIMP50)
    rng = np.random.default_rng(61)
    w = rng.standard_normal((512, 1024, 3, 3), dtype=np.float32) * np.float32(0.02)
    scale = float(np.sqrt(1.0 / (512 * 16)))
    xb = T(rng.standard_normal((1024, 18, 18), dtype=np.float32))
    a = bench_frame.TrackState(cfg, 12, seed=62, device=DEV)
    b = bench_frame.TrackState(cfg, 12, seed=62, device=DEV)
    a.attach_head(T(w), scale)
    a.step_from_backbone(xb, slot=5, num_iter=5)
    head = _clf_head(1024, 512, scale, w)
    with torch.no_grad():
        feat = head(xb[None])[0].contiguous()
    b.step(feat, slot=5, num_iter=5)
    torch.cuda.synchronize()
    assert torch.equal(a.mem_feat[5], feat) and torch.equal(a.mem_feat, b.mem_feat)
    assert torch.equal(a.scores, b.scores) and torch.equal(a.filter, b.filter) and torch.equal(a.mem_bb, b.mem_bb)


@pytest.mark.parametrize("mode", ["back_to_back", "side_streams_eager", "side_streams_captured"])
@pytest.mark.parametrize("kind", ["dimp", "prdimp"])
def test_sd_multi_sequence_batch_equals_single_sequence_calls(kind, mode):
    """S = 5 sequences through ONE pt_sd_solve_batch_f32 call against five single-sequence solves: bit-equal iterates and losses (the
    same kernels on the same operands; only the streams differ), at the deployed map size.
      back_to_back          : n_aux = 0, what an eager call of the module does -- all sequences on the current stream
      side_streams_eager    : n_aux = 3 in eager mode (optimizer.EAGER_SIDE_STREAMS): this stream + 3 side streams, the fifth sequence
                              sharing the first lane -- the fork / join path of sd_solver.hip with every result checked
      side_streams_captured : the same inside a torch.cuda.graph capture (what the module does on its own when captured), replayed twice
    A missing join or overlapping workspaces would show up as differing iterates."""
    from pytracking_amd import optimizer as OM
    cfg = synth.DIMP50 if kind == "dimp" else synth.PRDIMP50
    S, n, C = 5, 9, 128
    probs = [synth.dimp_problem(900 + s, n, dict(cfg, C=C)) for s in range(S)]
    w0 = torch.stack([T(p[0]) for p in probs])                                   # (S,C,K,K)
    feat = torch.stack([T(p[1]) for p in probs], dim=1).contiguous()              # (n,S,C,H,W)
    bb = torch.stack([T(p[2]) for p in probs], dim=1).contiguous()                # (n,S,4)
    sw = torch.stack([T(p[3]) for p in probs], dim=1).contiguous()                # (n,S)
    mod = _dimp_module(cfg) if kind == "dimp" else _prdimp_module(cfg)
    with torch.no_grad():
        single = []
        for s in range(S):
            _, its_s, l_s = mod(w0[s:s + 1], feat[:, s].contiguous(), bb[:, s].contiguous(), sample_weight=sw[:, s].contiguous(),
                                num_iter=4, compute_losses=True)
            single.append((torch.stack(its_s)[:, 0], torch.cat(l_s)))
        torch.cuda.synchronize()
        if mode == "side_streams_captured":
            mod(w0, feat, bb, sample_weight=sw, num_iter=4, compute_losses=True)          # workspaces / side streams exist before the capture
            torch.cuda.synchronize()
            side = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(side):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    _, its, losses = mod(w0, feat, bb, sample_weight=sw, num_iter=4, compute_losses=True)
                for _ in range(2):
                    g.replay()
                side.synchronize()
        else:
            OM.EAGER_SIDE_STREAMS = mode == "side_streams_eager"
            try:
                _, its, losses = mod(w0, feat, bb, sample_weight=sw, num_iter=4, compute_losses=True)
            finally:
                OM.EAGER_SIDE_STREAMS = False
            torch.cuda.synchronize()
    batch_its = torch.stack(its[1:])                                              # (T,S,C,K,K); its[0] is the caller's tensor
    for s in range(S):
        assert torch.equal(batch_its[:, s], single[s][0][1:]), (mode, s)
    tot = sum(x[1] for x in single) / S
    close(torch.cat(losses), tot.cpu().numpy(), atol=1e-6, rtol=1e-6)


def test_sd_multi_sequence_refuses_bad_side_streams_before_forking():
    """pt_sd_solve_batch_f32 validates EVERY auxiliary stream before it records the fork event: a null or repeated later entry returns
    PT_ERR_SHAPE with nothing queued on the earlier streams (sd_solver.hip; advisor finding of round 5)."""
    import ctypes
    from pytracking_amd import _lib
    cfg = synth.DIMP50
    S, n, C = 3, 4, 64
    L = _lib.lib()
    probs = [synth.dimp_problem(950 + s, n, dict(cfg, C=C)) for s in range(S)]
    from pytracking_amd import bench_frame
    holder = bench_frame.TrackState(dict(cfg, C=C), n, seed=3, device=DEV)       # owns a filled pt_sd_params (+ its look-up tables)
    prm = holder.params
    H, W, K = cfg["H"], cfg["W"], cfg["K"]
    nb = (L.pt_sd_ws_bytes(n, C, H, W, K) + 255) // 256 * 256
    ws = torch.empty(nb * S, dtype=torch.uint8, device=DEV)
    w = [T(p[0]) for p in probs]; f = [T(p[1]) for p in probs]; b = [T(p[2]) for p in probs]
    its = [torch.zeros(3, C, K, K, device=DEV) for _ in range(S)]
    arr = ctypes.c_void_p * S
    side = torch.cuda.Stream(device=DEV)
    cur = torch.cuda.current_stream().cuda_stream
    for aux in ([side.cuda_stream, None], [side.cuda_stream, side.cuda_stream], [side.cuda_stream, cur]):
        p_aux = (ctypes.c_void_p * 2)(*aux)
        rc = L.pt_sd_solve_batch_f32(ctypes.byref(prm), S, arr(*[x.data_ptr() for x in w]), arr(*[x.data_ptr() for x in f]),
                                     f[0].stride(0), arr(*[x.data_ptr() for x in b]), None, n, C, H, W, K, 2,
                                     arr(*[x.data_ptr() for x in its]), None, arr(*[ws.data_ptr() + s * nb for s in range(S)]), nb, cur,
                                     p_aux, 2)
        assert rc == _lib.PT_ERR_SHAPE, (aux, rc)
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0.0 for x in its)           # nothing ran


def test_atom_cg_folded_partial_sum_knob():
    """The round-5 experiment kept behind PT_ACG_FOLD=1 (partial sums folded into the forward kernel: measured slower, off by default)
    computes the same update: run in a child process with the knob on, against the BASELINE configs[0]-size golden."""
    import subprocess
    import sys
    code = ("import os,sys,numpy as np,torch;sys.path.insert(0,'tests');sys.path.insert(0,'.');"
            "import test_gpu_parity as G;from conftest import load_golden;from pytracking_amd import synth;"
            "g=load_golden('atom_cg_cfg1_n250');x0,s,y,sw=synth.atom_problem(int(g['seed']),int(g['n']));"
            "o=G._atom_run(x0,s,y,sw,5,False,1).cpu().numpy();print('ERR',float(np.abs(o-g['x_out']).max()))")
    env = dict(os.environ, PT_ACG_FOLD="1")
    res = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    err = float([ln for ln in res.stdout.splitlines() if ln.startswith("ERR")][0].split()[1])
    assert err < 5e-6, err
