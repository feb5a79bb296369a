"""ECO's Fourier-domain path without a GPU: the torch.rfft / torch.irfft shim the goldens rest on (tests/eco_shim.py) against a float64
dense DFT, the float64 restatements of tests/eco_cases.py against the goldens' float64, pytracking_amd.eco's torch forms against the goldens,
the argument checks of the new entry points, the install(eco=True) round trip, and the unmodified ECO tracker on CPU tensors through
install(eco=True) -- which the installed torch cannot run otherwise (no torch.rfft).  Parity with the reference means: with the unmodified
reference running on the shim checked here."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import f64_bound  # noqa: E402
import eco_cases as EC  # noqa: E402
import eco_shim  # noqa: E402
from oracle import ref_harness  # noqa: E402
from pytracking_amd import _lib, eco  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")


def golden(name):
    return np.load(os.path.join(EC.GOLDEN, name + ".npz"))


def at_positions(a, seed):
    a = np.asarray(a)
    return a.reshape(-1)[EC.sample_positions(seed, a.size)]


T = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)      # noqa: E731


# ---- the shim ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 4), (5, 5), (6, 9), (9, 6), (1, 1), (15, 16)])
def test_shim_matches_a_float64_dense_dft(H, W):
    rng = np.random.default_rng(100 * H + W)
    a = rng.standard_normal((2, 3, H, W))
    spec = eco_shim.rfft(torch.from_numpy(a), 2).numpy()
    want = np.einsum("kh,...hw,xw->...kx", EC.phases(np.arange(H), np.arange(H), H, -1), a, EC.phases(np.arange(W // 2 + 1), np.arange(W), W, -1))
    assert spec.shape == (2, 3, H, W // 2 + 1, 2)
    assert np.abs(EC.to_c(spec) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the inverse with signal_sizes returns the signal; without it the last dimension has 2 (W / 2 + 1 - 1) points
    back = eco_shim.irfft(torch.from_numpy(spec), 2, signal_sizes=[H, W]).numpy()
    assert np.abs(back - a).max() <= 1e-12 * max(1.0, np.abs(a).max())
    if W > 1:
        assert eco_shim.irfft(torch.from_numpy(spec), 2).shape[-1] == 2 * (W // 2)
    # ... and is the normalised dense inverse of a half spectrum that no forward transform produced (zero padded columns, as sample_fs)
    Oh, Ow = H + 3, 2 * (W // 2 + 1) + 2
    z = rng.standard_normal((H, W // 2 + 1, 2))
    pad = np.zeros((Oh, Ow // 2 + 1, 2))
    pad[:H, :W // 2 + 1] = z
    got = eco_shim.irfft(torch.from_numpy(pad), 2, signal_sizes=[Oh, Ow]).numpy()
    m = np.where((np.arange(Ow // 2 + 1) == 0) | (2 * np.arange(Ow // 2 + 1) == Ow), 1.0, 2.0)
    dense = np.einsum("yk,kx,ux->yu", EC.phases(np.arange(Oh), np.arange(Oh), Oh, +1), EC.to_c(pad), EC.phases(np.arange(Ow), np.arange(Ow // 2 + 1), Ow, +1) * m).real
    assert np.abs(got - dense / (Oh * Ow)).max() <= 1e-12


# ---- restatements and torch forms against the goldens ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g_sample():
    return golden("eco_sample")


@pytest.fixture(scope="module")
def g_ops():
    return golden("eco_ops")


def check_case(g, key, seed, want, got32, shifted=False):
    """want: the float64 restatement; got32: the torch form in fp32 (both full outputs)."""
    assert tuple(g[key + "/shape"]) == want.shape
    w64 = g[key + "/want_f64"]
    # fourier.shift_fs evaluates its phases in fp32 whatever the dtype: the reference's float64 run of a shifted case carries that rounding
    tol = (8 * EC.EPS if shifted else 1e-12) * max(1.0, float(g[key + "/max_abs"]))
    assert np.abs(at_positions(want, seed) - w64).max() <= tol, key
    assert abs(np.abs(want).max() - float(g[key + "/max_abs"])) <= tol
    assert np.abs(at_positions(got32, seed) - g[key + "/out"]).max() <= 1e-4, key
    err = float(np.abs(got32.astype(np.float64) - want).max())
    assert err <= f64_bound.bound(g[key + "/ref_fp32_err"], floor=f64_bound.ulp_of_max(want)), (key, err, float(g[key + "/ref_fp32_err"]))


@pytest.mark.parametrize("case", list(EC.SAMPLE_CASES))
def test_sample_transform_restatement_and_torch_form(g_sample, case):
    c = EC.SAMPLE_CASES[case]
    x, P, win, interp, shift = EC.sample_inputs(case)
    want = EC.sample_np(x, P, win, interp, shift)
    got = eco.sample_transform_torch(T(x), T(P), T(win), (T(interp[0]), T(interp[1])), shift).numpy()
    check_case(g_sample, case, c["seed"], want, got, shifted=shift is not None)


@pytest.mark.parametrize("case", list(EC.APPLY_CASES))
def test_apply_filter_restatement_and_torch_form(g_ops, case):
    hf, xf = EC.apply_inputs(case)
    check_case(g_ops, "apply/" + case, EC.APPLY_CASES[case]["seed"], EC.apply_filter_np(hf, xf), eco.apply_filter_torch(T(hf), T(xf)).numpy())


@pytest.mark.parametrize("case", list(EC.LOC_CASES))
def test_localize_restatement_and_torch_form(g_ops, case):
    c = EC.LOC_CASES[case]
    sfs = EC.loc_inputs(case)
    assert EC._LOC_SEEDS[case] == int(g_ops[f"loc/{case}/seed"])
    scores, max_val, argmax = EC.localize_np(sfs, c["weights"], c["grid"])
    s32, m32, a32 = eco.localize_torch([T(e) for e in sfs], c["weights"], c["grid"])
    s64, m64, a64 = eco.localize_torch([T(e, torch.float64) for e in sfs], c["weights"], c["grid"])
    assert np.abs(s64.numpy() - scores).max() <= 1e-11 * np.abs(scores).max()           # the torch form computes the header's definition
    assert np.array_equal(a64.numpy(), argmax) and np.array_equal(a32.numpy(), argmax)
    key = f"loc/{case}/scores"
    if key + "/out" not in g_ops:                                                       # grid equal to the series: no reference golden
        assert tuple(c["grid"]) == (max(e.shape[2] for e in sfs), 2 * max(e.shape[3] for e in sfs) - 1)
        return
    check_case(g_ops, key, c["seed"], scores, s32.numpy())
    assert np.array_equal(g_ops[f"loc/{case}/argmax"], argmax)
    assert np.abs(g_ops[f"loc/{case}/max_val_f64"] - max_val).max() <= 1e-11 * np.abs(scores).max()
    assert np.abs(g_ops[f"loc/{case}/max_val"] - m32.numpy()).max() <= 1e-4


@pytest.mark.parametrize("case", list(EC.INSERT_CASES))
def test_insert_restatement_and_torch_form(g_ops, case):
    c = EC.INSERT_CASES[case]
    mem, xf = EC.insert_inputs(case)
    want = EC.insert_np(mem, xf, c["ind"], c["shift"])
    got = eco.insert_torch(T(mem).clone(), T(xf), c["ind"], c["shift"]).numpy()
    check_case(g_ops, "insert/" + case, c["seed"], want, got, shifted=c["shift"] is not None)
    keep = np.ones(c["n"], dtype=bool)
    keep[c["ind"]] = False
    assert np.array_equal(got[:, :, keep], mem[:, :, keep])


@pytest.mark.parametrize("case", [c for c in EC.FU_CASES if c != "deployed_shallow"])
def test_filter_update_restatement_reproduces_the_reference(case):
    """The float64 restatement of FilterOptim.run against the unmodified reference's float64 run (every call, every block), and the
    restatement's fp32 mode within the bound of its float64 (deployed_shallow: tests/test_gpu_eco.py checks it the same way)."""
    check_filter_update_restatement(case)


def check_filter_update_restatement(case):
    g = golden("eco_fu")
    c = EC.FU_CASES[case]
    outs, _ = EC.fu_run_np(case)
    for k, call in enumerate(outs):
        for b, want in enumerate(call):
            key = f"{case}/call{k}/block{b}"
            if c.get("no_ref"):
                assert key + "/out" not in g
                continue
            assert np.abs(at_positions(want, c["seed"]) - g[key + "/want_f64"]).max() <= 1e-10 * float(g[key + "/max_abs"]), key
    return outs


def test_cfft2_cifft2_round_trip_and_layout():
    for H, W in ((4, 4), (5, 6), (6, 9), (1, 1)):
        a = torch.from_numpy(np.random.default_rng(H * W).standard_normal((2, 3, H, W)))
        spec = eco.cfft2(a)
        assert spec.shape == (2, 3) + EC.series_sizes(H, W) + (2,)
        assert np.abs(EC.to_c(spec.numpy()) - EC.cfft2_np(a.numpy())).max() <= 1e-12 * max(1.0, float(a.abs().max()) * H * W)
        if H % 2 == 0:
            assert torch.equal(spec[:, :, 0], spec[:, :, -1])                           # the Nyquist row at both ends
        if H % 2 == 1:                                                                  # even H: the doubled row does not invert
            assert (eco.cifft2(spec, signal_sizes=(H, W)) - a).abs().max() <= 1e-12 * H * W


def test_get_reg_filter_reproduces_the_goldens():
    g = golden("eco_reg")
    cases = sorted({k.split("/")[0] for k in g.files})
    assert len(cases) == 5
    for case in cases:
        use, lo, edge, power, thr = g[case + "/params"]
        prm = types.SimpleNamespace(use_reg_window=bool(use), reg_window_min=float(lo), reg_window_edge=float(edge), reg_window_power=int(power),
                                    reg_sparsity_threshold=float(thr))
        out = eco.get_reg_filter(torch.Tensor(g[case + "/sz"]), torch.Tensor(g[case + "/target_sz"]), prm).numpy()
        assert out.shape == g[case + "/out"].shape, case
        assert np.abs(out - g[case + "/out"]).max() <= 1e-6 * np.abs(g[case + "/out"]).max(), case


def test_loop_cases_have_a_margin():
    """The closed loop of tests/test_gpu_eco.py compares arg-max positions and scale indices exactly: in float64 every frame's winning
    scale leads the others, and its peak every other value of its map, by 1e-4 of the score range."""
    feats = [EC.loop_features(t) for t in range(EC.LOOP["frames"])]
    margins = []

    class Ops(EC.NumpyOps):
        @staticmethod
        def localize(sfs, weights, grid):
            scores, mv, am = EC.localize_np(sfs, weights, grid)
            flat = np.sort(scores.reshape(scores.shape[0], -1), axis=1)
            best = np.sort(mv.reshape(-1))
            win = int(np.argmax(mv.reshape(-1)))
            margins.append(min(float(flat[win, -1] - flat[win, -2]), float(best[-1] - best[-2])) / float(scores.max() - scores.min()))
            return scores, mv, am
    log, mems = EC.track_frames(Ops, EC.loop_state(), feats)
    assert min(margins) >= 1e-4, margins
    assert len({e["slot"] for e in log}) >= 3 and len({e["scale_ind"] for e in log}) >= 2       # the loop moves through slots and scales
    assert all(np.abs(m).max() > 0 for m in mems) and [e["trained"] for e in log].count(True) == 2


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_do_not_launch():
    _lib.build_library()
    L = _lib.lib()
    n, one = None, ctypes.c_void_p(256)
    assert L.pt_eco_sample_f32(n, one, one, one, one, 0, 0.0, 0.0, one, 1, 3, 2, 4, 4, n) == _lib.PT_ERR_NULL
    assert L.pt_eco_sample_f32(one, one, one, one, n, 0, 0.0, 0.0, one, 1, 3, 2, 4, 4, n) == _lib.PT_ERR_NULL         # one factor only
    assert L.pt_eco_sample_f32(one, one, one, one, one, 0, 0.0, 0.0, one, 0, 3, 2, 4, 4, n) == _lib.PT_ERR_SHAPE
    assert L.pt_eco_sample_f32(one, n, one, one, one, 0, 0.0, 0.0, one, 1, 3, 2, 4, 4, n) == _lib.PT_ERR_SHAPE          # no projection, c != Cin
    assert L.pt_eco_sample_f32(one, one, one, one, one, 0, 0.0, 0.0, one, 1, 3, 2, 65, 4, n) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_eco_shift_f32(one, 0.1, 0.1, n, 1, 2, 5, 3, n) == _lib.PT_ERR_NULL
    assert L.pt_eco_shift_f32(one, 0.1, 0.1, one, 1, 2, 4, 3, n) == _lib.PT_ERR_SHAPE                                   # even Hf
    assert L.pt_eco_apply_filter_f32(one, n, one, 1, 2, 5, 3, n) == _lib.PT_ERR_NULL
    assert L.pt_eco_apply_filter_f32(one, one, one, 1, 0, 5, 3, n) == _lib.PT_ERR_SHAPE
    assert L.pt_eco_insert_f32(n, 0, 0.0, 0.0, one, 2, 5, 3, 4, 0, n) == _lib.PT_ERR_NULL
    assert L.pt_eco_insert_f32(one, 0, 0.0, 0.0, one, 2, 5, 3, 4, 4, n) == _lib.PT_ERR_SHAPE                            # slot == n
    assert L.pt_eco_insert_f32(one, 0, 0.0, 0.0, one, 2, 5, 3, 4, -1, n) == _lib.PT_ERR_SHAPE
    blk = (_lib.EcoFuBlock * 1)()
    for name in ("samples", "weights", "yf", "reg_filter", "sample_energy", "x", "p", "r_prev", "state"):
        setattr(blk[0], name, 256)
    blk[0].Hf, blk[0].Wh, blk[0].c, blk[0].n, blk[0].Rh, blk[0].Rw = 9, 5, 4, 6, 5, 5
    need = L.pt_eco_filter_update_ws_bytes(blk, 1)
    assert need >= 4 * (9 * 5 * 4 * 9) and L.pt_eco_filter_update_ws_bytes(blk, 5) == 0
    fu = lambda *a: L.pt_eco_filter_update_f32(*a)      # noqa: E731
    assert fu(None, 1, 5, 0, 1, 0.0, 0.3, 0.15, one, 1 << 30, n) == _lib.PT_ERR_NULL
    assert fu(blk, 0, 5, 0, 1, 0.0, 0.3, 0.15, one, 1 << 30, n) == _lib.PT_ERR_SHAPE
    assert fu(blk, 1, 63, 0, 1, 0.0, 0.3, 0.15, one, 1 << 30, n) == _lib.PT_ERR_UNSUPPORTED
    assert fu(blk, 1, 5, 0, 1, 0.0, 0.3, 0.15, one, 16, n) == _lib.PT_ERR_WORKSPACE
    assert fu(blk, 1, 0, 0, 1, 0.0, 0.3, 0.15, one, 16, n) == 0                          # num_iter == 0 returns at once
    blk[0].Hf = 3                                                                        # 5 x 5 against Hf = 3: the clipped padding does not give
    assert fu(blk, 1, 5, 0, 1, 0.0, 0.3, 0.15, one, 1 << 30, n) == _lib.PT_ERR_UNSUPPORTED   # the filter's size back (the reference raises)
    blk[0].Hf, blk[0].c = 9, 65
    assert fu(blk, 1, 5, 0, 1, 0.0, 0.3, 0.15, one, 1 << 30, n) == _lib.PT_ERR_UNSUPPORTED and L.pt_eco_filter_update_ws_bytes(blk, 1) == 0
    blk[0].c, blk[0].state = 4, None
    assert fu(blk, 1, 5, 0, 1, 0.0, 0.3, 0.15, one, 1 << 30, n) == _lib.PT_ERR_NULL
    assert L.pt_eco_localize_ws_bytes(5, 31, 240, 240) >= 8 * (5 * 240 * 31) + 16 * 480
    assert L.pt_eco_localize_ws_bytes(5, 65, 240, 240) == 0 and L.pt_eco_localize_ws_bytes(5, 31, 1025, 240) == 0
    ptrs, hf, wh = (ctypes.c_void_p * 2)(256, 256), (ctypes.c_int * 2)(9, 7), (ctypes.c_int * 2)(5, 4)
    big = 1 << 30
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 2, 1, 12, 10, one, one, one, n, big, n) == _lib.PT_ERR_NULL
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 0, 1, 12, 10, one, one, one, one, big, n) == _lib.PT_ERR_SHAPE
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 5, 1, 12, 10, one, one, one, one, big, n) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 2, 1, 8, 10, one, one, one, one, big, n) == _lib.PT_ERR_SHAPE          # grid below the series
    assert L.pt_eco_localize_f32(ptrs, (ctypes.c_int * 2)(7, 9), wh, None, 2, 1, 12, 10, one, one, one, one, big, n) == _lib.PT_ERR_SHAPE   # largest not first
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 2, 1, 12, 2000, one, one, one, one, big, n) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 2, 1, 12, 10, one, one, one, one, 16, n) == _lib.PT_ERR_WORKSPACE
    assert L.pt_eco_localize_f32(ptrs, hf, wh, None, 2, 1, 12, 10, one, one, one, ctypes.c_void_p(260), big, n) == _lib.PT_ERR_WORKSPACE


def test_product_path_refuses_cpu_tensors():
    x = torch.zeros(1, 2, 5, 3, 2)
    for call in (lambda: eco.sample_transform(torch.zeros(1, 2, 4, 4), None, None, None), lambda: eco.apply_filter(x, x),
                 lambda: eco.shift_fs(x, (0.1, 0.2)), lambda: eco.localize([x[:, :1]], None, (8, 8)),
                 lambda: eco.insert(torch.zeros(5, 3, 4, 2, 2), x, 0)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


# ---- install(eco=True) ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def amd():
    ref_harness.install()
    import pytracking.tracker.eco.eco  # noqa: F401
    import pytracking.tracker.eco.optim  # noqa: F401
    from pytracking_amd import install as amd
    amd.install(eco=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_reference
def test_install_eco_round_trip_and_default_set(amd):
    import test_install_ledger as TL
    before = TL.snapshot()
    amd.install()
    default = TL.changed(before, TL.snapshot())
    with open(TL.REBOUND) as fh:
        assert default == json.load(fh)                                                 # a default install() rebinds exactly the pinned set
    amd.uninstall()
    assert TL.changed(before, TL.snapshot()) == []
    amd.install(eco=True)
    extra = sorted(set(TL.changed(before, TL.snapshot())) - set(default))
    assert extra == sorted(["pytracking.libs.fourier.cfft2", "pytracking.libs.fourier.cifft2", "pytracking.libs.fourier.shift_fs",
                            "pytracking.libs.dcf.get_reg_filter", "pytracking.tracker.eco.optim.FilterOptim.run"]
                           + ["pytracking.tracker.eco.eco.ECO." + m for m in (
                                "preprocess_sample", "extract_fourier_sample", "apply_filter", "localize_target", "update_memory")])
    amd.uninstall()
    assert TL.changed(before, TL.snapshot()) == []


@needs_reference
def test_unmodified_eco_runs_on_cpu_through_install(amd, monkeypatch):
    """initialize() + 3 x track() of the reference ECO on CPU tensors.  The installed torch has no torch.rfft (oracle/ref_harness.py:132-143 installs a stand-in
    of its own for ATOM's localisation, the same two functions as tests/eco_shim.py: it is taken away for the test), so without install(eco=True) this raises in ECO.initialize."""
    import eco_tracker as ET
    monkeypatch.delattr(torch, "rfft", raising=False)
    monkeypatch.delattr(torch, "irfft", raising=False)
    with pytest.raises(AttributeError, match="rfft"):
        ET.run(n_frames=0)
    amd.install(eco=True)
    amd.stats.clear()
    boxes, scores, tracker = ET.run(n_frames=3)
    stats = dict(amd.stats)
    assert boxes.shape == (3, 4) and np.isfinite(boxes).all() and np.isfinite(scores).all() and (scores > 0).all()
    assert [tuple(r.shape[-2:]) for r in tracker.reg_filter] == [(5, 5), (3, 3)]
    # CPU tensors: every dispatcher hands the call to the reference's own code; the joint Gauss-Newton is ECO's problem class, which the
    # ATOM dispatcher declines
    assert not [k for k in stats if k.endswith(".fast")], stats
    for name in ("cfft2", "shift_fs", "FilterOptim.run", "ECO.preprocess_sample", "ECO.extract_fourier_sample", "ECO.apply_filter",
                 "ECO.localize_target", "ECO.update_memory"):
        assert stats.get(name + ".reference", 0) >= 1, (name, stats)
    # (eco.py:9 imports GaussNewtonCG by name: a tracker module imported before install() holds the reference class itself)
    import pytracking.libs.optimization as po
    from pytracking_amd import optimization as ours
    amd.stats.clear()
    opt = po.GaussNewtonCG(tracker.joint_problem, tracker.filter.concat(tracker.projection_matrix))
    assert not isinstance(opt, ours.GaussNewtonCG) and isinstance(opt, amd.original(po, "GaussNewtonCG"))
    assert dict(amd.stats) == {"GaussNewtonCG.reference": 1}
