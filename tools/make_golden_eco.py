"""TEST INFRASTRUCTURE ONLY -- tests/golden/eco_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_eco.py
ECO's Fourier-domain per-frame path (pytracking/tracker/eco/eco.py:181-245).  The installed torch has neither torch.rfft nor torch.irfft:
tests/eco_shim.py (two functions on torch.fft, checked against a float64 dense DFT by tests/test_eco_cpu.py) is installed into `torch`
BEFORE the reference is imported, so every golden is pinned to the unmodified reference plus that shim.  The reference's methods are called
unbound on a plain namespace that carries the attributes they read; no tracker is constructed.
  eco_sample   ECO.project_sample + ECO.preprocess_sample (+ fourier.shift_fs) for tests/eco_cases.SAMPLE_CASES
  eco_ops      ECO.apply_filter, ECO.localize_target's score map with dcf.max2d, fourier.shift_fs + ECO.update_memory
  eco_reg      dcf.get_reg_filter at the default parameter sets
Per case: the reference's fp32 output `out`, the same call in float64 `want_f64` (both at eco_cases.sample_positions when the output is
large), `ref_fp32_err` = max |fp32 - float64| over the WHOLE output and `max_abs` = max |float64|.  Inputs come from seeds
(pytracking_amd.synth): only outputs are stored.  fourier.shift_fs evaluates its phases in fp32 whatever the input's dtype, so the
float64 run of a shifted case carries that rounding; the tests compare with the float64 restatement of tests/eco_cases.py."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eco_shim  # noqa: E402

eco_shim.install()

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import eco_cases as EC  # noqa: E402

OUT = os.environ.get("ECO_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
NS = types.SimpleNamespace


def T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def record(g, name, seed, f32, f64):
    """The golden entries of one output: sampled values, the full-output error of the reference's own fp32 and the float64 magnitude."""
    f32, f64 = f32.numpy().astype(np.float32), f64.numpy().astype(np.float64)
    idx = EC.sample_positions(seed, f32.size)
    g[name + "/out"], g[name + "/want_f64"] = f32.reshape(-1)[idx], f64.reshape(-1)[idx]
    g[name + "/shape"] = np.array(f32.shape)
    g[name + "/ref_fp32_err"], g[name + "/max_abs"] = np.abs(f32 - f64).max(), np.abs(f64).max()
    return float(g[name + "/ref_fp32_err"]), float(g[name + "/max_abs"])


def run_sample(case, dtype):
    from pytracking import TensorList, fourier
    from pytracking.tracker.eco.eco import ECO
    x, P, win, interp, shift = EC.sample_inputs(case)
    me = NS(projection_matrix=TensorList([None if P is None else T(P, dtype)]), window=TensorList([T(win, dtype)]),
            interp_fs=TensorList([(T(interp[0], dtype), T(interp[1], dtype))]))
    xf = ECO.preprocess_sample(me, ECO.project_sample(me, TensorList([T(x, dtype)])))
    if shift is not None:
        xf = fourier.shift_fs(xf, shift=torch.Tensor(shift))
    return xf[0]


def make_sample():
    g = {}
    for case, c in EC.SAMPLE_CASES.items():
        err, mx = record(g, case, c["seed"], run_sample(case, torch.float32), run_sample(case, torch.float64))
        print("eco_sample", case, "ref_fp32_err", err, "max |v|", mx)
    np.savez_compressed(os.path.join(OUT, "eco_sample.npz"), **g)


def run_apply(case, dtype):
    from pytracking import TensorList
    from pytracking.tracker.eco.eco import ECO
    hf, xf = EC.apply_inputs(case)
    return ECO.apply_filter(NS(filter=TensorList([T(hf, dtype)])), TensorList([T(xf, dtype)]))[0]


def run_localize(case, dtype):
    from pytracking import TensorList, dcf
    from pytracking.tracker.eco.eco import ECO
    c = EC.LOC_CASES[case]
    sfs = EC.loc_inputs(case)
    grid = torch.Tensor(c["grid"])
    me = NS(params=NS(score_fusion_strategy="sum" if c["weights"] is None else "weightedsum", scale_factors=torch.ones(c["S"])),
            fparams=TensorList([NS(translation_weight=w) for w in (c["weights"] or [1.0] * len(sfs))]), output_sz=grid, img_support_sz=grid,
            target_scale=1.0)
    _, _, scores = ECO.localize_target(me, TensorList([T(e, dtype) for e in sfs]))
    max_val, argmax = dcf.max2d(scores)
    return scores, max_val, argmax


def run_insert(case, dtype):
    from pytracking import TensorList, fourier
    from pytracking.tracker.eco.eco import ECO
    c = EC.INSERT_CASES[case]
    mem, xf = EC.insert_inputs(case)
    xf = T(xf, dtype)
    if c["shift"] is not None:
        xf = fourier.shift_fs(xf, shift=torch.Tensor(c["shift"]))
    me = NS(training_samples=TensorList([T(mem, dtype)]), update_sample_weights=lambda: [c["ind"]])
    ECO.update_memory(me, TensorList([xf]))
    return me.training_samples[0]


def make_ops():
    g = {}
    for case, c in EC.APPLY_CASES.items():
        err, mx = record(g, "apply/" + case, c["seed"], run_apply(case, torch.float32), run_apply(case, torch.float64))
        print("eco_apply", case, "ref_fp32_err", err, "max |v|", mx)
    for case, c in EC.LOC_CASES.items():
        sfs = EC.loc_inputs(case)
        g[f"loc/{case}/seed"] = EC._LOC_SEEDS[case]
        if tuple(c["grid"]) == (sfs[0].shape[2] if len(sfs) == 1 else max(e.shape[2] for e in sfs), 2 * max(e.shape[3] for e in sfs) - 1):
            print("eco_loc", case, "grid equal to the series: the reference returns 2 Wh - 2 columns there, no golden")
            continue
        s32, m32, a32 = run_localize(case, torch.float32)
        s64, m64, a64 = run_localize(case, torch.float64)
        assert torch.equal(a32, a64), case
        err, mx = record(g, f"loc/{case}/scores", c["seed"], s32, s64)
        g[f"loc/{case}/max_val"], g[f"loc/{case}/max_val_f64"], g[f"loc/{case}/argmax"] = m32.numpy(), m64.numpy(), a64.numpy()
        print("eco_loc", case, "seed", EC._LOC_SEEDS[case], "ref_fp32_err", err, "max |v|", mx, "argmax", a64.reshape(-1, 2).tolist())
    for case, c in EC.INSERT_CASES.items():
        err, mx = record(g, "insert/" + case, c["seed"], run_insert(case, torch.float32), run_insert(case, torch.float64))
        print("eco_insert", case, "ref_fp32_err", err, "max |v|", mx)
    np.savez_compressed(os.path.join(OUT, "eco_ops.npz"), **g)


REG_CASES = {      # name: (support size, base target size, use_reg_window, min, edge, power, sparsity threshold)   parameter/eco/default.py
    "shallow_240": ((240.0, 240.0), (48.0, 60.0), True, 1e-4, 10e-3, 2, 0.05),
    "deep_240": ((240.0, 240.0), (48.0, 60.0), True, 10e-4, 50e-3, 2, 0.1),
    "deep_208_tall": ((208.0, 208.0), (70.0, 30.0), True, 10e-4, 50e-3, 2, 0.1),
    "shallow_208_wide": ((208.0, 208.0), (25.0, 80.0), True, 1e-4, 10e-3, 2, 0.05),
    "off": ((240.0, 240.0), (48.0, 60.0), False, 1e-4, 10e-3, 2, 0.05),
}


def reg_params(case):
    _, _, use, lo, edge, power, thr = REG_CASES[case]
    return NS(use_reg_window=use, reg_window_min=lo, reg_window_edge=edge, reg_window_power=power, reg_sparsity_threshold=thr)


def make_reg():
    from pytracking import dcf
    g = {}
    for case, (sz, tsz, *_rest) in REG_CASES.items():
        out = dcf.get_reg_filter(torch.Tensor(sz), torch.Tensor(tsz), reg_params(case))
        g[case + "/out"], g[case + "/sz"], g[case + "/target_sz"] = out.numpy(), np.array(sz), np.array(tsz)
        g[case + "/params"] = np.array(REG_CASES[case][2:], dtype=np.float64)
        print("eco_reg", case, tuple(out.shape))
    np.savez_compressed(os.path.join(OUT, "eco_reg.npz"), **g)


if __name__ == "__main__":
    what = sys.argv[1:] or ["sample", "ops", "reg"]
    if "sample" in what:
        make_sample()
    if "ops" in what:
        make_ops()
    if "reg" in what:
        make_reg()


def run_fu(case, dtype):
    """The unmodified FilterOptim (tracker/eco/optim.py) on a case of eco_cases.FU_CASES -> the filters after every call."""
    from pytracking import TensorList
    from pytracking.tracker.eco.optim import FilterOptim
    c, d = EC.FU_CASES[case], EC.fu_inputs(case)
    tl = lambda arrs: TensorList([T(a, dtype) for a in arrs])      # noqa: E731
    prm = NS(fletcher_reeves=c.get("fr", False), standard_alpha=c.get("std_alpha", True), direction_forget_factor=c.get("forget", 0), debug=0,
             precond_learning_rate=TensorList(d["lrs"]), precond_data_param=0.3, precond_reg_param=0.15)
    opt = FilterOptim(prm, TensorList([torch.tensor(v, dtype=dtype) for v in d["reg_energy"]]))
    filt = tl(d["filters"])
    opt.register(filt, tl(d["samples"]), tl(d["yf"]), tl(d["weights"]), tl(d["regs"]))
    opt.sample_energy = tl(d["energy"])
    outs = []
    for k, it in enumerate(c["iters"]):
        opt.run(it, tl(d["new_xf"][k]) if c.get("new_xf", True) else None)
        outs.append([f.clone() for f in filt])
    return outs


def make_fu():
    g = {}
    for case, c in EC.FU_CASES.items():
        if c.get("no_ref"):
            continue
        o32, o64 = run_fu(case, torch.float32), run_fu(case, torch.float64)
        for k, (a, b) in enumerate(zip(o32, o64)):
            for blk, (x32, x64) in enumerate(zip(a, b)):
                err, mx = record(g, f"{case}/call{k}/block{blk}", c["seed"], x32, x64)
                print("eco_fu", case, "call", k, "block", blk, "ref_fp32_err", err, "max |v|", mx)
    np.savez_compressed(os.path.join(OUT, "eco_fu.npz"), **g)


if __name__ == "__main__" and (not sys.argv[1:] or "fu" in sys.argv[1:]):
    make_fu()
