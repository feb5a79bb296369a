"""TEST INFRASTRUCTURE ONLY -- tests/golden/eco_init.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_eco_init.py [case ...]
ECO's first-frame joint optimisation (pytracking/tracker/eco/eco.py:152-158): the reference's FactorizedConvProblem (tracker/eco/optim.py)
is constructed as ECO.initialize constructs it and GaussNewtonCG (libs/optimization.py, two autograd passes per application of J^T J) runs
`run(num_cg_iter, num_gn_iter)` on it, in fp32 and in float64.  tests/eco_shim.py is installed first, on the pattern of
tools/make_golden_eco.py (nothing on this path transforms, so it is not exercised).  Per case, call and block, for the filter (`hf`) and the
projection matrix (`P`): the fp32 output `out` and the float64 output `want_f64` at eco_cases.sample_positions, `ref_fp32_err` =
max |fp32 - float64| over the WHOLE output and `max_abs` = max |float64|.  Inputs come from seeds (tests/eco_init_cases.py): only outputs
are stored.  The preconditioner is the constructor's own in either precision."""
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
import eco_init_cases as IC  # noqa: E402

OUT = os.environ.get("ECO_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
NS = types.SimpleNamespace


def T(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)           # a copy: the optimiser updates its variable in place, the inputs are cached


def run_reference(case, dtype):
    """-> [hf per block] + [P per block] after GaussNewtonCG.run."""
    from pytracking import TensorList
    from pytracking.libs.optimization import GaussNewtonCG
    from pytracking.tracker.eco.optim import FactorizedConvProblem
    c, d = IC.CASES[case], IC.inputs(case)
    tl = lambda arrs: TensorList([T(a, dtype) for a in arrs])      # noqa: E731
    prm = NS(precond_data_param=IC.PRECOND["dp"], precond_reg_param=IC.PRECOND["rp"], precond_proj_param=IC.PRECOND["pp"],
             projection_reg=IC.projection_reg(case), debug=0)
    filt, proj = tl(d["filters"]), tl(d["projs"])
    # the tracker hands over the weights (ones(1) / n, eco.py:133); the problem takes their square root itself
    problem = FactorizedConvProblem(tl(d["samples"]), tl(d["yf"]), tl(d["regs"]), proj, prm, TensorList([T(w, dtype) ** 2 for w in d["sw"]]))
    if dtype == torch.float64:                                       # the restatement's constructor arithmetic is the reference's
        for b, dm in enumerate(d["diag_M"]):
            assert np.abs(problem.diag_M[b].numpy().reshape(dm.shape) - dm).max() <= 2 * EC.EPS * np.abs(dm).max(), (case, b)
            assert abs(float(problem.diag_M[len(d["diag_M"]) + b]) - d["proj_precond"][b]) <= 2 * EC.EPS * d["proj_precond"][b], (case, b)
    opt = GaussNewtonCG(problem, filt.concat(proj), debug=False)
    opt.run(c["cg"], c["gn"])
    return [t.detach().clone() for t in list(filt) + list(proj)]


def record(g, name, seed, f32, f64):
    f32, f64 = f32.numpy().astype(np.float32), f64.numpy().astype(np.float64)
    idx = EC.sample_positions(seed, f32.size)
    g[name + "/out"], g[name + "/want_f64"] = f32.reshape(-1)[idx], f64.reshape(-1)[idx]
    g[name + "/shape"] = np.array(f32.shape)
    g[name + "/ref_fp32_err"], g[name + "/max_abs"] = np.abs(f32 - f64).max(), np.abs(f64).max()
    return float(g[name + "/ref_fp32_err"]), float(g[name + "/max_abs"])


def main(cases):
    path = os.path.join(OUT, "eco_init.npz")
    g = dict(np.load(path)) if cases and os.path.exists(path) else {}
    for case in cases or list(IC.CASES):
        c = IC.CASES[case]
        if c.get("no_ref"):
            continue
        o32, o64 = run_reference(case, torch.float32), run_reference(case, torch.float64)
        for key, x32, x64 in zip(IC.keys(case), o32, o64):
            err, mx = record(g, key, c["seed"], x32, x64)
            print("eco_init", key, "ref_fp32_err", err, "max |v|", mx)
    np.savez_compressed(path, **g)


if __name__ == "__main__":
    main(sys.argv[1:])
