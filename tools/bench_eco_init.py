"""ECO's first-frame joint optimisation on one MI355X at the default parameter set (pytracking/parameter/eco/default.py: shallow block
96 -> 16 channels on 61 x 31 coefficients, deep block 256 -> 64 on 15 x 8, n = 30 augmented samples, init_CG_iter 100 over init_GN_iter 10,
projection_reg 5e-8):
    python -B tools/bench_eco_init.py [--rounds N] [--out profiles/eco_init_bench.json] [--fused-only]
  fused   pytracking_amd.eco.joint_init, both blocks, 10 Gauss-Newton x 10 CG iterations in one call (1 + 10 x 54 launches)
  stock   the reference's own GaussNewtonCG.run(10, 10) on its FactorizedConvProblem (two autograd passes per CG iteration) on the same
          tensors and the same GPU -- needs the reference tree or its bundle; without one the tool says so and times the kernels only
Both are interleaved in ONE process: every round resets the variables and times each once, so clock and thermal drift hit them alike.
`device_ms` is event-timed around the call (for the stock run this includes the host's launch gaps: it is what the tracker waits for),
`host_ms` = the call + synchronisation on the host clock.  Medians over the rounds.  `max_abs_fused_minus_stock` compares the results."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pytracking_amd import eco  # noqa: E402

DEV = "cuda:0"
GN, CG = 10, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eco_init_bench.json"))
    ap.add_argument("--fused-only", action="store_true", help="skip the reference's run (for a kernel trace)")
    a = ap.parse_args()
    import eco_init_cases as IC
    d, preg = IC.inputs("deployed"), IC.projection_reg("deployed")
    tl = lambda k: [torch.from_numpy(v).to(DEV) for v in d[k]]      # noqa: E731
    f0, p0 = tl("filters"), tl("projs")
    filters, projs = [t.clone() for t in f0], [t.clone() for t in p0]
    fixed = [tl(k) for k in ("samples", "sw", "yf", "regs", "diag_M")]
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "gn_iter": GN, "cg_iter": CG, "projection_reg": preg,
           "blocks": [list(b[:5]) + list(b[5]) for b in IC.CASES["deployed"]["blocks"]], "launches_fused": 1 + GN * (3 + 5 * CG + 1),
           "sample_bytes": sum(int(s.numel()) * 4 for s in fixed[0])}

    def fused():
        for dst, src in zip(filters + projs, f0 + p0):
            dst.copy_(src)
        eco.joint_init(filters, projs, *fixed, d["proj_precond"], CG, GN, preg)
        return [t.clone() for t in filters + projs]

    variants = {"fused": fused}
    res["stock"] = "absent (no reference tree or bundle): the kernels only"
    try:
        from oracle import ref_harness
        if ref_harness.available() and not a.fused_only:
            ref_harness.install()
            from pytracking import TensorList
            from pytracking.libs.optimization import GaussNewtonCG
            from pytracking.tracker.eco.optim import FactorizedConvProblem
            prm = types.SimpleNamespace(precond_data_param=IC.PRECOND["dp"], precond_reg_param=IC.PRECOND["rp"],
                                        precond_proj_param=IC.PRECOND["pp"], projection_reg=preg, debug=0)
            problem = FactorizedConvProblem(TensorList(fixed[0]), TensorList(fixed[2]), TensorList(fixed[3]), TensorList([t.clone() for t in p0]),
                                            prm, TensorList([w ** 2 for w in fixed[1]]))

            def stock():
                var = TensorList([t.clone() for t in f0 + p0])
                GaussNewtonCG(problem, var).run(CG, GN)
                return [t.detach() for t in var]
            variants["stock"] = stock
            res["stock"] = "the reference's GaussNewtonCG.run on FactorizedConvProblem in stock PyTorch on the same GPU"
    except Exception as exc:      # noqa: BLE001
        res["stock"] = f"absent ({type(exc).__name__}: {exc}): the kernels only"
    outs = {k: fn() for k, fn in variants.items()}                  # warm-up and the comparison
    torch.cuda.synchronize()
    if "stock" in outs:
        res["max_abs_fused_minus_stock"] = max(float((x - y).abs().max()) for x, y in zip(outs["fused"], outs["stock"]))
        res["max_abs_stock"] = max(float(y.abs().max()) for y in outs["stock"])
    dev_t, host_t = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            host_t[k].append((time.perf_counter() - t0) * 1e3)
            dev_t[k].append(e0.elapsed_time(e1))
    for k in variants:
        res[k + "_ms"] = {"device_ms": statistics.median(dev_t[k]), "device_ms_min": min(dev_t[k]), "host_ms": statistics.median(host_t[k])}
    if "stock" in variants:
        res["stock_over_fused_device"] = res["stock_ms"]["device_ms"] / res["fused_ms"]["device_ms"]
        res["stock_over_fused_host"] = res["stock_ms"]["host_ms"] / res["fused_ms"]["host_ms"]
    res["fused_us_per_cg_iteration"] = res["fused_ms"]["device_ms"] * 1e3 / (GN * CG)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
