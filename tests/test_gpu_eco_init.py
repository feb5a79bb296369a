"""ECO's first-frame joint Gauss-Newton optimisation on the kernels (pytracking_amd.eco.joint_init, eco_init.hip) against the float64
restatement of tests/eco_init_cases.py, which tests/test_eco_init_cpu.py holds to the unmodified reference's float64 run.  The bound is the
project's (tests/f64_bound.py): FACTOR x the larger of the reference's own fp32 error on the case (the golden's `ref_fp32_err`: autograd
GaussNewtonCG in fp32 on CPU) and one fp32 ulp of the largest value.  With ECO_INIT_F64_OUT set the table of ratios is written
(profiles/eco_init_f64.txt)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import eco_cases as EC  # noqa: E402
import eco_init_cases as IC  # noqa: E402
import f64_bound  # noqa: E402
from f64_bound import host, needs_bundle  # noqa: E402
from oracle import ref_harness  # noqa: E402
from pytracking_amd import eco  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE = f64_bound.Table("ECO_INIT_F64_OUT",
                        "ECO first-frame joint optimisation on gfx950: max |out - float64| per output, as a multiple of max(ref_fp32_err, 2^-23 max |want|)\n"
                        f"(bound: {f64_bound.FACTOR}); ref_fp32_err: the unmodified reference's own fp32 error (golden) or, marked *, the restatement's fp32 mode")
dev = functools.partial(f64_bound.dev, device=DEV, dtype=torch.float32)


@pytest.fixture(scope="module")
def g_init():
    return np.load(IC.GOLDEN)


def on_device(case, d=None, preg=None):
    """The case on the kernels -> [hf per block] + [P per block] (the tensors the call updated in place)."""
    c, d = IC.CASES[case], d or IC.inputs(case)
    tl = lambda k: [dev(a) for a in d[k]]      # noqa: E731
    filters, projs = tl("filters"), tl("projs")
    out = eco.joint_init(filters, projs, tl("samples"), tl("sw"), tl("yf"), tl("regs"), tl("diag_M"), d["proj_precond"], c["cg"], c["gn"],
                         IC.projection_reg(case) if preg is None else preg)
    assert out[0][0].data_ptr() == filters[0].data_ptr() and out[1][0].data_ptr() == projs[0].data_ptr()       # updated in place
    torch.cuda.synchronize()
    return filters + projs


@pytest.mark.parametrize("case", [k for k, c in IC.CASES.items() if not c.get("no_ref")])
def test_joint_init(g_init, case):
    c = IC.CASES[case]
    outs = on_device(case)
    for key, x, want in zip(IC.keys(case), outs, IC.run_np(case)):
        got = host(x)
        assert got.shape == want.shape
        f64_bound.held("joint_init " + key, got, want, g_init[key + "/ref_fp32_err"], floor=f64_bound.ulp_of_max, table=TABLE)
        idx = EC.sample_positions(c["seed"], got.size)
        assert np.abs(got.reshape(-1)[idx] - g_init[key + "/out"]).max() <= 1e-4, key
    assert all(torch.equal(a, b) for a, b in zip(on_device(case), outs))                  # the same call twice: the same bits


@pytest.mark.parametrize("case", ["zero_gn", "zero_cg"])
def test_zero_iterations_touch_nothing(case):
    d = IC.inputs(case)
    for x, src in zip(on_device(case), d["filters"] + d["projs"]):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), src.view(np.uint32))


def test_strided_projection_is_updated_in_place():
    """The tracker's projection matrix (eco.py:113, the clone of a column slice) keeps the slice's strides: the same bits as from a dense one."""
    c, d = IC.CASES["two_blocks"], IC.inputs("two_blocks")
    dense = on_device("two_blocks")
    tl = lambda k: [dev(a) for a in d[k]]      # noqa: E731
    filters, wide = tl("filters"), [torch.zeros(p.shape[0], p.shape[1] + 3, device=DEV) for p in d["projs"]]
    projs = [w[:, :p.shape[1]] for w, p in zip(wide, d["projs"])]
    for v, p in zip(projs, d["projs"]):
        v.copy_(dev(p))
    assert not projs[0].is_contiguous()
    eco.joint_init(filters, projs, tl("samples"), tl("sw"), tl("yf"), tl("regs"), tl("diag_M"), d["proj_precond"], c["cg"], c["gn"],
                   IC.projection_reg("two_blocks"))
    assert all(torch.equal(a, b) for a, b in zip(filters + projs, dense)) and not any(w[:, -3:].any() for w in wide)


def test_exact_zero_rho_leaves_the_variables():
    """Block 0 has all-zero samples and label and a zero filter, projection_reg is 0: J^T f0 of that block is exactly 0, rho is exactly 0 at
    the top of the first CG iteration of EVERY Gauss-Newton iteration, the check is joint, and (include/pt_hot.h) the variables of BOTH blocks
    stay as they stand -- bit for bit, nothing NaN or Inf -- where the reference raises on `x += None`.  The restatement does the same."""
    c, d = IC.CASES["two_blocks"], dict(IC.inputs("two_blocks"))
    for k in ("samples", "yf", "filters"):
        d[k] = [np.zeros_like(d[k][0]), d[k][1]]
    outs = on_device("two_blocks", d, preg=0.0)
    for x, src in zip(outs, d["filters"] + d["projs"]):
        assert torch.isfinite(x).all() and np.array_equal(x.cpu().numpy().view(np.uint32), src.view(np.uint32))
    opt = IC.JointGNNp(d["filters"], d["projs"], d["samples"], d["sw"], d["yf"], d["regs"], 0.0, d["diag_M"], d["proj_precond"])
    want = opt.run(c["cg"], c["gn"])
    assert opt.exits == c["gn"] and all(np.array_equal(w, src.astype(np.float64)) for w, src in zip(want, d["filters"] + d["projs"]))
    # ... and with only the zero block in the call nothing is NaN either when projection_reg > 0 moves its projection matrix
    one = {k: v[:1] for k, v in d.items()}
    tl = lambda k: [dev(a) for a in one[k]]      # noqa: E731
    filters, projs = tl("filters"), tl("projs")
    eco.joint_init(filters, projs, tl("samples"), tl("sw"), tl("yf"), tl("regs"), tl("diag_M"), one["proj_precond"], 1, 1, 1e-4)
    torch.cuda.synchronize()
    assert torch.isfinite(filters[0]).all() and torch.isfinite(projs[0]).all() and not filters[0].any()


def replayed(fn):
    """Warm-up on a side stream, capture, replay: what the captured graph computes (the GraphOps._replayed pattern of tests/test_gpu_eco.py)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                                            # warm-up: kernels loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()
    torch.cuda.synchronize()
    return out


def test_joint_init_is_graph_capturable():
    eager = on_device("two_blocks")
    c, d = IC.CASES["two_blocks"], IC.inputs("two_blocks")
    tl = lambda k: [dev(a) for a in d[k]]      # noqa: E731
    f0, p0 = tl("filters"), tl("projs")
    filters, projs = [f.clone() for f in f0], [p.clone() for p in p0]
    fixed = [tl(k) for k in ("samples", "sw", "yf", "regs", "diag_M")]

    def call():
        for dst, src in zip(filters + projs, f0 + p0):
            dst.copy_(src)
        eco.joint_init(filters, projs, *fixed, d["proj_precond"], c["cg"], c["gn"], IC.projection_reg("two_blocks"))
        return [t.clone() for t in filters + projs]
    captured = replayed(call)
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))


@needs_bundle
def test_unmodified_eco_initialises_on_the_kernels(monkeypatch):
    """initialize() + 3 x track() of the reference ECO on the device under install(eco=True, eco_init=True): the joint optimisation takes the
    kernels once, and at that call the filter and the projection matrix agree within the bound with the float64 restatement started from the
    same inputs (the tracker's own preconditioner), the restatement's fp32 mode being the yardstick."""
    import eco_tracker as ET
    ref_harness.install()
    from pytracking_amd import install as amd
    real, ratios = eco.joint_init, []

    def checked(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond, num_cg_iter, num_gn_iter, projection_reg):
        pre = [[host(t) for t in ts] for ts in (filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M)]
        runs = [IC.JointGNNp(*pre[:6], projection_reg, pre[6], proj_precond, single=single).run(num_cg_iter, num_gn_iter) for single in (False, True)]
        out = real(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond, num_cg_iter, num_gn_iter, projection_reg)
        for q, (x, w, r) in enumerate(zip(list(filters) + list(projections), *runs)):
            assert not np.array_equal(host(x), (pre[0] + pre[1])[q])                        # the tracker's tensors moved
            err = f64_bound.held(f"tracker joint_init output {q}", host(x), w, np.abs(r - w).max(), floor=f64_bound.ulp_of_max, table=TABLE, star=True)[""]
            ratios.append(err / max(float(np.abs(r - w).max()), f64_bound.ulp_of_max(w)))
        return out
    monkeypatch.setattr(eco, "joint_init", checked)
    amd.install(eco=True, eco_init=True)
    amd.stats.clear()
    try:
        boxes, scores, tracker = ET.run(device=DEV, n_frames=3)
        stats = dict(amd.stats)
    finally:
        amd.uninstall()
    print("\ninstall(eco=True, eco_init=True):", stats, [f"{v:.2f}" for v in ratios])
    assert stats.get("ECO.GaussNewtonCG.run.fast") == 1 and "ECO.GaussNewtonCG.run.reference" not in stats, stats
    assert len(ratios) == 4                                                                # two blocks: two filters, two projection matrices
    assert np.isfinite(boxes).all() and np.isfinite(scores).all() and tracker.filter[0].is_cuda
    assert tracker.joint_optimizer.residuals.numel() == 0 and stats.get("FilterOptim.run.fast", 0) >= 1
