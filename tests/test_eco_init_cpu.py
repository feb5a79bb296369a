"""ECO's first-frame joint Gauss-Newton optimisation without a GPU: the float64 restatement of tests/eco_init_cases.py against the unmodified
reference's float64 run (tests/golden/eco_init.npz), the transposes of its analytic Jacobian, pytracking_amd.eco.joint_init_torch against
both, the argument checks of the new entry points, and the install(eco=True, eco_init=True) round trip."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import f64_bound  # noqa: E402
import eco_cases as EC  # noqa: E402
import eco_init_cases as IC  # noqa: E402
from oracle import ref_harness  # noqa: E402
from pytracking_amd import _lib, eco  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
WITH_GOLDEN = [k for k, c in IC.CASES.items() if not c.get("no_ref")]


@pytest.fixture(scope="module")
def g_init():
    return np.load(IC.GOLDEN)


T = lambda a, dt: torch.from_numpy(np.array(a)).to(dt)      # noqa: E731


@pytest.mark.parametrize("case", WITH_GOLDEN)
def test_restatement_is_the_references_float64(g_init, case):
    """The analytic J^T J, the detached left extension and the per-block CG scalars reproduce the autograd run."""
    c = IC.CASES[case]
    for key, out in zip(IC.keys(case), IC.run_np(case)):
        assert tuple(g_init[key + "/shape"]) == out.shape
        got = out.reshape(-1)[EC.sample_positions(c["seed"], out.size)]
        assert np.abs(got - g_init[key + "/want_f64"]).max() <= 1e-10 * float(g_init[key + "/max_abs"]), key


def dot(a, b):
    return float((a.real * b.real).sum() + (a.imag * b.imag).sum())


@pytest.mark.parametrize("case", ["tiny", "two_blocks", "reg_1x1", "reg_7x1", "reg_clipped", "cin_70", "uniform_n30"])
def test_transposes(case):
    """<J u, g> == <u, J^T g> in float64 on random vectors, for the data, the regularisation and the projection part on its own."""
    d = IC.inputs(case)
    opt = IC.JointGNNp(d["filters"], d["projs"], d["samples"], d["sw"], d["yf"], d["regs"], IC.projection_reg(case))
    rng = np.random.default_rng(11)
    cplx = lambda shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)      # noqa: E731
    for b in range(len(opt.h)):
        if not np.abs(opt.h[b]).any():
            opt.h[b] = cplx(opt.h[b].shape)
        dh, dP = cplx(opt.h[b].shape), rng.standard_normal(opt.P[b].shape)
        Ju = opt.J(b, dh, dP)
        g = (cplx(Ju[0].shape), rng.standard_normal(Ju[1].shape), rng.standard_normal(Ju[2].shape))
        for part in range(3):
            only = [gp if q == part else np.zeros_like(gp) for q, gp in enumerate(g)]
            gh, gP = opt.JT(b, *only)
            lhs, rhs = dot(Ju[part], only[part]), dot(dh, gh) + dot(dP, gP)
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-30), (case, b, part, lhs, rhs)
        # the detached left extension is in the residual, not in J: the regulariser of J is the correlation of [0, dh]
        p2 = opt.pads(b)[1]
        if p2 > 0:
            assert np.abs(opt.reg_fwd(b, dh, True) - opt.reg_fwd(b, dh, False)).max() > 0


def torch_run(case, dtype):
    c, d = IC.CASES[case], IC.inputs(case)
    tl = lambda k: [T(a, dtype) for a in d[k]]      # noqa: E731
    filters, projs = tl("filters"), tl("projs")
    if dtype == torch.float64:                        # float64: the preconditioner in float64, as the restatement's
        pre = [IC.preconditioner(s, p, y, r, IC.projection_reg(case), **IC.PRECOND) for s, p, y, r in zip(d["samples"], d["projs"], d["yf"], d["regs"])]
        diag, pc = [torch.from_numpy(v) for v, _ in pre], [v for _, v in pre]
    else:
        diag, pc = tl("diag_M"), d["proj_precond"]
    eco.joint_init_torch(filters, projs, tl("samples"), tl("sw"), tl("yf"), tl("regs"), diag, pc, c["cg"], c["gn"], IC.projection_reg(case))
    return [t.double().numpy() for t in filters + projs]


@pytest.mark.parametrize("case", list(IC.CASES))
def test_torch_form(g_init, case):
    want = IC.run_np(case)
    for key, got, w in zip(IC.keys(case), torch_run(case, torch.float64), want):
        assert np.abs(got - w).max() <= 1e-10 * max(np.abs(w).max(), 1e-30), key
    for key, got, w in zip(IC.keys(case), torch_run(case, torch.float32), want):
        ref_err = g_init[key + "/ref_fp32_err"] if key + "/ref_fp32_err" in g_init else 0.0
        bound = f64_bound.bound(ref_err, floor=f64_bound.ulp_of_max(w))
        err = np.abs(got - w).max()
        print(f"\n{key}: torch fp32 {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (key, err, bound)


def test_zero_iterations_touch_nothing_in_the_torch_form():
    for case in ("zero_gn", "zero_cg"):
        d = IC.inputs(case)
        for got, src in zip(torch_run(case, torch.float32), d["filters"] + d["projs"]):
            assert np.array_equal(got, src.astype(np.float64))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def init_block():
    blk = (_lib.EcoInitBlock * 1)()
    for name in ("samples", "weights_sqrt", "yf", "reg_filter", "diag_M", "hf", "proj"):
        setattr(blk[0], name, 256)
    blk[0].Hf, blk[0].Wh, blk[0].Cin, blk[0].c, blk[0].n, blk[0].nw, blk[0].Rh, blk[0].Rw = 9, 5, 6, 4, 6, 1, 5, 5
    blk[0].proj_precond = 1.0
    return blk


def test_argument_checks_do_not_launch():
    _lib.build_library()
    L = _lib.lib()
    n, one, big = None, ctypes.c_void_p(256), 1 << 30
    run = lambda *a: L.pt_eco_joint_init_f32(*a)      # noqa: E731
    blk = init_block()
    need = L.pt_eco_joint_init_ws_bytes(blk, 1)
    assert need >= 4 * (2 * 45 * 6 + 4 * 2 * 45 * 4 + 4 * 24)
    assert run(None, 1, 2, 3, 1e-4, one, big, n) == _lib.PT_ERR_NULL
    assert run(blk, 1, 2, 3, 1e-4, n, big, n) == _lib.PT_ERR_NULL
    assert run(blk, 0, 2, 3, 1e-4, one, big, n) == _lib.PT_ERR_SHAPE
    assert run(blk, 1, -1, 3, 1e-4, one, big, n) == _lib.PT_ERR_SHAPE and run(blk, 1, 2, -1, 1e-4, one, big, n) == _lib.PT_ERR_SHAPE
    assert run(blk, 5, 2, 3, 1e-4, one, big, n) == _lib.PT_ERR_UNSUPPORTED
    assert run(blk, 1, 33, 3, 1e-4, one, big, n) == _lib.PT_ERR_UNSUPPORTED and run(blk, 1, 2, 63, 1e-4, one, big, n) == _lib.PT_ERR_UNSUPPORTED
    assert run(blk, 1, 2, 3, 1e-4, one, 16, n) == _lib.PT_ERR_WORKSPACE
    assert run(blk, 1, 2, 3, 1e-4, ctypes.c_void_p(260), big, n) == _lib.PT_ERR_WORKSPACE
    assert run(blk, 1, 0, 3, 1e-4, n, 0, n) == 0 and run(blk, 1, 2, 0, 1e-4, n, 0, n) == 0          # zero iterations return at once
    for name in ("samples", "weights_sqrt", "yf", "reg_filter", "diag_M", "hf", "proj"):
        blk = init_block()
        setattr(blk[0], name, None)
        assert run(blk, 1, 2, 3, 1e-4, one, big, n) == _lib.PT_ERR_NULL, name
    for name, bad in (("Hf", 0), ("Cin", 0), ("c", -1), ("n", 0), ("Rw", 0), ("nw", 2), ("nw", 0)):
        blk = init_block()
        setattr(blk[0], name, bad)
        assert run(blk, 1, 2, 3, 1e-4, one, big, n) == _lib.PT_ERR_SHAPE, name


@pytest.mark.parametrize("name,inside,outside", [("Cin", 512, 513), ("c", 64, 65), ("n", 64, 65), ("Rh", 15, 16), ("Rw", 15, 16)])
def test_limits(name, inside, outside):
    _lib.build_library()
    L = _lib.lib()
    blk = init_block()
    setattr(blk[0], name, inside)
    blk[0].nw = 1
    assert L.pt_eco_joint_init_ws_bytes(blk, 1) > 0
    setattr(blk[0], name, outside)
    assert L.pt_eco_joint_init_ws_bytes(blk, 1) == 0
    assert L.pt_eco_joint_init_f32(blk, 1, 2, 3, 1e-4, ctypes.c_void_p(256), 1 << 30, None) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_eco_joint_init_ws_bytes(init_block(), _lib.PT_ECO_MAX_BLOCKS + 1) == 0


def test_product_path_refuses_cpu_tensors_and_source_is_listed():
    d = IC.inputs("tiny")
    tl = lambda k: [T(a, torch.float32) for a in d[k]]      # noqa: E731
    with pytest.raises(RuntimeError, match="MI355X"):
        eco.joint_init(tl("filters"), tl("projs"), tl("samples"), tl("sw"), tl("yf"), tl("regs"), tl("diag_M"), d["proj_precond"], 3, 1, 1e-4)
    assert not eco.covered_joint_init(tl("filters"), tl("projs"), tl("samples"), tl("sw"), tl("yf"), tl("regs"), tl("diag_M"), d["proj_precond"], 3, 1)
    assert "eco_init.hip" in _lib.SOURCES
    assert {"pt_eco_joint_init_ws_bytes", "pt_eco_joint_init_f32"} <= set(_lib.EXPORTS)


# ---- install(eco=True, eco_init=True) --------------------------------------------------------------------------------------------------
@pytest.fixture()
def amd():
    ref_harness.install()
    import pytracking.tracker.eco.eco  # noqa: F401
    import pytracking.tracker.eco.optim  # noqa: F401
    from pytracking_amd import install as amd
    amd.install(eco=True, eco_init=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_reference
def test_install_eco_init_rebinds_one_name(amd):
    import test_install_ledger as TL
    import pytracking.libs.optimization as po
    import pytracking.tracker.eco.eco as emod
    before = TL.snapshot()
    amd.install(eco=True)
    eco_set = TL.changed(before, TL.snapshot())
    amd.uninstall()
    amd.install(eco=True, eco_init=True)
    both = TL.changed(before, TL.snapshot())
    assert sorted(set(both) - set(eco_set)) == ["pytracking.tracker.eco.eco.GaussNewtonCG"] and set(eco_set) <= set(both)
    ref = amd.original(emod, "GaussNewtonCG")
    assert issubclass(emod.GaussNewtonCG, getattr(ref, "_pt_reference", ref)) and emod.GaussNewtonCG is not ref
    assert po.GaussNewtonCG is not emod.GaussNewtonCG
    amd.uninstall()
    assert TL.changed(before, TL.snapshot()) == []
    amd.install(eco_init=True)                                                          # the switch on its own: the default set plus the one name
    alone = TL.changed(before, TL.snapshot())
    amd.uninstall()
    amd.install()
    assert sorted(set(alone) - set(TL.changed(before, TL.snapshot()))) == ["pytracking.tracker.eco.eco.GaussNewtonCG"]
    amd.uninstall()
    assert TL.changed(before, TL.snapshot()) == []


@needs_reference
def test_cpu_tracker_takes_the_reference_run(amd):
    import eco_tracker as ET
    amd.install(eco=True, eco_init=True)
    amd.stats.clear()
    boxes, scores, tracker = ET.run(n_frames=1)
    stats = dict(amd.stats)
    assert stats.get("ECO.GaussNewtonCG.run.reference") == 1 and "ECO.GaussNewtonCG.run.fast" not in stats, stats
    assert not [k for k in stats if k.endswith(".fast")], stats
    assert np.isfinite(boxes).all() and np.isfinite(scores).all()
    assert tracker.joint_optimizer.residuals.numel() == 0 and tracker.joint_optimizer.losses.numel() == 0
