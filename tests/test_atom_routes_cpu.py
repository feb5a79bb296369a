"""CPU half of the ATOM route tests (tests/atom_cases.py): every case lands on the route pinned next to it, a sweep of the two host-only
queries over the grid stated there reaches exactly the tables' cells (a plan change that opens a cell no case runs fails here), the queries
follow the entries' predicates and refusals, the oracle matches the reference's goldens off the 4x4 shapes, the inputs keep the
max(beta, 0) clamp away from zero, and every seeded defect of the fp32 restatement misses the float64 bound that the device is held to."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import atom_cases as AC
import f64_bound
from conftest import load_golden
from oracle import np_oracle as O
from pytracking_amd import _lib, synth


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


# ---- pins and sweeps ---------------------------------------------------------------------------------------------------------------------
def test_every_case_lands_on_its_pinned_route(L):
    assert len({c.name for c in AC.CG_CASES}) == len(AC.CG_CASES) and len({c.name for c in AC.GN_CASES}) == len(AC.GN_CASES)
    for c in AC.CG_CASES:
        assert AC.cg_case_route(L, c) == (0, c.route), c.name
        assert (c.route[0] == 1) == (c in AC.CG_FUSED), c.name
    for c in AC.GN_CASES:
        assert AC.gn_case_route(L, c) == (0, c.route), c.name
    assert set(AC.CG_FOLD) <= {c.name for c in AC.CG_FUSED}


def test_tables_cover_what_the_issue_lists():
    """the variants, schedules and edges spread over the cells as tests/atom_cases.py promises"""
    fused = [c for c in AC.CG_FUSED if c.edge != "zero_rhs"]
    for cell in {("geo", t, k) for t in (4, 5) for k in (AC.NONE, AC.LEFT, AC.PART)}:
        on = [c for c in fused if cell in AC.cg_cells(c.route)]
        assert any(c.variant[0] for c in on) and any(c.variant[1] != 0 and len(c.calls) > 1 for c in on), cell      # FR, and forgetting with state
    assert {("slices", l, b) for l in (0, 1) for b in (8, 16, 32, 64)} <= set().union(*(AC.cg_cells(c.route) for c in fused))
    assert {c.route[4] for c in fused} >= {6, 7, 8, 16, 32, 64} and {c.route[3] for c in fused} >= {0, 1, 4, 5, 15}
    assert {c.calls for c in fused} == {AC.A, AC.B, AC.S1, AC.S2} and {c.variant for c in fused} >= {AC.PR0, AC.PR75, AC.FR0, AC.FR75}
    assert {c.edge for c in AC.CG_FUSED} == {None, "zero_tail", "view", "zero_rhs"} and any(c.n == 1 for c in fused)
    gen = AC.CG_GENERIC
    assert {(c.K, c.C) for c in gen if c.K < 4} >= {(1, 24), (1, 32), (2, 32), (2, 40), (3, 40), (3, 24)}
    assert all({(c.H * c.W) % 4 == 0 for c in gen if c.K == k} == {True, False} for k in (1, 2, 3))
    assert {c.route[2] for c in gen} == {16, 8, 4, 0} and {c.edge for c in gen} == {None, "mis_base", "stride1", "mis_state", "zero_rhs"}
    assert {c.variant for c in gen} >= {AC.PR0, AC.PR75, AC.FR0, AC.FR75} and {c.calls for c in gen} == {AC.A, AC.B, AC.S1, AC.S2}
    gn = AC.GN_CASES
    assert {c.Kc for c in gn} >= {8, 16, 24, 32, 40} and {c.K for c in gn} == {1, 2, 3, 4} and {c.fr for c in gn} == {True, False}
    assert {c.M % 16 == 0 for c in gn} == {True, False} and {(c.H * c.W) % 4 == 0 for c in gn} == {True, False}
    assert any(c.route[3] != c.n for c in gn) and {c.edge for c in gn} == {None, "stride1", "mis_base", "view"}
    assert any(c.Kc % 16 == 0 and (c.H * c.W) % 4 for c in gn) and any(list(c.iters) == [2, 0, 1] for c in gn) and any(c.one_weight for c in gn)
    assert any((c.n, c.M, c.Kc, c.H, c.W, c.K) == (30, 256, 64, 18, 18, 4) for c in gn)


def test_cg_sweep_reaches_exactly_the_tables_cells(L):
    reached = set()
    for H, W, n, C, K, (off, extra) in itertools.product(AC.GRID_HW, AC.GRID_HW, AC.GRID_CG_N, AC.GRID_CG_C, AC.GRID_K, AC.GRID_LAYOUT):
        rc, route = AC.cg_route(L, n, C, H, W, K, samples=256 + off, stride=C * H * W + extra)
        assert rc == 0
        reached |= AC.cg_cells(route)
    table = set().union(*(AC.cg_cells(c.route) for c in AC.CG_CASES))
    assert reached == table, (sorted(reached - table), sorted(table - reached))


def test_gn_sweep_reaches_exactly_the_tables_cells(L):
    reached, paired = set(), set()
    for H, W, n, Kc, M, K, (off, extra) in itertools.product(AC.GRID_HW, AC.GRID_HW, AC.GRID_GN_N, AC.GRID_GN_KC, AC.GRID_GN_M, AC.GRID_GN_K,
                                                             AC.GRID_LAYOUT):
        rc, route = AC.gn_route(L, n, M, Kc, H, W, K, samples=256 + off, stride=M * H * W + extra)
        assert rc == 0
        reached.add(AC.gn_cell(route))
        paired.add(route[4])
    table = {AC.gn_cell(c.route) for c in AC.GN_CASES}
    assert reached == table, (sorted(reached - table), sorted(table - reached))
    # the unpaired fallback of the CG step's two correlations needs the two map bases to differ mod 16; they are carved from one
    # 256-byte aligned workspace in 256-byte granules, so no shape reaches it
    assert paired == {1}


# ---- the queries follow the entries ------------------------------------------------------------------------------------------------------
def test_cg_query_follows_the_entry(L):
    fused, generic = (1, 5, AC.LEFT, 1, 8), (0, 1, 4, 4, 1)
    q = lambda **kw: AC.cg_route(L, 5, 64, 18, 18, 4, **kw)
    assert q() == (0, fused)
    for kw in (dict(samples=260), dict(x=260), dict(state=260), dict(stride=64 * 324 + 1), dict(stride=64 * 324 + 2)):
        rc, route = q(**kw)
        assert rc == 0 and route[0] == 0 and route[2] == generic[2], kw                       # each misalignment flips the route
        assert route[1] == (0 if "samples" in kw or "stride" in kw else 1), kw                # and only the samples' decide VEC
    assert q(stride=2 * 64 * 324) == (0, fused) and q(samples=256 + 16, x=512 + 16, state=1024 + 16) == (0, fused)
    # refusals: the entry's codes, `out` zeroed
    one, it = 256, (ctypes.c_int * 5)()
    refusals = [(dict(x=None), _lib.PT_ERR_NULL), (dict(samples=None), _lib.PT_ERR_NULL), (dict(state=None), _lib.PT_ERR_NULL),
                (dict(stride=64 * 324 - 1), _lib.PT_ERR_SHAPE)]
    for kw, code in refusals:
        assert q(**kw) == (code, (0,) * 5), kw
    assert AC.cg_route(L, 0, 64, 18, 18, 4) == (_lib.PT_ERR_SHAPE, (0,) * 5) and AC.cg_route(L, 5, 64, 18, 18, 5) == (_lib.PT_ERR_UNSUPPORTED, (0,) * 5)
    assert L.pt_atom_cg_route(one, one, 64 * 324, one, 5, 64, 18, 18, 4, None) == _lib.PT_ERR_NULL
    # the entry refuses the same shapes with the same codes in front of anything it would launch (workspace 0 bytes: -4 once the shape is accepted)
    entry = lambda n, K, stride: L.pt_atom_cg_f32(one, one, stride, one, one, 0.1, 0.05, n, 64, 18, 18, K, 2, 0, 0.0, one, one, 0, None)
    assert entry(0, 4, 64 * 324) == _lib.PT_ERR_SHAPE and entry(5, 5, 64 * 324) == _lib.PT_ERR_UNSUPPORTED
    assert entry(5, 4, 64 * 324 - 1) == _lib.PT_ERR_SHAPE and entry(5, 4, 64 * 324) == _lib.PT_ERR_WORKSPACE
    for i in range(5):
        it[i] = 7
    assert L.pt_atom_cg_route(one, one, 64 * 324, one, 5, 64, 18, 18, 5, it) == _lib.PT_ERR_UNSUPPORTED and list(it) == [0] * 5


def test_gn_query_follows_the_entry(L):
    q = lambda **kw: AC.gn_route(L, 6, 32, 16, 12, 12, 2, **kw)
    assert q()[1][:2] == (AC.DIRECT, AC.GEMM)
    for kw in (dict(samples=260), dict(stride=32 * 144 + 1), dict(stride=32 * 144 + 2)):
        assert q(**kw)[1][:2] == (AC.BANKED, AC.BANKED), kw
    assert q(stride=2 * 32 * 144)[1][:2] == (AC.DIRECT, AC.GEMM)
    assert q(samples=None) == (_lib.PT_ERR_NULL, (0,) * 10) and q(stride=32 * 144 - 1) == (_lib.PT_ERR_SHAPE, (0,) * 10)
    assert AC.gn_route(L, 0, 32, 16, 12, 12, 2) == (_lib.PT_ERR_SHAPE, (0,) * 10)
    assert AC.gn_route(L, 6, 32, 16, 12, 12, 5) == (_lib.PT_ERR_UNSUPPORTED, (0,) * 10)
    assert L.pt_atom_gn_route(256, 32 * 144, 6, 32, 16, 12, 12, 2, None) == _lib.PT_ERR_NULL
    one, it = 256, (ctypes.c_int * 2)(2, 2)
    entry = lambda n, K, stride: L.pt_atom_gn_f32(one, one, one, stride, one, one, 0.1, 1e-4, 0.05, n, 32, 16, 12, 12, K, it, 2, 1, one, 0, None)
    assert entry(0, 2, 32 * 144) == _lib.PT_ERR_SHAPE and entry(6, 5, 32 * 144) == _lib.PT_ERR_UNSUPPORTED
    assert entry(6, 2, 32 * 144 - 1) == _lib.PT_ERR_SHAPE and entry(6, 2, 32 * 144) == _lib.PT_ERR_WORKSPACE
    # the workspace the entry carves is what the query's alignment argument rests on: 256-byte granules
    assert L.pt_atom_gn_ws_bytes(6, 32, 16, 12, 12, 2) % 256 == 0


# ---- the oracle against the reference off the 4x4 goldens --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,atol,rtol", [(np.float64, 2e-5, 1e-4), (np.float32, 2e-5, 1e-4)], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", ["pr", "fr", "pr0", "fr0"])
def test_oracle_matches_reference_on_fused_shape(tag, dtype, atol, rtol):
    g = load_golden("atom_cg_c64_fused")
    c = next(c for c in AC.CG_CASES if c.name == f"golden-{tag}")
    assert (int(g["seed"]), int(g["n"]), int(g["H"]), int(g["W"])) == (c.seed, c.n, c.H, c.W) and tuple(g["iters"]) == c.calls
    assert (bool(int(g[f"{tag}_fr"])), float(g[f"{tag}_forget"])) == c.variant
    for k, x in enumerate(AC.cg_run(c, dtype).values()):
        np.testing.assert_allclose(x.astype(np.float64), g[f"{tag}_x_out"][k].astype(np.float64), atol=atol, rtol=rtol)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_oracle_matches_reference_cg_small_filters(K, dtype):
    """conv2d(mode='same') with a 1-, 2- and 3-tap filter side: until these the oracle was pinned to the reference at K = 4 only"""
    g = load_golden(f"atom_cg_k{K}")
    assert g["x0"].shape[-1] == K
    x, state = g["x0"].astype(dtype), None
    for k, iters in enumerate(g["iters"]):
        x, state = O.atom_cg(x, g["samples"].astype(dtype), g["y"].astype(dtype), g["sw"].astype(dtype), filter_reg=synth.ATOM18["filter_reg"],
                             act_min_val=synth.ATOM18["act_min_val"], num_iter=int(iters), fletcher_reeves=bool(int(g["fletcher_reeves"])),
                             state=state, direction_forget_factor=float(g["forget"]))
        assert x.dtype == dtype
        np.testing.assert_allclose(x.astype(np.float64), g["x_out"][k].astype(np.float64), atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["atom_gn_k3", "atom_gn_kc24"])
def test_oracle_matches_reference_gn(name, dtype):
    g = load_golden(name)
    f, P = O.atom_gn_cg(*(g[k].astype(dtype) for k in ("f0", "P0", "samples", "y", "sw")), filter_reg=float(g["filter_reg"]),
                        projection_reg=float(g["projection_reg"]), act_min_val=float(g["act_min_val"]),
                        cg_iters=[int(v) for v in g["cg_iters"]], fletcher_reeves=bool(int(g["fletcher_reeves"])))
    np.testing.assert_allclose(f.astype(np.float64), g["f_out"], atol=5e-5)
    np.testing.assert_allclose(P.astype(np.float64), g["P_out"], atol=5e-5)


# ---- conditions on the inputs ------------------------------------------------------------------------------------------------------------
def _steps(trace):
    return [e for call in trace for e in (call if isinstance(call, list) else [call])]


def _check_trace(name, steps):
    betas = [e["beta"] for e in steps if e.get("beta") is not None]
    assert all("pq" in e and e["pq"] > 0 and e["rho"] > 0 for e in steps), name              # no stop, every p.q and rho positive
    if name == AC.CLAMP:
        assert min(betas) <= AC.BETA_CLAMPED and all(b <= AC.BETA_CLAMPED or b >= AC.BETA_MIN for b in betas), (name, betas)
    else:
        assert min(betas, default=1.0) >= AC.BETA_MIN, (name, betas)
    return betas


@pytest.mark.parametrize("c", [c for c in AC.CG_CASES if c.edge != "zero_rhs"], ids=lambda c: c.name)
def test_cg_inputs_keep_the_clamp_away_from_zero(c):
    trace = []
    AC.cg_run(c, np.float64, trace=trace)
    betas = _check_trace(c.name, _steps(trace))
    assert len(_steps(trace)) == sum(c.calls)
    if c.name == AC.CLAMP:                         # the same steps are clamped in fp32
        t32 = []
        AC.cg_run(c, np.float32, trace=t32)
        assert [b < 0 for b in _check_trace(c.name, _steps(t32))] == [b < 0 for b in betas]


@pytest.mark.parametrize("c", [c for c in AC.CG_CASES if c.edge == "zero_rhs"], ids=lambda c: c.name)
def test_cg_zero_right_hand_side_stops_in_the_oracle(c):
    for dtype in (np.float64, np.float32):
        trace, problem = [], AC.cg_problem(c)
        out = AC.cg_run(c, dtype, problem, trace=trace)
        assert _steps(trace) == [dict(rho=0.0)] * len(c.calls) and all(np.array_equal(x, problem[0]) for x in out.values())


@pytest.mark.parametrize("c", AC.GN_CASES, ids=lambda c: c.name)
def test_gn_inputs_keep_the_clamp_away_from_zero(c):
    trace = []
    AC.gn_run(c, np.float64, trace=trace)
    _check_trace(c.name, trace)
    assert len(trace) == sum(c.iters)


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------------
def _miss(run, c, defect, key):
    """largest err / max(ref_err, floor) over the outputs of the fp32 restatement with `defect`, the units those of the device tests"""
    a = f64_bound.anchor((key, c.name), lambda dt: run(c, dt), group=lambda q: q)
    bad = run(c, np.float32, defect=defect)
    return max(f64_bound.errors(w, bad[q])[""] / max(a.ref_errs[q], f64_bound.spacing_of_max(w)) for q, w in a.want.items())


# the cases a defect can show on: small ones (the restatement runs three times per case), with the state, variant or weights it needs
_SMALL = [c for c in AC.CG_CASES if c.n <= 5 and c.edge != "zero_rhs"]
CG_DEFECT_CASES = {
    "forget_rho": [c for c in _SMALL if c.variant[1] != 0 and len(c.calls) > 1],
    "drop_state": [c for c in _SMALL if c.variant[1] != 0 and len(c.calls) > 1],
    "pr_for_fr": [c for c in _SMALL if c.variant[0] and max(c.calls) >= 3],
    "stale_r_prev": [c for c in _SMALL if not c.variant[0] and max(c.calls) >= 3],
    "sw_not_sqrt": _SMALL[:6],
    "no_lambda_p": _SMALL[:6],
}
_GN_SMALL = [c for c in AC.GN_CASES if c.name != "first-frame"]


def test_cg_seeded_defects_miss_the_bound():
    assert set(CG_DEFECT_CASES) == set(O.ATOM_CG_DEFECTS) | {"drop_state"}
    worst = {d: max(_miss(AC.cg_run, c, d, "atom_cg") for c in cases) for d, cases in CG_DEFECT_CASES.items()}
    print("\nCG seeded defects, largest miss ratio over the table: " + "  ".join(f"{d} {r:.3g}" for d, r in worst.items()))
    assert all(r > f64_bound.FACTOR for r in worst.values()), worst
    assert f64_bound.FACTOR < AC.F_MAX_CG <= math.floor(min(worst.values())) < 2 * AC.F_MAX_CG, worst


def test_gn_seeded_defects_miss_the_bound():
    worst = {d: max(_miss(AC.gn_run, c, d, "atom_gn") for c in _GN_SMALL) for d in O.ATOM_GN_DEFECTS}
    print("\nGN seeded defects, largest miss ratio over the table: " + "  ".join(f"{d} {r:.3g}" for d, r in worst.items()))
    assert all(r > f64_bound.FACTOR for r in worst.values()), worst
    assert f64_bound.FACTOR < AC.F_MAX_GN <= math.floor(min(worst.values())) < 2 * AC.F_MAX_GN, worst
