"""The plan space of the XCD-aligned feature passes and of the steepest-descent solve on them, without a GPU: every case of
tests/fast_pass_cases.py lands on the cell pinned next to it (pt_corr_pass_plan, pt_corr_pass_tail, pt_adj_pass_plan and
pt_sd_solve_route: the launchers' own plan and dispatch helpers, host only), and a sweep of the queries over the grid stated in that
file reaches exactly the cells of the table -- a change of the cost model that opens a cell no case runs, or moves a case off its cell,
fails here.  The dispatch arms that no shape of the grid reaches are pinned as well."""
import ctypes
import itertools

import pytest

import fast_pass_cases as FP
from pytracking_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


@pytest.fixture(scope="module")
def sweep(L):
    """{(n, C, H, W, K, out): (correlation cell, adjoint cell)} of every covered shape of the grid."""
    got = {}
    for C, K, (H, W) in itertools.product(FP.GRID_C, FP.GRID_K, FP.GRID_HW):
        for out in (FP.GRID_OUT if K % 2 == 0 else FP.GRID_OUT[:1]):       # odd K: both output sizes are the same call
            for n in FP.GRID_N:
                c = FP.cells(L, n, C, H, W, K, out)
                if c is not None:
                    got[(n, C, H, W, K, out)] = c
    return got


@pytest.mark.parametrize("idx", range(len(FP.CASES)), ids=lambda i: "-".join(str(v) for v in FP.CASES[i][0]))
def test_case_lands_on_its_pinned_cells(L, idx):
    case, corr, adj = FP.CASES[idx]
    n, C, H, W, K, out, sf = case
    assert out in FP.GRID_OUT and sf in (1, 2) and (out == "full" or K % 2 == 0)
    assert FP.cells(L, *case) == (corr, adj), (case, FP.cells(L, *case))
    assert sf * n * C * H * W * 4 < 2 ** 31 and n * C * H * W <= 8.5e6            # the strided view stays on the fast route; size cap
    # the plan's own arithmetic, restated
    cp, tail, ap = FP.queries(L, n, C, H, W, K, out)
    rem = (H * W // 4) % 16
    assert tail[2] == rem and FP.TAILS[tail[3]] == ("none" if rem == 0 else "left" if rem <= 4 else "part")
    _, E, UM, U, KSPL, gper, CB, bpx, ns_max, PW, adj_lds = ap
    NG = -(-n * H * W // 16)
    OH, OW = FP.out_size(H, W, K, out)
    assert E == (6 if OH * OW <= 384 else 9 if OH * OW <= 576 else 16) and CB == C // 16 and bpx == CB // 8
    assert U == -(-gper // 8) and U <= UM and KSPL == -(-NG // gper) and (KSPL - 1) * gper < NG
    assert UM == (16 if E != 9 else 12 if U <= 12 else 16 if U <= 16 else 24)
    assert ns_max == -(-gper * 16 // (H * W)) + 1 and PW >= W + K - 1 and PW % 16 == 8 and 0 < adj_lds <= 96 * 1024


def test_queries_refuse_and_zero_what_the_plan_does_not_cover(L):
    for q, m in ((L.pt_corr_pass_tail, 4), (L.pt_adj_pass_plan, 11)):
        assert q(3, 128, 18, 18, 4, 4, 19, 19, None) == _lib.PT_ERR_NULL
        for shape in ((3, 100, 18, 18, 4, 4, 19, 19), (3, 128, 9, 7, 3, 3, 9, 7), (3, 128, 6, 6, 4, 4, 7, 7), (3, 128, 18, 18, 5, 5, 18, 18)):
            out = (ctypes.c_int * m)(*([-1] * m))
            assert q(*shape, out) == 0 and list(out) == [0] * m, (shape, list(out))
    assert FP.cells(L, 3, 100, 18, 18, 4) is None
    # DiMP-50, PrDiMP-50 and ATOM at their deployed sizes
    assert FP.cells(L, 50, 512, 18, 18, 4) == ((1, 16, 1, 1, 2, 8, 1, "left"), (6, 16, 8, 0, 0))
    assert FP.cells(L, 50, 512, 22, 22, 4) == ((0, 16, 1, 1, 1, 8, 1, "part"), (9, 24, 8, 0, 0))
    assert FP.cells(L, 250, 64, 18, 18, 4, "same") == ((0, 8, 1, 2, 1, 1, 1, "left"), (6, 16, 64, 1, 0))


def test_reachable_cells_are_the_cells_of_the_table(sweep):
    table_corr, table_adj = {c for _, c, _ in FP.CASES}, {a for _, _, a in FP.CASES}
    grid_corr, grid_adj = {c for c, _ in sweep.values()}, {a for _, a in sweep.values()}
    print(f"\n{len(sweep)} covered shapes of the grid: {len(grid_corr)} correlation cells, {len(grid_adj)} adjoint cells; "
          f"{len(FP.CASES)} cases, {sum(c[0][0] * c[0][1] * c[0][2] * c[0][3] for c in FP.CASES) / 1e6:.1f} M feature floats")
    assert grid_corr - table_corr == set(), f"correlation cells no case runs: {sorted(grid_corr - table_corr)}"
    assert table_corr - grid_corr == set(), f"pinned correlation cells the grid does not reach: {sorted(table_corr - grid_corr)}"
    assert grid_adj - table_adj == set(), f"adjoint cells no case runs: {sorted(grid_adj - table_adj)}"
    assert table_adj - grid_adj == set(), f"pinned adjoint cells the grid does not reach: {sorted(table_adj - grid_adj)}"
    assert len(grid_corr) == 81 and len(grid_adj) == 46
    # every case with sf == 1 is itself a point of the grid
    for (n, C, H, W, K, out, sf), c, a in FP.CASES:
        assert sweep[(n, C, H, W, K, out)] == (c, a)


def test_same_crop_and_strided_variants_are_in_the_table():
    same = [c for c in FP.CASES if c[0][5] == "same"]
    assert len({c for _, c, _ in same}) >= 4 and len({a for _, _, a in same}) >= 4
    strided = [c for c in FP.CASES if c[0][6] == 2]
    assert len({c for _, c, _ in strided}) >= 2 and len({a for _, _, a in strided}) >= 2


# ---- dispatch arms -----------------------------------------------------------------------------------------------------------------
# pt_launch_corr2 compiles PT_C2(NK) for NK in {2, 4, 8, 16} x LEFT x K16 x NH in {1, 2}, and PT_C2M(NK) for NK in {4, 8, 16} x LEFT
CORR_ARMS = ({(0, NK, left, k16, nh) for NK in (2, 4, 8, 16) for left in (0, 1) for k16 in (0, 1) for nh in (1, 2)}
             | {(1, NK, left, 1, 1) for NK in (4, 8, 16) for left in (0, 1)})
CORR_ARMS_UNREACHED = {(0, 2, left, k16, 1) for left in (0, 1) for k16 in (0, 1)}     # NK = 2 is C = 128 split in k-step halves only
ADJ_ARMS = {(6, 16), (9, 12), (9, 16), (9, 24), (16, 16)}


def test_dispatch_arms_no_shape_of_the_grid_reaches(sweep):
    """(MIX, NK, LEFT, K16, NH) of k_corr2 and (E, UM) of k_adj2: which compiled arms the grid runs.  The unreached ones are listed in
    DESIGN.md section 10; a plan change that reaches one of them, or stops reaching another, fails here."""
    reached = {(c[0], c[1], int(c[7] == "left"), c[2], c[3]) for c, _ in sweep.values()}
    assert reached <= CORR_ARMS
    assert CORR_ARMS - reached == CORR_ARMS_UNREACHED, sorted(CORR_ARMS - reached)
    assert {a[:2] for _, a in sweep.values()} == ADJ_ARMS
    assert len(reached) == 34


# ---- solver ------------------------------------------------------------------------------------------------------------------------
def _solver_cell(L, v, n, C, H, W, K, want_losses=True):
    """(V, (E, UM), FUSE, layout) of a solve on the fast route, None on the generic one."""
    rc, out = FP.solve_route(L, v, n, C, H, W, K, want_losses)
    assert rc == 0, (rc, v, n, C, H, W, K)
    if not out[0]:
        assert out == [0, 0, 0, 0]
        return None
    assert out[3] == int(want_losses)
    _, adj = FP.cells(L, n, C, H, W, K)
    return out[1], adj[:2], out[2], FP.layout_of(L, n, C, H, W, K)


@pytest.mark.parametrize("case", FP.SOLVER_CASES, ids=lambda c: f"{FP.V_NAMES[c[0]]}-{c[1]}")
def test_solver_case_lands_on_its_pinned_route(L, case):
    v, tag, has_sw, iters, seed = case
    shape, want = FP.SOLVER_SHAPES[tag]
    for want_losses in (True, False):
        assert _solver_cell(L, v, *shape, want_losses) == (v,) + want, (case, _solver_cell(L, v, *shape, want_losses))


def test_reachable_solver_pairs_are_the_pairs_of_the_table(L, sweep):
    table = {(v,) + FP.SOLVER_SHAPES[tag][1] for v, tag, *_ in FP.SOLVER_CASES}
    grid = set()
    for (n, C, H, W, K, out), (corr, adj) in sweep.items():
        if out != "full":
            continue
        for v in FP.V_NAMES:
            c = _solver_cell(L, v, n, C, H, W, K)
            assert (c is None) == (adj[2] > 16), (n, C, H, W, K, c)           # more than 16 adjoint slices: the generic route
            if c is not None:
                grid.add(c)
    for name, pick in (("(V, adjoint instantiation)", lambda c: (c[0], c[1])), ("(V, FUSE)", lambda c: (c[0], c[2])),
                       ("(V, correlation layout)", lambda c: (c[0], c[3]))):
        g, t = {pick(c) for c in grid}, {pick(c) for c in table}
        assert g == t, f"{name}: reachable but not in the table {sorted(g - t)}, in the table but not reachable {sorted(t - g)}"
    assert len({(c[0], c[1]) for c in table}) == 20 and len({(c[0], c[2]) for c in table}) == 8 and len({(c[0], c[3]) for c in table}) == 16
    assert {has_sw for _, _, has_sw, *_ in FP.SOLVER_CASES} == {True, False}
    for v in FP.V_NAMES:
        assert {has_sw for vv, _, has_sw, *_ in FP.SOLVER_CASES if vv == v} == {True, False}


def test_solve_route_follows_the_solves_own_predicate(L):
    out = (ctypes.c_int * 4)()
    p = FP.solver_params(FP.V_RELU)
    shape = (7, 128, 18, 18, 4)
    args = lambda w=256, f=256, stride=128 * 324, it=256: (ctypes.byref(p), w, f, stride, it, *shape, 1, out)
    assert L.pt_sd_solve_route(*args()) == 0 and list(out) == [1, FP.V_RELU, 8, 1]
    assert L.pt_sd_solve_route(None, 256, 256, 128 * 324, 256, *shape, 1, out) == _lib.PT_ERR_NULL
    assert L.pt_sd_solve_route(ctypes.byref(p), 256, 256, 128 * 324, 256, *shape, 1, None) == _lib.PT_ERR_NULL
    assert L.pt_sd_solve_route(*args(stride=128 * 324 - 4)) == _lib.PT_ERR_SHAPE
    for kw in (dict(f=260), dict(w=260), dict(it=260), dict(stride=128 * 324 + 2)):        # what the 16-byte loads need
        assert L.pt_sd_solve_route(*args(**kw)) == 0 and list(out) == [0, 0, 0, 0], kw
    p.num_bins = 4100                                                                      # tables beyond the init stage's LDS
    assert L.pt_sd_solve_route(*args()) == 0 and list(out) == [0, 0, 0, 0]
    p.num_bins = 0
    assert L.pt_sd_solve_route(*args()) == _lib.PT_ERR_NULL                                # as the solve: no look-up tables
    p = FP.solver_params(FP.V_PRDIMP)
    assert L.pt_sd_solve_route(ctypes.byref(p), 256, 256, 64 * 324, 256, 250, 64, 18, 18, 4, 0, out) == 0 and list(out) == [0, 0, 0, 0]
    assert L.pt_sd_solve_route(ctypes.byref(p), 256, 256, 128 * 252, 256, 66, 128, 14, 18, 4, 0, out) == 0
    assert list(out) == [1, FP.V_PRDIMP, 16, 0]
    assert L.pt_sd_solve_route(ctypes.byref(p), 256, 256, 128 * 324, 256, 7, 128, 18, 18, 5, 0, out) == _lib.PT_ERR_UNSUPPORTED
