"""Case tables of ATOM's two solvers -- the conjugate-gradient filter update (csrc/atom_cg.hip, pt_atom_cg_f32) and the first-frame joint
Gauss-Newton (csrc/atom_gn.hip, pt_atom_gn_f32) -- each case pinned to the kernel route it takes through the library's own host-only
queries (pt_atom_cg_route, pt_atom_gn_route: the entries' predicates and the launchers' dispatch helpers, nothing launched).
tests/test_atom_routes_cpu.py checks the pins and that a sweep of the queries over GRID reaches exactly the cells of the tables;
tests/test_gpu_atom_routes.py runs every case on the device against oracle.np_oracle in float64 under the bound of tests/f64_bound.py.

A CG route is what pt_atom_cg_route writes:   fused (1, tiles, tail, leftover quads, adjoint slices)
                                              generic (0, VEC, NK arm, channel slices, adjoint slices)
and its cells are   ("geo", tiles, tail)  +  ("slices", LEFT instantiation, bucket of the adjoint slices: 8 = up to 8 | 16 | 32 | 64)
for the fused route (k_acg_fwd<LEFT, .> with its tile count and tail kind; the partial sums k_acg_red / k_acg_final fold) and
("generic", VEC, NK arm) for the generic one (the k_corr<VEC, NK> instantiation).  A GN cell is (conv1x1 arm, projection-adjoint arm).

numpy only at import.  Test infrastructure only."""
import ctypes
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import np_oracle as O
from pytracking_amd import synth

CFG = synth.ATOM18
NONE, LEFT, PART = 0, 1, 2                         # tail kinds of the fused route
DIRECT, BANKED, GROUPS = 0, 1, 2                   # conv1x1 arms of the joint Gauss-Newton
GEMM = 0                                           # its projection-adjoint arms: GEMM, BANKED, GROUPS

# (fletcher_reeves, direction_forget_factor)
PR0, PR75, FR0, FR75 = (False, 0.0), (False, 0.75), (True, 0.0), (True, 0.75)
# iterations per run() call; the CG state is carried from call to call
A, B, S1, S2 = (3, 2, 3), (1, 1, 4), (1,), (2,)

# edge: None | "zero_tail" (the last `arg` samples have zero weight and zero features) | "view" (channels [0, C) of a (n, 2C, H, W) tensor)
#       | "zero_rhs" (samples = 0, x0 = 0) | "mis_base" (sample base 4 bytes off 16) | "stride1" (sample stride C*H*W + 1)
#       | "mis_state" (cg_state 4 bytes off 16: through the C entry)
CgCase = namedtuple("CgCase", "name n C H W K variant calls seed route edge arg", defaults=(None, 0))

CG_FUSED = [
    #       name               n   C   H   W  K variant calls seed  route
    CgCase("t4-none",          3, 64, 16, 16, 4, FR75, A, 401, (1, 4, NONE, 0, 8)),
    CgCase("t4-left1-n1",      1, 64, 10, 26, 4, PR75, B, 702, (1, 4, LEFT, 1, 6)),          # n = 1; 6 ragged slices
    CgCase("t4-left4",         2, 64, 16, 17, 4, FR0, A, 403, (1, 4, LEFT, 4, 7)),           # 7 ragged slices
    CgCase("t4-part9",         5, 64, 12, 19, 4, FR75, B, 404, (1, 4, PART, 9, 8)),
    CgCase("t4-part15",        4, 64, 14, 18, 4, PR0, S2, 405, (1, 4, PART, 15, 8)),
    CgCase("t5-none-n1",       1, 64, 16, 20, 4, FR75, A, 406, (1, 5, NONE, 0, 7)),
    CgCase("t5-left1",         5, 64, 18, 18, 4, FR75, B, 407, (1, 5, LEFT, 1, 8)),
    CgCase("t5-left4",         3, 64, 12, 28, 4, PR75, A, 408, (1, 5, LEFT, 4, 8)),
    CgCase("t5-part5",         2, 64, 12, 23, 4, FR75, A, 409, (1, 5, PART, 5, 7)),          # odd W
    CgCase("t5-part8-1iter",   1, 64, 16, 18, 4, PR0, S1, 410, (1, 5, PART, 8, 6)),          # num_iter == 1: no phase-2 launch
    CgCase("t5-part8",         5, 64, 16, 18, 4, PR75, B, 411, (1, 5, PART, 8, 8)),
    # slice buckets 16 / 32 / 64 on a non-LEFT and on a LEFT map, at the smallest n of each
    CgCase("s16-t5-none",     52, 64, 16, 20, 4, FR75, A, 412, (1, 5, NONE, 0, 16)),
    CgCase("s32-t5-none",    103, 64, 16, 20, 4, FR0, S2, 413, (1, 5, NONE, 0, 32)),
    CgCase("s64-t5-none",    205, 64, 16, 20, 4, FR75, B, 414, (1, 5, NONE, 0, 64)),
    CgCase("s16-t4-left",     64, 64, 10, 26, 4, FR75, B, 415, (1, 4, LEFT, 1, 16)),
    CgCase("s32-t4-left",    127, 64, 10, 26, 4, PR0, S1, 416, (1, 4, LEFT, 1, 32)),
    CgCase("s64-t4-left",    253, 64, 10, 26, 4, FR75, B, 417, (1, 4, LEFT, 1, 64)),         # 4.2 M feature floats
    # the reference's golden atom_cg_c64_fused (oracle/make_golden.py gen_atom_routes): the four variants of atom_cg_c64 at 16x16
    CgCase("golden-pr",       12, 64, 16, 16, 4, (False, 0.75), A, 322, (1, 4, NONE, 0, 8)),
    CgCase("golden-fr",       12, 64, 16, 16, 4, (True, 0.5), A, 322, (1, 4, NONE, 0, 8)),
    CgCase("golden-pr0",      12, 64, 16, 16, 4, PR0, A, 322, (1, 4, NONE, 0, 8)),
    CgCase("golden-fr0",      12, 64, 16, 16, 4, FR0, A, 322, (1, 4, NONE, 0, 8)),
    # edges
    CgCase("zero-tail",        5, 64, 18, 18, 4, PR75, A, 418, (1, 5, LEFT, 1, 8), "zero_tail", 3),
    CgCase("view",             4, 64, 16, 16, 4, FR0, A, 419, (1, 4, NONE, 0, 8), "view"),
    CgCase("zero-rhs-left",    3, 64, 18, 18, 4, PR75, A, 420, (1, 5, LEFT, 1, 8), "zero_rhs"),
    CgCase("zero-rhs-none",    2, 64, 16, 20, 4, FR0, S2, 421, (1, 5, NONE, 0, 8), "zero_rhs"),
]

CG_GENERIC = [
    # K = 1, 2, 3 at C in {24, 32, 40}, H*W % 4 != 0 and == 0
    CgCase("k1-c24-odd",       3, 24,  7,  9, 1, FR75, A, 431, (0, 0, 0, 1, 1)),
    CgCase("k1-c24-clamp",     3, 24,  7,  9, 1, PR75, A, 5000, (0, 0, 0, 1, 1)),        # CLAMP: one beta <= -0.05, clamped to 0
    CgCase("k1-c32",           4, 32,  8,  8, 1, FR0, B, 432, (0, 1, 4, 2, 1)),
    CgCase("k2-c32",           4, 32, 10, 10, 2, FR75, A, 433, (0, 1, 4, 2, 1)),
    CgCase("k2-c40-odd",       2, 40,  9, 11, 2, PR0, S2, 434, (0, 0, 0, 2, 1)),
    CgCase("k3-c40",           2, 40, 10, 12, 3, PR75, B, 435, (0, 1, 0, 2, 1)),
    CgCase("k3-c24-odd",       5, 24,  9,  9, 3, FR75, A, 436, (0, 0, 0, 1, 1)),
    CgCase("k3-c32-odd",       3, 32,  7,  7, 3, FR0, S1, 437, (0, 0, 4, 2, 1)),
    # the k_corr<VEC, NK> arms
    CgCase("nk16",           256, 128, 6,  6, 4, PR0, S2, 438, (0, 1, 16, 2, 8)),
    CgCase("nk16-odd",       256, 128, 7,  7, 2, FR0, S2, 439, (0, 0, 16, 2, 8)),
    CgCase("nk8",            256, 64,  6,  6, 4, FR75, B, 440, (0, 1, 8, 2, 8)),
    CgCase("nk8-odd",        256, 64,  7,  7, 3, FR75, A, 441, (0, 0, 8, 2, 8)),
    CgCase("nk0-n1",           1, 40, 10, 10, 4, FR75, A, 442, (0, 1, 0, 2, 1)),
    # each way a C = 64, K = 4 problem falls off the fused route
    CgCase("c64-2tiles",       3, 64, 12, 12, 4, FR75, A, 443, (0, 1, 4, 4, 1)),
    CgCase("c64-8tiles",       2, 64, 22, 22, 4, PR75, B, 444, (0, 1, 4, 4, 1)),
    CgCase("c64-mis-base",     3, 64, 18, 18, 4, FR75, A, 445, (0, 0, 4, 4, 1), "mis_base"),
    CgCase("c64-stride1",      3, 64, 18, 18, 4, PR75, A, 446, (0, 0, 4, 4, 1), "stride1"),
    CgCase("c64-mis-state",    3, 64, 18, 18, 4, PR75, A, 447, (0, 1, 4, 4, 1), "mis_state"),
    CgCase("c64-n405",       405, 64, 18, 18, 4, PR0, S2, 448, (0, 1, 8, 2, 64)),            # the fused plan finds no slice count
    CgCase("zero-rhs",         2, 32,  7,  7, 3, PR75, A, 449, (0, 0, 4, 2, 1), "zero_rhs"),
]
CG_CASES = CG_FUSED + CG_GENERIC
# Conditions on the inputs (tests/test_atom_routes_cpu.py, in float64): every Polak-Ribiere / Fletcher-Reeves beta before the max(beta, 0)
# clamp is >= BETA_MIN, so that the clamp is no discontinuity between float64, fp32 and the device -- but for CLAMP, the first of 200 seeds
# at the smallest shape with a beta <= BETA_CLAMPED in float64 and in fp32 alike (and every other beta >= BETA_MIN).
BETA_MIN, BETA_CLAMPED, CLAMP = 0.02, -0.05, "k1-c24-clamp"
# the four cases of the PT_ACG_FOLD=1 child process: LEFT and non-LEFT, <= 8 and 64 slices, PR with forgetting and FR, state carried
CG_FOLD = ("t5-left4", "t4-part9", "s64-t5-none", "s64-t4-left")

# edge: None | "stride1" (sample stride M*H*W + 1) | "mis_base" | "view" (channels [0, M) of a (n, 2M, H, W) tensor)
# one_weight: the single broadcast sample weight 1 / n;  zero_f0: the tracker's zero initial filter;  route: pt_atom_gn_route's ten ints
GnCase = namedtuple("GnCase", "name n M Kc H W K fr iters seed route edge one_weight zero_f0", defaults=(None, False, False))

GN_CASES = [
    #       name            n    M  Kc   H   W  K  fr     iters     seed  (proj, jT, NGRP, NSG, paired, adj grid.z, VEC, NK, KS, KSPL)
    GnCase("first-frame",  30, 256, 64, 18, 18, 4, True,  [4, 4, 4],  77, (DIRECT, GEMM, 4, 30, 1, 16, 1, 4, 4, 8), None, False, True),
    GnCase("kc8-k1",        4,  16,  8, 10, 10, 1, False, [2, 0, 1], 451, (GROUPS, GROUPS, 1, 4, 1, 9, 1, 0, 1, 1)),
    GnCase("kc16-odd-k3",   3,  24, 16,  9, 11, 3, True,  [3, 2],    452, (BANKED, BANKED, 1, 3, 1, 13, 0, 4, 1, 1)),
    GnCase("kc16-k2",       6,  32, 16, 12, 12, 2, False, [2, 2],    453, (DIRECT, GEMM, 1, 6, 1, 25, 1, 4, 1, 1)),
    GnCase("kc24-k3",       4,  16, 24, 10, 10, 3, True,  [3, 3],    454, (GROUPS, GROUPS, 2, 4, 1, 13, 1, 0, 1, 1)),
    GnCase("kc40-odd",      2,  32, 40,  9,  9, 4, False, [2, 0, 1], 455, (GROUPS, GROUPS, 3, 2, 1, 8, 0, 0, 2, 1)),
    GnCase("kc32-one-w",    5,  48, 32,  8, 10, 4, True,  [3, 2],    456, (DIRECT, GEMM, 2, 5, 1, 21, 1, 4, 2, 1), None, True),
    GnCase("nsg-split",     1,  16, 16,  9, 32, 1, True,  [3, 2],    457, (DIRECT, BANKED, 1, 2, 1, 5, 1, 4, 1, 1)),
    GnCase("stride1",       3,  16, 16, 12, 12, 3, False, [2, 2],    458, (BANKED, BANKED, 1, 3, 1, 13, 1, 4, 1, 1), "stride1"),
    GnCase("mis-base",      3,  32, 32, 10, 10, 2, True,  [2, 0, 1], 459, (BANKED, BANKED, 2, 3, 1, 13, 1, 4, 2, 1), "mis_base"),
    GnCase("m12",           4,  12, 16, 10, 10, 4, True,  [3, 2],    460, (BANKED, GEMM, 1, 4, 1, 17, 1, 4, 1, 1)),
    GnCase("view-kc24",     2,  16, 24, 11,  9, 2, False, [2, 2],    461, (GROUPS, GROUPS, 2, 2, 1, 7, 0, 0, 1, 1), "view"),
]

# The grid of the sweeps: every map from 6x6 to 32x32, the n of the tables, the channel counts below, every filter side, and the three
# sample layouts (16-byte aligned and dense | base 4 bytes off | stride + 1 float).
GRID_HW = range(6, 33)
GRID_CG_C = (24, 32, 40, 64, 128)
GRID_GN_KC = (8, 16, 24, 32, 40, 64)
GRID_GN_M = (12, 16, 48, 256)
GRID_K = (1, 2, 3, 4)
GRID_GN_K = (1, 4)                                 # the filter side enters no dispatch of the joint Gauss-Newton: its extremes
GRID_LAYOUT = ((0, 0), (4, 0), (0, 1))             # (bytes added to a 256-byte aligned base, floats added to the dense stride)
GRID_CG_N = sorted({c.n for c in CG_CASES})
GRID_GN_N = sorted({c.n for c in GN_CASES})


# The smallest ratio by which a seeded defect of the fp32 restatement misses max(ref_err, floor) on its best case of the table, rounded
# down to a power of two because ref_err moves by tens of per cent with the summation blocking (tests/test_atom_routes_cpu.py computes them
# -- CG: 4.26e5, the missing lambda * p of q; GN: 8.14e4, the missing projection regulariser -- and asserts that they lie in
# [F_MAX, 2 F_MAX)): raised_factor() may not lift a device bound above it.  The iterates move by 1e-2 under any of the defects, 1e5 roundings.
F_MAX_CG, F_MAX_GN = 2 ** 18, 2 ** 16


# ---- the queries -----------------------------------------------------------------------------------------------------------------------
def cg_route(L, n, C, H, W, K, x=256, samples=256, stride=None, state=256):
    """(status, the five ints) of pt_atom_cg_route; the operands are addresses (nothing reads through them)"""
    out = (ctypes.c_int * 5)()
    rc = L.pt_atom_cg_route(x, samples, C * H * W if stride is None else stride, state, n, C, H, W, K, out)
    return rc, tuple(out)


def gn_route(L, n, M, Kc, H, W, K, samples=256, stride=None):
    out = (ctypes.c_int * 10)()
    rc = L.pt_atom_gn_route(samples, M * H * W if stride is None else stride, n, M, Kc, H, W, K, out)
    return rc, tuple(out)


def cg_cells(route):
    if route[0] == 1:
        _, tiles, tail, _, kspl = route
        return {("geo", tiles, tail), ("slices", int(tail == LEFT), 8 if kspl <= 8 else kspl)}
    return {("generic", route[1], route[2])}


def gn_cell(route):
    return route[0], route[1]


def cg_layout(c):
    """(bytes off a 256-byte aligned sample base, sample stride in floats, bytes off an aligned cg_state) of a CG case"""
    dense = c.C * c.H * c.W
    return (4 if c.edge == "mis_base" else 0, 2 * dense if c.edge == "view" else dense + 1 if c.edge == "stride1" else dense,
            4 if c.edge == "mis_state" else 0)


def gn_layout(c):
    dense = c.M * c.H * c.W
    return 4 if c.edge == "mis_base" else 0, 2 * dense if c.edge == "view" else dense + 1 if c.edge == "stride1" else dense


def cg_case_route(L, c):
    off, stride, soff = cg_layout(c)
    return cg_route(L, c.n, c.C, c.H, c.W, c.K, samples=256 + off, stride=stride, state=256 + soff)


def gn_case_route(L, c):
    off, stride = gn_layout(c)
    return gn_route(L, c.n, c.M, c.Kc, c.H, c.W, c.K, samples=256 + off, stride=stride)


# ---- the problems and their float64 / fp32 restatements ----------------------------------------------------------------------------------
def cg_problem(c):
    """fp32 (x0, samples, y, sw) of a CG case"""
    x0, samples, y, sw = synth.atom_problem(c.seed, c.n, CFG, small=dict(C=c.C, H=c.H, W=c.W, K=c.K))
    if c.edge == "zero_tail":
        samples[c.n - c.arg:] = 0
        sw = sw.copy()
        sw[c.n - c.arg:] = 0
    if c.edge == "zero_rhs":
        samples[:] = 0
        x0[:] = 0
    return x0, samples, y, sw


def cg_run(c, dtype, problem=None, defect=None, trace=None):
    """OrderedDict {"call k": x after run() call k} of oracle.np_oracle.atom_cg in `dtype`.  defect: one of O.ATOM_CG_DEFECTS, or
    "drop_state" (the state is dropped in front of the second call although forget != 0)."""
    x0, samples, y, sw = (a.astype(dtype) for a in (problem or cg_problem(c)))
    fr, forget = c.variant
    x, state, out = x0, None, OrderedDict()
    for k, iters in enumerate(c.calls):
        if defect == "drop_state" and k == 1:
            state = None
        tr = None if trace is None else []
        x, state = O.atom_cg(x, samples, y, sw, filter_reg=CFG["filter_reg"], act_min_val=CFG["act_min_val"], num_iter=iters,
                             fletcher_reeves=fr, state=state, direction_forget_factor=forget,
                             defect=None if defect == "drop_state" else defect, trace=tr)
        if trace is not None:
            trace.append(tr)
        out[f"call {k}"] = x
    return out


def gn_problem(c):
    """fp32 (f0, P0, samples, y, sw (n,)) of a GN case; "first-frame" is tests/test_gpu_parity.py's first-frame-size problem"""
    rng = np.random.default_rng(c.seed)
    samples = rng.standard_normal((c.n, c.M, c.H, c.W), dtype=np.float32) * np.float32(0.1)
    _, _, y, sw = synth.atom_problem(c.seed, c.n, CFG, small=dict(C=c.Kc, H=c.H, W=c.W))
    f0 = np.zeros((c.Kc, c.K, c.K), np.float32) if c.zero_f0 else rng.standard_normal((c.Kc, c.K, c.K), dtype=np.float32) * np.float32(0.05)
    P0 = rng.standard_normal((c.Kc, c.M), dtype=np.float32) * np.float32(1.0 / np.sqrt(c.M))
    if c.one_weight:
        sw = np.full(c.n, np.float32(1.0 / c.n), np.float32)
    return f0, P0, samples, y, sw


PROJECTION_REG = 1e-4


def gn_run(c, dtype, problem=None, defect=None, trace=None):
    f0, P0, samples, y, sw = (a.astype(dtype) for a in (problem or gn_problem(c)))
    f, P = O.atom_gn_cg(f0, P0, samples, y, sw, filter_reg=CFG["filter_reg"], projection_reg=PROJECTION_REG, act_min_val=CFG["act_min_val"],
                        cg_iters=list(c.iters), fletcher_reeves=c.fr, defect=defect, trace=trace)
    return OrderedDict((("filter", f), ("projection", P)))
