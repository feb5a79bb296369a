"""Every kernel route of ATOM's conjugate-gradient update (csrc/atom_cg.hip) and first-frame joint Gauss-Newton (csrc/atom_gn.hip) on the
MI355X: the cases of tests/atom_cases.py through pytracking_amd.optimization (the C entry where the Python layer cannot express the
case), each asserted onto its pinned route through pt_atom_cg_route / pt_atom_gn_route before it launches, against oracle.np_oracle in
float64 under tests/f64_bound.py's bound

    |out - float64| <= FACTOR x max(the fp32 restatement's own distance from float64 on that case, one fp32 spacing of the output's range)

CG: x after every run() call, one bound per call; GN: filter and projection, one bound each.  The zero right-hand side must give back x0
exactly.  Every test prints its figures before it asserts (run with -s); with ATOM_ROUTES_F64_OUT set the table is written to that file
(profiles/atom_routes_f64.txt).  Needs no reference tree."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import atom_cases as AC
import f64_bound
from conftest import load_golden
from pytracking_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# worst measured ratio on the MI355X: see profiles/atom_routes_f64.txt (below FACTOR / 2: the project's factor stands)
FACTOR = f64_bound.FACTOR
TABLE = f64_bound.Table("ATOM_ROUTES_F64_OUT",
                        "ATOM conjugate-gradient update and joint Gauss-Newton on gfx950 against float64 (tests/test_gpu_atom_routes.py -s), every\n"
                        "case of tests/atom_cases.py on its pinned kernel route.  err = max |out - float64 oracle| of x after a run() call (cg) or of\n"
                        "the filter / projection (gn), ref_err = the fp32 oracle's own distance from float64, floor = one fp32 spacing of the output's\n"
                        f"range, ratio = err / max(ref_err, floor); bound {FACTOR}.  `fold`: the same case in a child process with PT_ACG_FOLD=1.")
_ident = lambda q: q


def _samples_on_device(samples, edge):
    """the case's sample tensor: dense and 256-byte aligned, or the view / offset / stride its edge names"""
    n = samples.shape[0]
    dense = samples[0].size
    src = torch.from_numpy(samples)
    if edge == "view":
        big = torch.full((n, 2 * samples.shape[1]) + samples.shape[2:], 1e3, device=DEV)
        sd = big[:, :samples.shape[1]]
    elif edge == "mis_base":
        sd = torch.zeros(n * dense + 1, device=DEV)[1:].view(samples.shape)
    elif edge == "stride1":
        sd = torch.as_strided(torch.zeros(n * (dense + 1), device=DEV), samples.shape, (dense + 1,) + src.stride()[1:])
    else:
        sd = torch.empty(samples.shape, device=DEV)
    sd.copy_(src)
    return sd


def _cg_device(c, problem):
    """{"call k": x after run() call k} (numpy) of the case on the device, after the query has confirmed its route"""
    from pytracking_amd.filter import _ptr, _stream, workspace
    from pytracking_amd.optimization import ConjugateGradient, ConvProblem, MLU
    x0, samples, y, sw = problem
    L = _lib.lib()
    CKK = c.C * c.K * c.K
    sd = _samples_on_device(samples, c.edge)
    x = torch.from_numpy(x0.copy())[None].to(DEV)
    yd, swd = torch.from_numpy(y).to(DEV), torch.from_numpy(sw).to(DEV)
    state = torch.zeros(2 * CKK + 8, device=DEV)
    state = state[1:1 + 2 * CKK + 4] if c.edge == "mis_state" else state[:2 * CKK + 4]
    off, stride, soff = AC.cg_layout(c)
    assert (sd.data_ptr() % 16, sd.stride(0), state.data_ptr() % 16) == (off, stride, soff) and sd.stride()[1:] == (c.H * c.W, c.W, 1)
    route = AC.cg_route(L, c.n, c.C, c.H, c.W, c.K, x=x.data_ptr(), samples=sd.data_ptr(), stride=sd.stride(0), state=state.data_ptr())
    assert route == (0, c.route), (c.name, route)
    fr, forget = c.variant
    out = OrderedDict()
    if c.edge == "mis_state":                      # the Python layer allocates its own (aligned) state
        ws = workspace(L.pt_atom_cg_ws_bytes(c.n, c.C, c.H, c.W, c.K), x.device)
        for k, iters in enumerate(c.calls):
            rc = L.pt_atom_cg_f32(_ptr(x), _ptr(sd), sd.stride(0), _ptr(yd), _ptr(swd), AC.CFG["filter_reg"], AC.CFG["act_min_val"], c.n, c.C,
                                  c.H, c.W, c.K, iters, int(fr), forget, _ptr(state), _ptr(ws), ws.numel(), _stream())
            assert rc == 0, rc
            out[f"call {k}"] = x[0].cpu().numpy()
        return out
    opt = ConjugateGradient(ConvProblem([sd], [yd[:, None]], [AC.CFG["filter_reg"]], [swd], MLU(AC.CFG["act_min_val"])), [x],
                            fletcher_reeves=fr, direction_forget_factor=forget)
    opt._state = state                             # the buffer run() would allocate, so that the query sees its address
    for k, iters in enumerate(c.calls):
        opt.run(iters)
        assert opt._state is state
        out[f"call {k}"] = x[0].cpu().numpy()
    return out


def _cg_anchor(c):
    return f64_bound.anchor(("atom_cg", c.name), lambda dt: AC.cg_run(c, dt), group=_ident)


def _hold(tag, c, got, a):
    """every output (x after a call; filter, projection) within the bound of its own ref_err and floor"""
    for q, want in a.want.items():
        f64_bound.held(f"{tag} {c.name} {q}", got[q], want, a.ref_errs[q], factor=FACTOR, floor=f64_bound.spacing_of_max, table=TABLE,
                       msg=f"route {c.route}")


def _hold_cg(c, got, tag="cg"):
    _hold(tag, c, got, _cg_anchor(c))


@pytest.mark.parametrize("c", [c for c in AC.CG_CASES if c.edge != "zero_rhs"], ids=lambda c: c.name)
def test_cg_case_matches_float64(c):
    got = _cg_device(c, AC.cg_problem(c))
    _hold_cg(c, got)
    if c.name.startswith("golden-"):               # and the reference's own run, at the flat bound of the other golden tests
        g = load_golden("atom_cg_c64_fused")
        tag = c.name.split("-")[1]
        assert (int(g["seed"]), int(g["n"]), int(g["H"]), int(g["W"])) == (c.seed, c.n, c.H, c.W) and tuple(g["iters"]) == c.calls
        assert (bool(int(g[f"{tag}_fr"])), float(g[f"{tag}_forget"])) == c.variant
        for k in range(len(c.calls)):
            np.testing.assert_allclose(got[f"call {k}"].astype(np.float64), g[f"{tag}_x_out"][k].astype(np.float64), atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("c", [c for c in AC.CG_CASES if c.edge == "zero_rhs"], ids=lambda c: c.name)
def test_cg_zero_right_hand_side_returns_x0(c):
    """samples = 0, x0 = 0: the right-hand side is zero, the solve stops at rho == 0 (optimization.py:108-113) in every call and x stays x0,
    finite, whatever the carried state."""
    problem = AC.cg_problem(c)
    got = _cg_device(c, problem)
    for k, x in got.items():
        print(f"\ncg {c.name} {k}: max |x| {float(np.abs(x).max())!r}, finite {bool(np.isfinite(x).all())}")
    for k, x in got.items():
        assert np.isfinite(x).all() and np.array_equal(x, problem[0]), (c.name, k)


def _fold_child(path):
    """the PT_ACG_FOLD=1 child: the four cases on the device, outputs to `path`"""
    by = {c.name: c for c in AC.CG_CASES}
    out = {}
    for name in AC.CG_FOLD:
        for k, x in _cg_device(by[name], AC.cg_problem(by[name])).items():
            out[f"{name}__{k.split()[1]}"] = x
    np.savez(path, **out)


def test_cg_folded_partial_sums_match_float64(tmp_path):
    """The experiment kept behind PT_ACG_FOLD=1 (k_acg_fwd<., true>, k_acg_final_fold) on four fused cases -- LEFT and not, up to 8 and 64
    slices, PR with forgetting and FR, the state carried -- in a child process with the knob on, under the same bound."""
    path = str(tmp_path / "fold.npz")
    code = f"import sys;sys.path.insert(0,'tests');sys.path.insert(0,'.');import test_gpu_atom_routes as G;G._fold_child({path!r});print('FOLD_DONE')"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PT_ACG_FOLD="1"), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "FOLD_DONE" in res.stdout, res.stderr[-2000:]
    by = {c.name: c for c in AC.CG_CASES}
    with np.load(path) as z:
        for name in AC.CG_FOLD:
            _hold_cg(by[name], OrderedDict((f"call {k}", z[f"{name}__{k}"]) for k in range(len(by[name].calls))), tag="cg fold")


def _gn_device(c, problem):
    import torch.nn.functional as F
    from pytracking_amd.optimization import FactorizedConvProblem, GaussNewtonCG
    f0, P0, samples, y, sw = problem
    sd = _samples_on_device(samples, c.edge)
    off, stride = AC.gn_layout(c)
    assert (sd.data_ptr() % 16, sd.stride(0)) == (off, stride)
    route = AC.gn_route(_lib.lib(), c.n, c.M, c.Kc, c.H, c.W, c.K, samples=sd.data_ptr(), stride=sd.stride(0))
    assert route == (0, c.route), (c.name, route)
    swd = torch.tensor([1.0 / c.n], device=DEV) if c.one_weight else torch.from_numpy(sw).to(DEV)
    a = AC.CFG["act_min_val"]
    prob = FactorizedConvProblem([sd], [torch.from_numpy(y).to(DEV)[:, None]], [AC.CFG["filter_reg"]], [AC.PROJECTION_REG], None, [swd],
                                 lambda x: x, lambda x: F.elu(F.leaky_relu(x, 1 / a), a))
    filt = torch.from_numpy(f0.copy())[None].to(DEV)
    proj = torch.from_numpy(P0.copy())[:, :, None, None].to(DEV)
    assert filt.data_ptr() % 16 == 0 and proj.data_ptr() % 16 == 0
    GaussNewtonCG(prob, [filt, proj], fletcher_reeves=c.fr).run(list(c.iters))
    return OrderedDict((("filter", filt[0].cpu().numpy()), ("projection", proj[:, :, 0, 0].cpu().numpy())))


@pytest.mark.parametrize("c", AC.GN_CASES, ids=lambda c: c.name)
def test_gn_case_matches_float64(c):
    got = _gn_device(c, AC.gn_problem(c))
    a = f64_bound.anchor(("atom_gn", c.name), lambda dt: AC.gn_run(c, dt), group=_ident)
    _hold("gn", c, got, a)
