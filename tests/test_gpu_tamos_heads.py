"""The TaMOs heads on the MI355X -- the two-level FPN and the multi-object DenseBoxRegressor (pt_fpn2_f32 / pt_tamos_bbreg_f32 of
pytracking_amd/csrc/tomp.hip through pytracking_amd/tamos.py) -- against float64 on every case of tests/tamos_heads_cases.py.  Every output
must be finite and lie within F x ref_err of float64 (tests/tamos_heads_f64.py; ref_err is the fp32 restatement's own distance from float64
on that case, the committed value), the inputs must be bit-unchanged and a second call must return the same bits.  `want` of the two
deployed cases comes from committed float64 strides (tests/golden/tamos_heads_reg_deployed.npz: the reference's own output;
tamos_heads_fpn_deployed.npz: the float64 restatement).  The C ABI is also called directly into NaN-prefilled buffers, captured and replayed
in a graph, tied to the pinned single-filter path pt_tomp_bbreg_f32 object by object, and chained FPN -> regressor through the two classes.

Every test prints the measured max |gpu - float64| and its ratio to ref_err before it asserts (run with -s)."""
import os

import numpy as np
import pytest
import torch

import tamos_heads_cases as HC
import f64_bound
import tamos_heads_f64 as F64
import tomp_cases as TPC
from f64_bound import dev
from pytracking_amd import _lib
from pytracking_amd.filter import _ptr, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"tamos_heads_{name}.npz"))


def run_reg(name):
    """The mirror's ltrb (1, n_img, T, 4, H, W) of a regressor case, once per session: (first call, second call, inputs unchanged)."""
    if name not in _RUNS:
        n_img, T, D, H, W = HC.REG[name]
        params, feat, filt = HC.reg_case(name)
        reg = HC.build_regressor(D, params, DEV)
        f, w = dev(feat)[None], dev(filt).reshape(n_img, T, D, 1, 1)
        keep = (f.clone(), w.clone())
        with torch.no_grad():
            got = reg(f, w).clone()
            again = reg(f, w)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (1, n_img, T, 4, H, W)
        _RUNS[name] = (got, again, torch.equal(f, keep[0]) and torch.equal(w, keep[1]))
    return _RUNS[name]


def run_fpn(name):
    if name not in _RUNS:
        n, C_hi, C_lo, D, H3, W3, H2, W2 = HC.FPN[name]
        params, hi, lo = HC.fpn_case(name)
        m = HC.build_fpn(name, params, DEV)
        enc, back = dev(lo)[None], {"layer2": dev(hi)}
        keep = (enc.clone(), back["layer2"].clone())
        with torch.no_grad():
            got = {q: t.clone() for q, t in m(enc, back).items()}
            again = m(enc, back)
        torch.cuda.synchronize()
        assert list(got) == ["feat2", "feat3"]
        assert tuple(got["feat2"].shape) == (1, n, D, H2, W2) and tuple(got["feat3"].shape) == (1, n, D, H3, W3)
        _RUNS[name] = (got, again, torch.equal(enc, keep[0]) and torch.equal(back["layer2"], keep[1]))
    return _RUNS[name]


def _check(name, got, again, unchanged, want):
    for q, t in got.items():
        assert bool(torch.isfinite(t).all()), q
        assert torch.equal(t, again[q]), q                         # no atomics: the same inputs give the same bits
    assert unchanged
    f64_bound.held(name, got, want, HC.REF_ERR[name], F64.F)


@pytest.mark.parametrize("name", HC.SMALL_REG)
def test_regressor_within_the_float64_bound(name):
    assert HC.case_routes(_lib.lib(), name) == (0, HC.ROUTES[name])
    got, again, unchanged = run_reg(name)
    _check(name, {"ltrb": got}, {"ltrb": again}, unchanged, F64.anchor(name).want)


@pytest.mark.parametrize("name", HC.SMALL_FPN)
def test_fpn_within_the_float64_bound(name):
    assert HC.case_routes(_lib.lib(), name) == (0, HC.ROUTES[name])
    got, again, unchanged = run_fpn(name)
    _check(name, got, again, unchanged, F64.anchor(name).want)


def test_deployed_regressor_within_the_float64_bound_and_equals_the_reference_golden():
    """48 x 72 map, 10 objects: the stored stride of ltrb against the reference's float64 output at F x ref_err, and against its fp32 and
    float64 outputs at 1e-4."""
    name = HC.REG_DEPLOYED
    assert HC.case_routes(_lib.lib(), name) == (0, HC.ROUTES[name])
    g = golden(name)
    got, again, unchanged = run_reg(name)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, again) and unchanged
    v = got.double().cpu().numpy().reshape(-1)[::int(g["stride"])]
    for tag in ("f64", "f32"):
        err = float(np.abs(v - g[f"ltrb_{tag}"].astype(np.float64)).max())
        print(f"\n{name} vs reference {tag}: max |gpu - reference| {err:.3e} ({err / HC.REF_ERR[name]:.2f}x ref_err {HC.REF_ERR[name]:.3e}, "
              f"bound {F64.F} x ref_err for f64)")
        assert err <= 1e-4, (tag, err)
        assert tag != "f64" or err <= f64_bound.bound(HC.REF_ERR[name], F64.F), err


def test_deployed_fpn_within_the_float64_bound():
    name = HC.FPN_DEPLOYED
    assert HC.case_routes(_lib.lib(), name) == (0, HC.ROUTES[name])
    g = golden("fpn_deployed")
    got, again, unchanged = run_fpn(name)
    assert unchanged
    for q, t in got.items():
        assert bool(torch.isfinite(t).all()) and torch.equal(t, again[q]), q
        err = float(np.abs(t.double().cpu().numpy().reshape(-1)[::int(g[f"{q}_stride"])] - g[f"{q}_f64"]).max())
        print(f"\n{name} {q}: max |gpu - float64| {err:.3e} ({err / HC.REF_ERR[name]:.2f}x ref_err {HC.REF_ERR[name]:.3e}, bound {F64.F} x)")
        assert err <= f64_bound.bound(HC.REF_ERR[name], F64.F), (q, err)


def _reg_abi(name):
    n_img, T, D, H, W = HC.REG[name]
    params, feat, filt = HC.reg_case(name)
    L = _lib.lib()
    reg = HC.build_regressor(D, params, DEV)
    with torch.cuda.device(0):
        pack = reg._params()
    f, w = dev(feat), dev(filt)
    nb = L.pt_tamos_bbreg_ws_bytes(n_img, T, D, H, W)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((n_img, T, 4, H, W), float("nan"), device=DEV)
    torch.cuda.synchronize()

    def call():
        assert L.pt_tamos_bbreg_f32(_ptr(pack), _ptr(f), _ptr(w), _ptr(out), n_img, T, D, H, W, _ptr(ws), nb, _stream()) == 0
    return call, out, (pack, f, w, ws, reg)


@pytest.mark.parametrize("name", ["reg_d64_5x7_t3", "reg_d256_12x18_t16", "reg_d128_5x7_t3_n2"])
def test_regressor_abi_fills_nan_prefilled_output(name):
    call, out, _keep = _reg_abi(name)
    with torch.cuda.device(0):
        call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    f64_bound.held(name + " (C ABI)", {"ltrb": out}, F64.anchor(name).want, HC.REF_ERR[name], F64.F)


@pytest.mark.parametrize("name", ["fpn_odd", "fpn_d256"])
def test_fpn_abi_fills_nan_prefilled_outputs_and_skips_feat3_on_request(name):
    n, C_hi, C_lo, D, H3, W3, H2, W2 = HC.FPN[name]
    params, hi, lo = HC.fpn_case(name)
    L = _lib.lib()
    m = HC.build_fpn(name, params, DEV)
    with torch.cuda.device(0):
        pack = m._params()
    h, l = dev(hi), dev(lo)
    nb = L.pt_fpn2_ws_bytes(n, C_hi, C_lo, D, H2, W2, H3, W3)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    want = F64.anchor(name).want
    for want3 in (1, 0):
        f2 = torch.full((n, D, H2, W2), float("nan"), device=DEV)
        f3 = torch.full((n, D, H3, W3), float("nan"), device=DEV)
        with torch.cuda.device(0):
            rc = L.pt_fpn2_f32(_ptr(pack), _ptr(h), _ptr(l), _ptr(f2), _ptr(f3), n, C_hi, C_lo, D, H2, W2, H3, W3, want3, _ptr(ws), nb, _stream())
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isfinite(f2).all())
        got = {"feat2": f2}
        if want3:
            assert bool(torch.isfinite(f3).all())
            got["feat3"] = f3
        else:
            assert bool(torch.isnan(f3).all())                       # skipped: left as it was
        f64_bound.held(f"{name} (C ABI, want_feat3={want3})", got, {q: want[q] for q in got}, HC.REF_ERR[name], F64.F)


def test_graph_replay_equals_the_eager_call():
    call, out, _keep = _reg_abi("reg_d128_9x13_t10")
    with torch.cuda.device(0):
        call()
        torch.cuda.synchronize()
        eager = out.clone()
        out.fill_(float("nan"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        torch.cuda.synchronize()
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("name", HC.SMALL_REG)
def test_each_object_equals_the_single_filter_path(name):
    """Object o of the multi-object call against the parent commit's pinned path, pt_tomp_bbreg_f32 (through the parent class) run with that
    object's filter alone, within F x ref_err of each other."""
    n_img, T, D, H, W = HC.REG[name]
    params, feat, filt = HC.reg_case(name)
    got, _, _ = run_reg(name)
    single = TPC.build_regressor(D, {"reg." + k: v for k, v in params.items()}, DEV)
    worst = 0.0
    with torch.no_grad():
        for i in range(n_img):
            for o in range(T):
                one = single(dev(feat[i:i + 1])[None], dev(filt[i, o]).reshape(1, D, 1, 1))
                assert tuple(one.shape) == (1, 1, 4, H, W)
                worst = max(worst, float((one[0, 0].double() - got[0, i, o].double()).abs().max()))
    print(f"\n{name}: max |multi-object - single-filter path| {worst:.3e} ({worst / HC.REF_ERR[name]:.2f}x ref_err)")
    assert worst <= f64_bound.bound(HC.REF_ERR[name], F64.F), worst


def test_fpn_to_regressor_chain_through_the_classes():
    name = "chain_odd_t3"
    fname, rp, filt = HC.chain_case(name)
    n, C_hi, C_lo, D = HC.FPN[fname][:4]
    T = filt.shape[1]
    params, hi, lo = HC.fpn_case(fname)
    fpn, reg = HC.build_fpn(fname, params, DEV), HC.build_regressor(D, rp, DEV)
    with torch.no_grad():
        maps = fpn(dev(lo)[None], {"layer2": dev(hi)})
        ltrb = reg(maps["feat2"], dev(filt).reshape(n, T, D, 1, 1))
    torch.cuda.synchronize()
    got = {"feat2": maps["feat2"], "ltrb": ltrb}
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    f64_bound.held(name, got, F64.anchor(name).want, HC.REF_ERR[name], F64.F)


def test_mirror_raises_before_any_launch_on_what_the_abi_refuses():
    L = _lib.lib()
    params, _, _ = HC.reg_case("reg_d64_5x7_t3")
    reg = HC.build_regressor(64, params, DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    assert L.pt_tamos_bbreg_ws_bytes(1, 17, 64, 5, 7) == 0
    with pytest.raises(NotImplementedError):                     # seventeen filters per sequence
        reg(z(1, 1, 64, 5, 7), z(1, 17, 64, 1, 1))
    with pytest.raises(ValueError):                              # filters of another width
        reg(z(1, 1, 64, 5, 7), z(1, 3, 32, 1, 1))
    with pytest.raises(NotImplementedError):                     # CPU tensors: no stock fallback
        reg.cpu()(torch.zeros(1, 1, 64, 5, 7), torch.zeros(1, 3, 64, 1, 1))
    reg.to(DEV)
    with pytest.raises(NotImplementedError):                     # training mode
        reg.train()(z(1, 1, 64, 5, 7), z(1, 3, 64, 1, 1))
    fparams, _, _ = HC.fpn_case("fpn_x2")
    fpn = HC.build_fpn("fpn_x2", fparams, DEV)
    with pytest.raises(ValueError):                              # a high-resolution map of another width
        fpn(z(1, 1, 64, 5, 7), {"layer2": z(1, 64, 10, 14)})
    with pytest.raises(NotImplementedError):
        fpn.train()(z(1, 1, 64, 5, 7), {"layer2": z(1, 128, 10, 14)})
    from pytracking_amd import tamos as TA
    assert L.pt_fpn2_param_floats(96, 64, 64) == 0
    with pytest.raises(NotImplementedError):                     # channel counts the kernels do not take
        TA.FPN(output_dim=64, input_dims=(96, 64))
