"""The ToMP model predictor on the MI355X against float64, on every kernel route its launchers can pick (tests/tomp_cases.py: the case
table with the route list each case is pinned to; tests/test_tomp_routes_cpu.py shows that the table covers every reachable route).
For each case the mirrored modules (pytracking_amd/transformer.py) produce the filters, the encoded features and, through the parallel
entry point, the classifier's scores and the regressor's boxes; the box regressor and pt_tomp_linear_f32 are also run alone.  Every
output must be finite and lie within F x ref_err of the float64 oracle (tests/tomp_f64.py: ref_err is the fp32 oracle's own distance
from float64 on that case, the committed value), where the golden tests of tests/test_gpu_parity.py allow a flat 1e-4.

Every test prints per output the measured max |gpu - float64| and its ratio to ref_err before it asserts (run with -s)."""
import ctypes

import pytest
import torch

import tomp_cases as TC
import f64_bound
import tomp_f64 as F64
from pytracking_amd import _lib
from pytracking_amd.filter import _ptr, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = lambda a: torch.from_numpy(a).to(DEV)


def _check(name, want, got):
    assert set(got) == set(want)
    for q, t in got.items():
        assert t.numel() == want[q].size and bool(torch.isfinite(t).all()), q          # finite before anything is compared
    f64_bound.held(name, got, want, TC.REF_ERR[name], F64.F, group=F64.group)


@pytest.mark.parametrize("name", list(TC.PREDICT))
def test_predictor_case_within_the_float64_bound(name):
    cfg, params, inputs = TC.predict_case(name)
    assert TC.case_routes(_lib.lib(), name) == (0, TC.ROUTES[name])                    # the library under test picks the pinned routes
    pred, cls, reg = TC.build_tomp_modules(cfg, params, DEV)
    train, test, lab, ltrb = [T(a) for a in inputs]
    with torch.no_grad():
        if cfg["mode"] == "parallel":
            cw, bw, cenc, benc = pred.predict_cls_bbreg_filters_parallel(train, test, lab, cfg["num_gth_frames"], ltrb)
            got = dict(cls_filter=cw, bbreg_filter=bw, cls_enc=cenc, bbreg_enc=benc, scores=cls(cenc, cw), ltrb=reg(benc, bw))
        else:
            w, enc = pred.predict_filter(train, test, lab, ltrb)
            got = dict(filter=w, enc=enc)
    torch.cuda.synchronize()
    _check(name, F64.anchor("predict", name).want, got)


@pytest.mark.parametrize("name", list(TC.BBREG))
def test_box_regressor_case_within_the_float64_bound(name):
    n, D, H, W, params, feat, filt = TC.bbreg_case(name)
    assert TC.bbreg_routes(_lib.lib(), n, D, H, W) == (0, TC.ROUTES[name])
    reg = TC.build_regressor(D, params, DEV)
    with torch.no_grad():
        got = dict(ltrb=reg(T(feat), T(filt).reshape(1, D, 1, 1)))
    torch.cuda.synchronize()
    _check(name, F64.anchor("bbreg", name).want, got)


@pytest.mark.parametrize("name", list(TC.LINEAR))
def test_linear_case_within_the_float64_bound(name):
    B, N, K, bias, relu, w, b, x = TC.linear_case(name)
    L = _lib.lib()
    assert TC.linear_routes(L, B, N, K) == (0, TC.ROUTES[name])
    wd, xd, bd = T(w), T(x), T(b) if bias else None
    y = torch.full((B, N), float("nan"), dtype=torch.float32, device=DEV)              # an element the grid's tail skips stays NaN
    with torch.cuda.device(0):
        rc = L.pt_tomp_linear_f32(_ptr(wd), _ptr(bd) if bias else None, _ptr(xd), _ptr(y), B, N, K, int(relu), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _check(name, F64.anchor("linear", name).want, dict(y=y))


def test_module_refuses_what_the_abi_refuses():
    """19x19 maps with three memory frames are over the LDS limit of k_dec_ctx: pt_tomp_predict_ws_bytes returns 0 and the mirror raises
    before anything is launched; so do nine sequences."""
    cfg = TC._p(256, 8, 256, 19, 19, 3, "filter")
    pred, _, _ = TC.build_tomp_modules(cfg, TC.synth.tomp_params(1, cfg), DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(NotImplementedError):
        pred.predict_filter(z(3, 1, 256, 19, 19), z(1, 1, 256, 19, 19), z(3, 1, 19, 19), z(3, 1, 4, 19, 19))
    with pytest.raises(NotImplementedError):
        pred.predict_filter(z(1, 9, 256, 5, 5), z(1, 9, 256, 5, 5), z(1, 9, 5, 5), z(1, 9, 4, 5, 5))
    d = pred._dims(19, 19)
    assert _lib.lib().pt_tomp_predict_ws_bytes(ctypes.byref(d), 3, 1, 0) == 0
