"""The TaMOs multi-object filter predictor on the MI355X (pt_tamos_* of pytracking_amd/csrc/tomp.hip through pytracking_amd/tamos.py)
against float64, on every case of tests/tamos_cases.py (tests/test_tamos_cpu.py shows that the table covers every reachable route).
Per case the mirror produces the filters and the encoded maps, and LinearFilterClassifier the T score maps per sequence; every output
must be finite and lie within F x ref_err of the float64 restatement (tests/tamos_f64.py; ref_err is the fp32 restatement's own distance
from float64 on that case, the committed value), the inputs must be bit-unchanged, a second call must return the same bits, and the
library must pick the pinned routes.  The C ABI is also called directly into NaN-prefilled buffers, captured and replayed in a graph, and
the deployed case compared with the reference's own output (tests/golden/tamos_deployed.npz).

Every test prints per output the measured max |gpu - float64| and its ratio to ref_err before it asserts (run with -s)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tamos_cases as TC
import f64_bound
import tamos_f64 as F64
from pytracking_amd import _lib
from pytracking_amd.filter import _ptr, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def _mirror(pred, cls, cfg, tr, te, lb, lt):
    T = cfg["T"]
    with torch.no_grad():
        if cfg["mode"] == "parallel":
            cw, bw, ce, be = pred.predict_cls_bbreg_filters_parallel(tr, te, lb, cfg["num_gth_frames"], lt)
            assert tuple(cw.shape) == tuple(bw.shape) == (1, T, cfg["D"], 1, 1) and tuple(ce.shape) == tuple(be.shape) == tuple(te.shape)
            return dict(cls_filter=cw, bbreg_filter=bw, cls_enc=ce, bbreg_enc=be, scores=cls(ce, cw))
        w, enc = pred.predict_filter(tr, te, lb, lt)
        assert tuple(w.shape) == (cfg["n_seq"], T, cfg["D"], 1, 1) and tuple(enc.shape) == tuple(te.shape)
        return dict(filter=w, enc=enc, scores=cls(enc, w))


def run(name):
    """The mirror's outputs of a case, computed once per session (two calls: the second must repeat the first bit for bit)."""
    if name not in _RUNS:
        cfg, params, inputs = TC.case(name)
        pred, cls = TC.build_modules(cfg, params, DEV)
        dev_in = [torch.from_numpy(a.copy()).to(DEV) for a in inputs]
        keep = [t.clone() for t in dev_in]
        got = _mirror(pred, cls, cfg, *dev_in)
        got = {q: t.clone() for q, t in got.items()}
        again = _mirror(pred, cls, cfg, *dev_in)
        torch.cuda.synchronize()
        _RUNS[name] = (got, again, all(torch.equal(a, b) for a, b in zip(dev_in, keep)))
    return _RUNS[name]


@pytest.mark.parametrize("name", list(TC.CASES))
def test_case_within_the_float64_bound(name):
    cfg = TC.CASES[name]
    assert TC.case_routes(_lib.lib(), name) == (0, TC.ROUTES[name])                     # the library under test picks the pinned routes
    got, again, inputs_unchanged = run(name)
    want = F64.anchor(name).want
    assert set(got) == set(want)
    for q, t in got.items():
        assert t.numel() == want[q].size and bool(torch.isfinite(t).all()), q
        assert torch.equal(t, again[q]), q                                               # no atomics: the same inputs give the same bits
    assert inputs_unchanged
    assert tuple(got["scores"].shape) == (1, cfg["n_seq"], cfg["T"], cfg["H"], cfg["W"])
    f64_bound.held(name, got, want, TC.REF_ERR[name], F64.F, group=F64.group)


def _abi(cfg, params, inputs, parallel, gth, stream_call=None):
    """pt_tamos_predict_f32 called directly; filters / enc prefilled with NaN.  -> (call, filters, enc): call() queues one prediction."""
    L = _lib.lib()
    pred, _ = TC.build_modules(cfg, params, DEV)
    tr, te, lb, lt = [torch.from_numpy(a.copy()).to(DEV) for a in inputs]
    d = TC.dims(cfg)
    T, D, H, W = cfg["T"], cfg["D"], cfg["H"], cfg["W"]
    B = 2 if parallel else cfg["n_seq"]
    nb = L.pt_tamos_predict_ws_bytes(ctypes.byref(d), T, cfg["n_train"], cfg["n_seq"], int(parallel))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    filters = torch.full((B, T, D), float("nan"), device=DEV)
    enc = torch.full((B, D, H, W), float("nan"), device=DEV)
    with torch.cuda.device(0):
        pack, prepared = pred._params()
        pos = pred._pos_table(H, W, torch.device(DEV))
    torch.cuda.synchronize()

    def call():
        rc = L.pt_tamos_predict_f32(ctypes.byref(d), T, _ptr(pack), _ptr(prepared), _ptr(pos), _ptr(tr), _ptr(te), _ptr(lb), _ptr(lt),
                                    cfg["n_train"], cfg["n_seq"], int(parallel), gth, _ptr(filters), _ptr(enc), _ptr(ws), nb, _stream())
        assert rc == 0
    return call, filters, enc, (pack, prepared, pos, tr, te, lb, lt, ws)


@pytest.mark.parametrize("name", ["base_t11", "mask9_gth2", "seq8"])
def test_abi_fills_nan_prefilled_outputs(name):
    """The entry point itself: every element of both outputs is written (the mirror's shortcut for num_gth_frames == n_train never reaches
    the parallel form with an empty mask; here it runs)."""
    cfg, params, inputs = TC.case(name)
    par = cfg["mode"] == "parallel"
    call, filters, enc, _keep = _abi(cfg, params, inputs, par, cfg["num_gth_frames"])
    with torch.cuda.device(0):
        call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(filters).all()) and bool(torch.isfinite(enc).all())
    want = F64.anchor(name).want
    got = ({"cls_filter": filters[0:1], "bbreg_filter": filters[1:2], "cls_enc": enc[0], "bbreg_enc": enc[1]} if par else {"filter": filters, "enc": enc})
    f64_bound.held(name + " (C ABI)", got, {q: want[q] for q in got}, TC.REF_ERR[name], F64.F, group=F64.group)
    if name == "mask9_gth2":                                     # an empty mask: both batch rows are the same problem
        assert torch.equal(filters[0], filters[1]) and torch.equal(enc[0], enc[1])


def test_graph_replay_equals_the_eager_call():
    cfg, params, inputs = TC.case("mask9_gth1")
    call, filters, enc, _keep = _abi(cfg, params, inputs, True, cfg["num_gth_frames"])
    with torch.cuda.device(0):
        call()
        torch.cuda.synchronize()
        eager = (filters.clone(), enc.clone())
        filters.fill_(float("nan"))
        enc.fill_(float("nan"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        torch.cuda.synchronize()
        filters.fill_(float("nan"))
        enc.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(filters, eager[0]) and torch.equal(enc, eager[1])


def test_deployed_case_equals_the_reference_golden():
    """24 x 36 maps, two memory frames, 10 objects: filters, score maps and the stored stride of the encoded maps against the reference's
    own fp32 and float64 outputs at 1e-4."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"tamos_{TC.DEPLOYED}.npz"))
    got, _, _ = run(TC.DEPLOYED)
    for q, t in got.items():
        v = t.detach().double().cpu().numpy().reshape(-1)
        if q.endswith("enc"):
            v = v[::int(g[f"{q}_stride"])]
        for tag in ("f64", "f32"):
            ref = g[f"{q}_{tag}"].astype(np.float64).reshape(-1)
            err = float(np.abs(v - ref).max())
            print(f"\ndeployed {q} vs reference {tag}: max |gpu - reference| {err:.3e} (values up to {np.abs(ref).max():.2f})")
            assert err <= 1e-4, (q, tag, err)


def test_mirror_raises_before_any_launch_on_what_the_abi_refuses():
    cfg, params, _ = TC.case("seq1")
    pred, _ = TC.build_modules(cfg, params, DEV)
    D, T = cfg["D"], cfg["T"]
    z = lambda *s: torch.zeros(*s, device=DEV)
    d = pred._dims(5, 5)
    assert _lib.lib().pt_tamos_predict_ws_bytes(ctypes.byref(d), T, 1, 9, 0) == 0
    with pytest.raises(NotImplementedError):                     # nine batch rows
        pred.predict_filter(z(1, 9, D, 5, 5), z(1, 9, D, 5, 5), z(1, 9, T, 5, 5), z(1, 9, T, 4, 5, 5))
    assert _lib.lib().pt_tamos_predict_ws_bytes(ctypes.byref(d), T, 2, 2, 1) == 0
    with pytest.raises(NotImplementedError):                     # the parallel form with two sequences
        pred.predict_cls_bbreg_filters_parallel(z(2, 2, D, 5, 5), z(1, 2, D, 5, 5), z(2, 2, T, 5, 5), 1, z(2, 2, T, 4, 5, 5))
    with pytest.raises(ValueError):                              # labels of another object count
        pred.predict_filter(z(1, 1, D, 5, 5), z(1, 1, D, 5, 5), z(1, 1, T + 1, 5, 5), z(1, 1, T + 1, 4, 5, 5))
    with pytest.raises(NotImplementedError):                     # training mode
        pred.train().predict_filter(z(1, 1, D, 5, 5), z(1, 1, D, 5, 5), z(1, 1, T, 5, 5), z(1, 1, T, 4, 5, 5))
