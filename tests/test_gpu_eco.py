"""ECO's Fourier-domain per-frame path on the MI355X (pytracking_amd/eco.py, eco.hip): sample transform, shift, filter response,
localisation and memory insert against the float64 restatements of tests/eco_cases.py, the closed per-frame loop (eager and as captured
graphs) and the unmodified reference ECO through install(eco=True).

Bounds are the project's (tests/f64_bound.py): an fp32 output lies within FACTOR x max(ref_fp32_err, 2^-23 max |want|) of float64, where
ref_fp32_err is the error of the unmodified reference's own fp32 run recorded in the golden (tests/golden/eco_*.npz, written by
tools/make_golden_eco.py from the reference on the torch.rfft / torch.irfft shim that tests/test_eco_cpu.py verifies), and within 1e-4 of
the golden; arg-max positions, scale indices and slots are compared exactly.  Where there is no golden (a score grid equal to the series,
which the reference evaluates on 2 Wh - 2 columns; the closed loop; the tracker run) ref_fp32_err is the error of pytracking_amd.eco's
torch form in fp32 on the same inputs.  Every test prints its measured ratio before it asserts (run with -s); when ECO_F64_OUT names a
file the ratios are written there as a table (profiles/eco_f64.txt is the table of such a run)."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import eco_cases as EC  # noqa: E402
import f64_bound  # noqa: E402
from f64_bound import host, needs_bundle  # noqa: E402
from oracle import ref_harness  # noqa: E402
from pytracking_amd import eco  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE = f64_bound.Table("ECO_F64_OUT",
                        "ECO Fourier-domain path on gfx950: max |out - float64| per case, as a multiple of max(ref_fp32_err, 2^-23 max |want|)\n"
                        f"(bound: {f64_bound.FACTOR}); ref_fp32_err: the unmodified reference's own fp32 error (golden) or, marked *, the torch form's")
dev = functools.partial(f64_bound.dev, device=DEV, dtype=torch.float32)


@pytest.fixture(scope="module")
def g_sample():
    return np.load(os.path.join(EC.GOLDEN, "eco_sample.npz"))


@pytest.fixture(scope="module")
def g_ops():
    return np.load(os.path.join(EC.GOLDEN, "eco_ops.npz"))


def near_golden(g, key, seed, got):
    idx = EC.sample_positions(seed, got.size)
    assert np.abs(got.reshape(-1)[idx] - g[key + "/out"]).max() <= 1e-4, key


# ---- sample transform --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EC.SAMPLE_CASES))
def test_sample_transform(g_sample, case):
    c = EC.SAMPLE_CASES[case]
    x, P, win, interp, shift = EC.sample_inputs(case)
    want = EC.sample_np(x, P, win, interp, shift)
    args = (dev(x), dev(P), dev(win), (dev(interp[0]), dev(interp[1])), shift)
    out = eco.sample_transform(*args)
    assert out.shape == want.shape
    got = host(out)
    f64_bound.held("sample " + case, got, want, g_sample[case + "/ref_fp32_err"], floor=f64_bound.ulp_of_max, table=TABLE)
    near_golden(g_sample, case, c["seed"], got)
    assert torch.equal(eco.sample_transform(*args), out)                                # no atomics: the same bits again


def test_sample_transform_without_window_and_factors_is_cfft2():
    x = EC.sample_inputs("6x9_3to2_S5_plain")[0]
    out = eco.cfft2_device(dev(x))
    want = EC.to_r(EC.cfft2_np(x))
    ref = eco.cfft2(torch.from_numpy(x)).numpy()
    f64_bound.held("cfft2 6x9", host(out), want, np.abs(ref - want).max(), floor=f64_bound.ulp_of_max, table=TABLE, star=True)
    assert torch.equal(out[:, :, 0], out[:, :, -1])                                     # even H: the Nyquist row at both ends


def test_real_interpolation_factors_and_views():
    """Factors without the centring phase are real (1, 1, Hf, 1) / (1, 1, 1, Wh); non-contiguous inputs give the bits of contiguous ones."""
    x, P, win, interp, _ = EC.sample_inputs("5x5_3to2_S5_plain")
    iy, ix = interp[0][..., 0].copy(), interp[1][..., 0].copy()
    want = EC.sample_np(x, P, win, (np.stack((iy, 0 * iy), -1), np.stack((ix, 0 * ix), -1)))
    out = eco.sample_transform(dev(x), dev(P), dev(win), (dev(iy), dev(ix)))
    ref = eco.sample_transform_torch(*[torch.from_numpy(a) for a in (x, P, win)], (torch.from_numpy(iy), torch.from_numpy(ix))).numpy()
    f64_bound.held("sample real factors", host(out), want, np.abs(ref - want).max(), floor=f64_bound.ulp_of_max, table=TABLE, star=True)
    xt = dev(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).transpose(2, 3)
    assert not xt.is_contiguous() and torch.equal(eco.sample_transform(xt, dev(P), dev(win), (dev(iy), dev(ix))), out)


# ---- filter response and localisation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EC.APPLY_CASES))
def test_apply_filter(g_ops, case):
    hf, xf = EC.apply_inputs(case)
    want = EC.apply_filter_np(hf, xf)
    out = eco.apply_filter(dev(hf), dev(xf))
    assert out.shape == want.shape
    f64_bound.held("apply " + case, host(out), want, g_ops[f"apply/{case}/ref_fp32_err"], floor=f64_bound.ulp_of_max, table=TABLE)
    near_golden(g_ops, "apply/" + case, EC.APPLY_CASES[case]["seed"], host(out))
    assert torch.equal(eco.apply_filter(dev(hf), dev(xf)), out)


@pytest.mark.parametrize("case", list(EC.LOC_CASES))
def test_localize(g_ops, case):
    c = EC.LOC_CASES[case]
    sfs = EC.loc_inputs(case)
    want, max_val, argmax = EC.localize_np(sfs, c["weights"], c["grid"])
    scores, mv, am = eco.localize([dev(e) for e in sfs], c["weights"], c["grid"])
    assert scores.shape == want.shape and mv.shape == (c["S"], 1) and am.shape == (c["S"], 1, 2) and am.dtype == torch.int64
    key = f"loc/{case}/scores"
    if key + "/out" in g_ops:
        ref_err, own = float(g_ops[key + "/ref_fp32_err"]), False
        near_golden(g_ops, key, c["seed"], host(scores))
        assert np.array_equal(g_ops[f"loc/{case}/argmax"], am.cpu().numpy())
    else:                                                                               # grid equal to the series: the torch form's fp32 error
        ref_err, own = float(np.abs(eco.localize_torch([torch.from_numpy(e) for e in sfs], c["weights"], c["grid"])[0].numpy() - want).max()), True
    f64_bound.held("localize " + case, host(scores), want, ref_err, floor=f64_bound.ulp_of_max, table=TABLE, star=own)
    f64_bound.held("localize max " + case, host(mv), max_val, ref_err, floor=f64_bound.ulp_of_max, table=TABLE, star=own)
    assert np.array_equal(am.cpu().numpy(), argmax)
    again = eco.localize([dev(e) for e in sfs], c["weights"], c["grid"])
    assert all(torch.equal(a, b) for a, b in zip(again, (scores, mv, am)))


def test_localize_ties_follow_max2d():
    """A constant series has every score equal: column 0, row 0, as torch.max over rows and then over columns gives."""
    sf = torch.zeros(2, 1, 5, 3, 2, device=DEV)
    sf[:, :, 2, 0, 0] = 1.5
    scores, mv, am = eco.localize([sf], None, (8, 6))
    assert torch.equal(scores, torch.full_like(scores, 1.5)) and torch.equal(am.cpu(), torch.zeros(2, 1, 2, dtype=torch.int64))


# ---- shift and memory insert -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EC.INSERT_CASES))
def test_insert(g_ops, case):
    c = EC.INSERT_CASES[case]
    mem, xf = EC.insert_inputs(case)
    want = EC.insert_np(mem, xf, c["ind"], c["shift"])
    m = dev(mem)
    assert eco.insert(m, dev(xf), c["ind"], c["shift"]) is m
    got = m.cpu().numpy()
    f64_bound.held("insert " + case, got.astype(np.float64), want, g_ops[f"insert/{case}/ref_fp32_err"], floor=f64_bound.ulp_of_max, table=TABLE)
    near_golden(g_ops, "insert/" + case, c["seed"], got)
    keep = np.ones(c["n"], dtype=bool)
    keep[c["ind"]] = False
    assert np.array_equal(got[:, :, keep].view(np.uint32), mem[:, :, keep].view(np.uint32))        # bytes outside the slot are unchanged
    if c["shift"] is None:
        assert np.array_equal(got[:, :, c["ind"]], xf[0].transpose(1, 2, 0, 3))
    else:                                                                               # shift_fs on its own gives the slot's bits
        sh = eco.shift_fs(dev(xf), c["shift"])
        assert torch.equal(sh[0].permute(1, 2, 0, 3), m[:, :, c["ind"]])
        assert eco.shift_fs(dev(xf), (0.0, 0.0)).data_ptr() != 0 and torch.equal(eco.shift_fs(dev(xf), (0.0, 0.0)), dev(xf))


# ---- filter update ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g_fu():
    return np.load(os.path.join(EC.GOLDEN, "eco_fu.npz"))


def fu_device(case, calls=None):
    """The case on the kernels -> per call the filters (device clones), the CG state and the live filter tensors."""
    c, d = EC.FU_CASES[case], EC.fu_inputs(case)
    filters, energy = [dev(f) for f in d["filters"]], [dev(e) for e in d["energy"]]
    fixed = [[dev(a) for a in d[k]] for k in ("samples", "weights", "yf", "regs")]
    state = eco.new_cg_state(filters)
    outs = []
    for k, it in enumerate(c["iters"] if calls is None else calls):
        nx = [dev(a) for a in d["new_xf"][k]] if c.get("new_xf", True) else None
        eco.filter_update(filters, *fixed, energy, nx, state, it, d["lrs"], d["reg_energy"], c.get("fr", False), c.get("std_alpha", True),
                          c.get("forget", 0.0))
        outs.append([f.clone() for f in filters])
    return outs, state, filters, energy


@pytest.mark.parametrize("case", list(EC.FU_CASES))
def test_filter_update(g_fu, case):
    c = EC.FU_CASES[case]
    want, want_energy = EC.fu_run_np(case)
    ref = EC.fu_run_np(case, single=True)[0] if c.get("no_ref") else None
    outs, state, filters, energy = fu_device(case)
    assert outs[-1][0].data_ptr() != filters[0].data_ptr() and torch.equal(outs[-1][0], filters[0])        # x is updated in place
    for k, call in enumerate(outs):
        for b, x in enumerate(call):
            key = f"{case}/call{k}/block{b}"
            got = host(x)
            if ref is None:
                assert np.abs(want[k][b].reshape(-1)[EC.sample_positions(c["seed"], got.size)] - g_fu[key + "/want_f64"]).max() <= 1e-10 * float(g_fu[key + "/max_abs"])       # the restatement is the reference's float64
                f64_bound.held("filter_update " + key, got, want[k][b], g_fu[key + "/ref_fp32_err"], floor=f64_bound.ulp_of_max, table=TABLE)
                near_golden(g_fu, key, c["seed"], got)
            else:
                f64_bound.held("filter_update " + key, got, want[k][b], np.abs(ref[k][b] - want[k][b]).max(), floor=f64_bound.ulp_of_max, table=TABLE, star=True)
    if c["iters"][-1] > 0 and c.get("new_xf", True):
        for b, e in enumerate(energy):
            assert np.abs(host(e) - want_energy[b]).max() <= 4 * f64_bound.ulp_of_max(want_energy[b])
    again = fu_device(case)[0]
    assert all(torch.equal(a, b) for ca, cb in zip(again, outs) for a, b in zip(ca, cb))                   # the same call twice: the same bits


def test_filter_update_zero_iterations_touch_nothing():
    outs, state, filters, energy = fu_device("zero_iterations")
    d = EC.fu_inputs("zero_iterations")
    assert np.array_equal(filters[0].cpu().numpy(), d["filters"][0]) and np.array_equal(energy[0].cpu().numpy(), d["energy"][0])
    assert state[0]["state"].tolist() == [1.0, 0.0]


def test_filter_update_joint_early_exit_leaves_x_unchanged():
    """Block 0 has an all-zero weight vector and a zero filter: r = 0, rho is exactly 0 at the top of the first iteration, and the run ends
    for BOTH blocks with x as it stands -- block 1's non-zero filter keeps its bits -- as check_zero does (optimization.py:108-113)."""
    d = EC.fu_inputs("two_blocks")
    d["weights"][0][:] = 0
    d["filters"][0][:] = 0
    filters, energy = [dev(f) for f in d["filters"]], [dev(e) for e in d["energy"]]
    state = eco.new_cg_state(filters)
    eco.filter_update(filters, *[[dev(a) for a in d[k]] for k in ("samples", "weights", "yf", "regs")], energy, [dev(a) for a in d["new_xf"][0]],
                      state, 4, d["lrs"], d["reg_energy"])
    torch.cuda.synchronize()
    assert all(np.array_equal(f.cpu().numpy().view(np.uint32), x.view(np.uint32)) for f, x in zip(filters, d["filters"]))
    assert state[0]["state"].tolist() == [0.0, 0.0] and state[1]["state"][1].item() == 0.0 and state[1]["state"][0].item() > 0   # rho kept, p never made
    opt = EC.FilterOptimNp(d["filters"], d["samples"], d["weights"], d["yf"], d["regs"], d["energy"], d["lrs"], d["reg_energy"])
    opt.run(4, d["new_xf"][0])
    assert opt.p is None and opt.rho[0] == 0 and all(np.array_equal(EC.to_r(x), f.astype(np.float64)) for x, f in zip(opt.x, d["filters"]))


def test_filter_update_is_graph_capturable():
    eager = fu_device("two_blocks")[0]
    d = EC.fu_inputs("two_blocks")
    f0, e0 = [dev(f) for f in d["filters"]], [dev(e) for e in d["energy"]]
    filters, energy = [f.clone() for f in f0], [e.clone() for e in e0]
    fixed = [[dev(a) for a in d[k]] for k in ("samples", "weights", "yf", "regs")]
    nx, state, fresh = [dev(a) for a in d["new_xf"][0]], eco.new_cg_state(f0), eco.new_cg_state(f0)

    def call():
        for dst, src in zip(filters + energy + [s["state"] for s in state], f0 + e0 + [s["state"] for s in fresh]):
            dst.copy_(src)
        eco.filter_update(filters, *fixed, energy, nx, state, 4, d["lrs"], d["reg_energy"])
        return [f.clone() for f in filters]
    captured = GraphOps._replayed(call)
    assert all(torch.equal(a, b) for a, b in zip(captured, eager[0]))


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------
class TorchOps:
    """track_frames on pytracking_amd.eco's torch forms (CPU, fp32): what fp32 costs on the loop in an order of summation nobody tuned."""
    sample_transform = staticmethod(lambda x, P, w, i: eco.sample_transform_torch(x, P, w, i))
    apply_filter = staticmethod(eco.apply_filter_torch)
    localize = staticmethod(eco.localize_torch)
    insert = staticmethod(lambda mem, xf, ind, shift: eco.insert_torch(mem, xf, ind, shift))
    host = staticmethod(lambda t: t.detach().double().cpu().numpy())

    @staticmethod
    def train(state, new_xf, sw, num_iter, forget):
        """The loop's fp32 anchor has no torch form of the solver: the float64 restatement's fp32 mode (tests/eco_cases.py) on the fp32 state."""
        f32 = lambda ts: [t.numpy() for t in ts]      # noqa: E731
        opt = EC.FilterOptimNp(f32(state["filter"]), f32(state["memory"]), [sw.astype(np.float32)] * len(new_xf), f32(state["yf"]), f32(state["regs"]),
                               f32(state["energy"]), state["lrs"], state["reg_energy"], forget=forget, single=True)
        if state["cg"] is not None:
            opt.p, opt.rho, opt.r_prev = state["cg"]
        opt.run(num_iter, f32(new_xf))
        state["cg"] = (opt.p, opt.rho, opt.r_prev)
        for f, x, e, en in zip(state["filter"], opt.x, state["energy"], opt.energy):
            f.copy_(torch.from_numpy(EC.to_r(x).astype(np.float32)))
            e.copy_(torch.from_numpy(en.astype(np.float32)))


class HipOps(TorchOps):
    sample_transform = staticmethod(lambda x, P, w, i: eco.sample_transform(x, P, w, i))
    apply_filter = staticmethod(eco.apply_filter)
    localize = staticmethod(eco.localize)
    insert = staticmethod(lambda mem, xf, ind, shift: eco.insert(mem, xf, ind, shift))

    @staticmethod
    def train(state, new_xf, sw, num_iter, forget):
        if state["cg"] is None:
            state["cg"] = eco.new_cg_state(state["filter"])
        w = dev(sw.astype(np.float32))
        eco.filter_update(state["filter"], state["memory"], [w] * len(new_xf), state["yf"], state["regs"], state["energy"], new_xf, state["cg"],
                          num_iter, state["lrs"], state["reg_energy"], direction_forget_factor=forget)


class GraphOps(HipOps):
    """Every device section of a frame -- transform + response + localisation, then the inserts -- replayed from a captured graph."""
    @staticmethod
    def _replayed(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                                                        # warm-up: kernels loaded before the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        graph.replay()
        torch.cuda.synchronize()
        return out

    @staticmethod
    def insert(mem, xf, ind, shift):
        keep = mem.clone()
        GraphOps._replayed(lambda: eco.insert(mem, xf, ind, shift))                     # warm-up, capture and replay write the same slot
        rest = [j for j in range(mem.shape[2]) if j != ind]
        assert torch.equal(mem[:, :, rest], keep[:, :, rest])


@pytest.fixture(scope="module")
def loop_anchor():
    feats = [EC.loop_features(t) for t in range(EC.LOOP["frames"])]
    want = EC.track_frames(EC.NumpyOps, EC.loop_state(), feats)
    ref = EC.track_frames(TorchOps, EC.loop_state(torch.from_numpy), feats, xp=torch.from_numpy)
    return feats, want, ref


def run_loop(ops, feats):
    with torch.no_grad():
        return EC.track_frames(ops, EC.loop_state(dev), feats, xp=dev)


def check_loop(tag, got, want, ref):
    (log, mems), (wlog, wmems), (rlog, rmems) = got, want, ref
    assert [e["scale_ind"] for e in log] == [e["scale_ind"] for e in wlog] and [e["slot"] for e in log] == [e["slot"] for e in wlog]
    assert len({e["slot"] for e in log}) >= 3
    boxes, wboxes = np.array([e["box"] for e in log]), np.array([e["box"] for e in wlog])
    assert np.array_equal(boxes, wboxes)                 # the arg-max positions agree and the host arithmetic is the same float64
    ms, wms, rms = (np.array([e["max_score"] for e in lg]) for lg in (log, wlog, rlog))
    f64_bound.held(tag + " max_score", ms, wms, np.abs(rms - wms).max(), floor=f64_bound.ulp_of_max, table=TABLE, star=True)
    assert [e["trained"] for e in log].count(True) == 2
    nb = len(mems) // 2
    for b, (m, w, r) in enumerate(zip(mems, wmems, rmems)):
        f64_bound.held(f"{tag} {'memory' if b < nb else 'final filter'}[{b % nb}]", m, w, np.abs(r - w).max(), floor=f64_bound.ulp_of_max, table=TABLE, star=True)


def test_closed_loop(loop_anchor):
    feats, want, ref = loop_anchor
    assert [e["scale_ind"] for e in ref[0]] == [e["scale_ind"] for e in want[0]]
    check_loop("loop", run_loop(HipOps, feats), want, ref)


def test_closed_loop_as_captured_graphs(loop_anchor):
    feats, want, ref = loop_anchor
    eager = run_loop(HipOps, feats)

    class FrameGraph(GraphOps):
        """sample_transform runs eagerly (its result feeds the insert) and records its arguments; localize captures the frame's whole
        device section -- every block's transform and response, then the localisation -- into one graph and replays it."""
        pending, filters = [], None

        @staticmethod
        def sample_transform(x, P, w, i):
            FrameGraph.pending.append((x, P, w, i))
            return eco.sample_transform(x, P, w, i)

        @staticmethod
        def localize(sfs, weights, grid):
            args, FrameGraph.pending = FrameGraph.pending, []

            def section():
                xf = [eco.sample_transform(*a) for a in args]
                return eco.localize([eco.apply_filter(h, e) for h, e in zip(FrameGraph.filters, xf)], weights, grid)
            return GraphOps._replayed(section)

    with torch.no_grad():
        state = EC.loop_state(dev)
        FrameGraph.filters = state["filter"]
        got = EC.track_frames(FrameGraph, state, feats, xp=dev)
    assert [(e["scale_ind"], e["slot"], e["max_score"]) for e in got[0]] == [(e["scale_ind"], e["slot"], e["max_score"]) for e in eager[0]]
    assert all(np.array_equal(e["box"], f["box"]) for e, f in zip(got[0], eager[0]))
    assert all(np.array_equal(a, b) for a, b in zip(got[1], eager[1]))


# ---- the unmodified tracker through install(eco=True) ----------------------------------------------------------------------------------
@needs_bundle
def test_unmodified_eco_on_device_through_install(monkeypatch):
    """initialize() + 7 x track() (train_skipping 3) of the reference ECO on the device.  Every rebound symbol with a kernel takes its
    gfx950 branch, and at each such call the torch form on the same inputs agrees within the bound (float64 and fp32 runs of the torch
    form on the device).  Not compared with a CPU run: initialize() goes through torch.svd and autograd CG, whose CPU and GPU results
    legitimately differ."""
    import eco_tracker as ET
    ref_harness.install()
    from pytracking_amd import install as amd
    calls = OrderedDict()

    def f64(v):
        if isinstance(v, torch.Tensor):
            return v.double() if v.is_floating_point() else v
        return type(v)(f64(e) for e in v) if isinstance(v, (tuple, list)) else v

    def checked(name, kernel, form):
        def fn(*args, **kw):
            args = args + tuple(kw.values())
            pre = [a.clone() if isinstance(a, torch.Tensor) else a for a in args]
            out = kernel(*args)
            want, ref = form(*f64(pre)), form(*pre)
            units = []
            for q, (o, w, r) in enumerate(zip(*[(v if isinstance(v, (tuple, list)) else (v,)) for v in (out, want, ref)])):
                if o.dtype == torch.int64:
                    continue
                w = w.cpu().numpy()
                err, ref_err = float(np.abs(host(o) - w).max()), float(np.abs(host(r) - w).max())
                units.append(max(ref_err, f64_bound.ulp_of_max(w)))
                calls.setdefault(name, []).append(err / units[-1] if units[-1] > 0 else 0.0)
                assert err <= f64_bound.bound(units[-1]), (name, q, err, units[-1])
            if name == "localize":                       # the arg-max: the float64 score at the kernel's position is the maximum up to the bound
                s64, am = want[0].cpu().numpy(), out[2].cpu().numpy()
                for sc in range(am.shape[0]):
                    assert s64[sc, 0].max() - s64[sc, 0, am[sc, 0, 0], am[sc, 0, 1]] <= 2 * f64_bound.bound(units[0]), (name, sc)
            return out
        return fn

    monkeypatch.setattr(eco, "sample_transform", checked("sample_transform", eco.sample_transform, eco.sample_transform_torch))
    monkeypatch.setattr(eco, "apply_filter", checked("apply_filter", eco.apply_filter, eco.apply_filter_torch))
    monkeypatch.setattr(eco, "localize", checked("localize", eco.localize, eco.localize_torch))
    monkeypatch.setattr(eco, "shift_fs", checked("shift_fs", eco.shift_fs, eco.shift_fs_torch))
    monkeypatch.setattr(eco, "insert", checked("insert", eco.insert, lambda m, x, i: eco.insert_torch(m, x, i)))
    real_update, fu_ratios = eco.filter_update, []

    def checked_update(filters, samples, weights, yf, regs, energy, new_xf, state, num_iter, lrs, reg_energy, fr, std_alpha, forget, dp, rp):
        """Against the float64 restatement (and its fp32 mode) started from the same filter, energy and carried CG state."""
        cx = lambda t: EC.to_c(host(t))      # noqa: E731
        runs = []
        for single in (False, True):
            o = EC.FilterOptimNp(*[[host(t) for t in ts] for ts in (filters, samples, weights, yf, regs, energy)], lrs, reg_energy, fr, std_alpha,
                                 forget, dp, rp, single=single)
            if all(s["state"][1].item() != 0 for s in state):
                o.p, o.r_prev, o.rho = [cx(s["p"]) for s in state], [cx(s["r_prev"]) for s in state], [s["state"][0].item() for s in state]
            o.run(num_iter, None if new_xf is None else [host(t) for t in new_xf])
            runs.append([EC.to_r(x) for x in o.x])
        out = real_update(filters, samples, weights, yf, regs, energy, new_xf, state, num_iter, lrs, reg_energy, fr, std_alpha, forget, dp, rp)
        for f, w, r in zip(filters, *runs):
            err, unit = float(np.abs(host(f) - w).max()), max(float(np.abs(r - w).max()), f64_bound.ulp_of_max(w))
            fu_ratios.append(err / unit)
            assert err <= f64_bound.bound(unit), ("filter_update", err, unit)
        return out
    monkeypatch.setattr(eco, "filter_update", checked_update)
    amd.install(eco=True)
    amd.stats.clear()
    try:
        boxes, scores, tracker = ET.run(device=DEV, n_frames=7, train_skipping=3)
        import pytracking.libs.fourier as fourier
        a = torch.randn(2, 3, 6, 9, device=DEV)
        assert (fourier.cfft2(a) - eco.cfft2(a)).abs().max() <= 1e-5
        stats = dict(amd.stats)
    finally:
        amd.uninstall()
    print("\ninstall(eco=True):", stats, {k: f"{max(v):.2f}x over {len(v)} calls" for k, v in calls.items()})
    print("filter_update:", [f"{v:.2f}" for v in fu_ratios])
    for name in ("cfft2", "shift_fs", "ECO.preprocess_sample", "ECO.extract_fourier_sample", "ECO.apply_filter", "ECO.localize_target",
                 "ECO.update_memory", "FilterOptim.run"):
        assert stats.get(name + ".fast", 0) >= 1, (name, stats)
    assert stats["FilterOptim.run.fast"] >= 2 and len(fu_ratios) >= 4                 # post-init call(s) and the training frames, two blocks
    assert stats.get("ECO.extract_fourier_sample.fast") == 7 and stats.get("ECO.localize_target.fast") == 7 and "ECO.localize_target.reference" not in stats
    assert set(calls) == {"sample_transform", "apply_filter", "localize", "shift_fs", "insert"}
    assert np.isfinite(boxes).all() and np.isfinite(scores).all() and tracker.training_samples[0].is_cuda
    assert not [k for k in stats if k.startswith("GaussNewtonCG") and k.endswith(".fast")]
