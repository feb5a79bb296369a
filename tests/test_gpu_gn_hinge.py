"""Hinge-residual GN solver on the MI355X (pt_gn_hinge_solve_f32 through pytracking_amd.gn_hinge) against the reference's goldens
(tools/make_golden_gn_hinge.py): iterates, losses and final scores within 1e-4; the deployed DiMP-simple size takes the fast route;
a captured graph replays bit-equal to the eager call; install() routes a reference LinearFilterHinge to the fused solver."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from pytracking_amd import _lib, gn_hinge as GH, synth
from pytracking_amd.filter import apply_filter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
SMALL = ["gn_hinge_relu_none", "gn_hinge_relu_img_leak0", "gn_hinge_bent_img", "gn_hinge_bent_slreg", "gn_hinge_relu_s2",
         "gn_hinge_relu_floatreg", "gn_hinge_fast_small"]
DEPLOYED = ["gn_hinge_dimp_simple_it10", "gn_hinge_dimp_simple_it2", "gn_hinge_rts_clf_it10"]


# stand-ins with the reference's class names and the attributes the fused class reads (residual_modules.py:88-106,
# activation.py:30-55); the reference objects themselves are covered by test_install_routes_reference_hinge below
class LeakyReluPar(nn.Module):
    pass


class BentIdentPar(nn.Module):
    def __init__(self, b):
        super().__init__()
        self.b = b


class LinearFilterHinge(nn.Module):
    def __init__(self, filter_reg, thr, leak, score_act, b, float_reg):
        super().__init__()
        self.filter_reg = filter_reg if float_reg else nn.Parameter(filter_reg * torch.ones(1))
        self.hinge_threshold, self.activation_leak = thr, leak
        self.score_activation = LeakyReluPar() if score_act == "relu" else BentIdentPar(b)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _problem(g):
    if "feat" in g:
        return g["w0"], g["feat"], g["label"], (g["sw"] if g["sw"].size else None)
    return synth.gn_hinge_problem(int(g["seed"]), int(g["n"]), int(g["C"]), int(g["H"]), int(g["W"]), int(g["K"]), int(g["S"]),
                                  str(g["sw_mode"]))


def _solver(g):
    res = LinearFilterHinge(float(g["filter_reg"]), float(g["hinge_threshold"]), float(g["activation_leak"]), str(g["score_act"]),
                            float(g["act_param"]), bool(g["float_reg"])).to(DEV)
    return GH.GNSteepestDescent(res, num_iter=int(g["num_iter"]), compute_losses=True, steplength_reg=float(g["steplength_reg"]),
                                residual_batch_dim=1)


def _run(g, opt=None):
    w0, feat, label, sw = _problem(g)
    S = int(g["S"])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f = d(feat) if S > 1 else d(feat[:, 0])
    lab = d(label) if S > 1 else d(label[:, 0])[:, None]
    opt = opt or _solver(g)
    with torch.no_grad():
        w, its, losses = opt([d(w0)], feat=f, bb=None, train_label=lab, sample_weight=None if sw is None else d(sw).view(-1, 1, 1, 1))
    return w, its, losses, d(feat)


@pytest.mark.parametrize("name", SMALL + DEPLOYED)
def test_fused_matches_reference_golden(name):
    g = _load(name)
    w, its, losses, feat5 = _run(g)
    torch.cuda.synchronize()
    assert len(its) == int(g["num_iter"]) + 1 and len(losses) == int(g["num_iter"]) + 1
    stack = torch.stack([i[0] for i in its], dim=1).cpu().numpy()             # (S, T+1, C, K, K)
    if "iterates" in g:
        np.testing.assert_allclose(stack, g["iterates"], atol=1e-4, rtol=0)
    else:
        np.testing.assert_allclose(stack[:, 1], g["iterate1"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(stack[:, -1], g["final"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(torch.stack(losses).cpu().numpy(), g["losses"], atol=1e-9, rtol=1e-4)
    with torch.no_grad():
        scores = apply_filter(feat5 if "scores" in g else feat5[:4], w[0]).cpu().numpy()
    np.testing.assert_allclose(scores, g["scores"] if "scores" in g else g["scores_first4"], atol=1e-4, rtol=0)


@pytest.mark.parametrize("name,want", [("gn_hinge_dimp_simple_it10", "fast"), ("gn_hinge_fast_small", "fast"),
                                       ("gn_hinge_rts_clf_it10", "generic")])
def test_route_taken_by_the_solve(name, want):
    """The route the solve took, read with the operands it was handed (the deployed DiMP-simple size must be on the fast one)."""
    g = _load(name)
    opt = _solver(g)
    _run(g, opt)
    assert opt.last_routes == [want], opt.last_routes


def test_map_larger_than_one_block_takes_the_generic_route():
    """33x33 score maps (1089 elements) pass the fast route's shape plan but not its one-element-per-thread init stage: the solve runs
    on the generic route and agrees with the float64 restatement."""
    from gn_hinge_np import gn_hinge
    w0, feat, label, sw = synth.gn_hinge_problem(720, 6, 128, 32, 32, 4, 1, "per_image")
    g = dict(filter_reg=0.1, hinge_threshold=0.05, activation_leak=0.1, score_act="relu", act_param=0.0, float_reg=False,
             num_iter=3, steplength_reg=0.0, S=1, w0=w0, feat=feat, label=label, sw=sw)
    opt = _solver(g)
    w, its, losses, _ = _run(g, opt)
    assert opt.last_routes == ["generic"]
    ref_its, ref_losses = gn_hinge(w0[0], feat[:, 0], label[:, 0], sw, 3, "relu", 0.0, 0.05, 0.1, 0.1, 0.0)
    np.testing.assert_allclose(torch.stack([i[0][0] for i in its]).cpu().numpy(), ref_its, atol=1e-4, rtol=0)
    np.testing.assert_allclose(torch.stack(losses).cpu().numpy(), ref_losses, atol=1e-9, rtol=1e-4)


@torch.no_grad()
def test_covered_screens_label_and_sample_weight():
    g = _load("gn_hinge_relu_none")
    res = _solver(g).residual_module
    w = torch.zeros(1, 16, 4, 4, device=DEV)
    feat = torch.zeros(5, 16, 7, 8, device=DEV)
    lab = torch.zeros(5, 1, 8, 9, device=DEV)
    kw = lambda **k: dict(dict(feat=feat, train_label=lab, sample_weight=None, _num_iter=2), **k)
    assert GH.covered(res, [w], kw())
    assert GH.covered(res, [w], kw(sample_weight=torch.ones(5, 1, 1, 1, device=DEV)))
    assert not GH.covered(res, [w], kw(train_label=lab.double()))
    assert not GH.covered(res, [w], kw(sample_weight=torch.ones(5, device=DEV)))          # 1-D: broadcast over the last axis
    assert not GH.covered(res, [w], kw(sample_weight=torch.ones(5, 1, 1, 1, device=DEV, dtype=torch.float64)))
    assert not GH.covered(res, [w], kw(sample_weight=torch.ones(5, 1, 1, 1)))            # host tensor
    assert not GH.covered(res, [w], kw(sample_weight=torch.ones(5, 1, 8, 9, device=DEV)))  # per element


def test_graph_capture_replay_is_bit_equal_to_eager():
    g = _load("gn_hinge_dimp_simple_it2")
    w0, feat, label, sw = _problem(g)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f, lab, sww, w0d = d(feat[:, 0]), d(label[:, 0])[:, None], d(sw).view(-1, 1, 1, 1), d(w0)
    opt = _solver(g)
    with torch.no_grad():
        w_e, _, l_e = opt([w0d], feat=f, train_label=lab, sample_weight=sww)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            opt([w0d], feat=f, train_label=lab, sample_weight=sww)        # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            w_g, _, l_g = opt([w0d], feat=f, train_label=lab, sample_weight=sww)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(w_g[0], w_e[0])
    assert torch.equal(torch.stack(l_g), torch.stack(l_e))


def test_install_routes_reference_hinge():
    from oracle import ref_harness
    if not ref_harness.available():
        pytest.skip("no reference tree / bundle (oracle/_ref)")
    ref_harness.install()
    from pytracking import TensorList
    import ltr.models.meta.steepestdescent as smod
    import ltr.models.target_classifier.residual_modules as rm
    from pytracking_amd import install as amd
    amd.install()
    try:
        g = _load("gn_hinge_dimp_simple_it10")
        res = rm.LinearFilterHinge(init_filter_reg=float(g["filter_reg"]), hinge_threshold=float(g["hinge_threshold"]),
                                   activation_leak=float(g["activation_leak"]), score_act="relu").to(DEV)
        opt = smod.GNSteepestDescent(residual_module=res, num_iter=int(g["num_iter"]), compute_losses=True, residual_batch_dim=1)
        assert isinstance(opt, GH.GNSteepestDescent)
        amd.stats.clear()
        w0, feat, label, sw = _problem(g)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        with torch.no_grad():
            w, its, losses = opt(TensorList([d(w0)]), feat=d(feat[:, 0]), bb=None, train_label=d(label[:, 0])[:, None])
        assert amd.stats["GNSteepestDescent.hinge.fast"] == 1 and amd.stats["GNSteepestDescent.hinge.reference"] == 0
        assert isinstance(w, TensorList) and isinstance(its[-1], TensorList)
        np.testing.assert_allclose(w[0].cpu().numpy(), g["final"], atol=1e-4, rtol=0)
    finally:
        amd.uninstall()


@pytest.mark.parametrize("name", ["gn_rts_small", "gn_rts_cfg5_n32"])
def test_install_routes_rts_residual_to_the_lwl_solver(name):
    """RTS segmentation learner (rts_net.py:309-315) built by the reference's constructors after install(), called as
    rts/linear_filter.py:85 calls it (label and sample weight per element): the LWL fused solver, within 1e-4 of the reference."""
    from oracle import ref_harness
    if not ref_harness.available():
        pytest.skip("no reference tree / bundle (oracle/_ref)")
    ref_harness.install()
    from pytracking import TensorList
    import ltr.models.meta.steepestdescent as smod
    import ltr.models.rts.loss_residual_modules as rts
    from pytracking_amd import install as amd, steepestdescent as SD
    g = _load(name)
    amd.install()
    try:
        res = rts.RTSResidual(init_filter_reg=float(g["filter_reg"])).to(DEV)
        opt = smod.GNSteepestDescent(residual_module=res, num_iter=int(g["num_iter"]), compute_losses=True, residual_batch_dim=1)
        assert isinstance(res, SD.LWTLResidual) and isinstance(opt, SD.GNSteepestDescent)
        if "feat" in g:
            w0, feat, label, sw = g["w0"], g["feat"], g["label"], g["sw"]
        else:
            cfg = {k: int(g[k]) for k in ("n", "F", "C", "H", "W", "K")}
            w0, feat, label, sw = synth.lwl_problem(int(g["seed"]), dict(cfg, filter_reg=float(g["filter_reg"])))
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        amd.stats.clear()
        with torch.no_grad():
            w, its, losses = opt(TensorList([d(w0)[None]]), feat=d(feat)[:, None], label=d(label)[:, None], sample_weight=d(sw)[:, None])
        torch.cuda.synchronize()
        assert amd.stats["GNSteepestDescent.fast"] == 1 and amd.stats["GNSteepestDescent.reference"] == 0
        stack = torch.stack([i[0][0] for i in its]).cpu().numpy()
        if "iterates" in g:
            np.testing.assert_allclose(stack, g["iterates"], atol=1e-4, rtol=0)
        else:
            np.testing.assert_allclose(stack[1], g["iterate1"], atol=1e-4, rtol=0)
            np.testing.assert_allclose(stack[-1], g["final"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(torch.stack([l.reshape(()) for l in losses]).cpu().numpy(), g["losses"], atol=1e-9, rtol=1e-4)
        with torch.no_grad():
            scores = apply_filter(d(feat if "scores" in g else feat[:2])[:, None], w[0])[:, 0].cpu().numpy()
        np.testing.assert_allclose(scores, g["scores"] if "scores" in g else g["scores_first2"], atol=1e-4, rtol=0)
    finally:
        amd.uninstall()
