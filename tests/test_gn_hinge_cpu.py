"""Hinge-residual GN solver (pytracking_amd.gn_hinge, pt_gn_hinge_solve_f32) without a GPU: the goldens are the reference's
bits and agree with the float64 restatement, the C ABI refuses bad arguments before any launch, and install() routes a reference
LinearFilterHinge / RTSResidual to the fused classes (CPU tensors take the reference forward)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gn_hinge_np import gn_hinge
from oracle import ref_harness
from pytracking_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = ["gn_hinge_relu_none", "gn_hinge_relu_img_leak0", "gn_hinge_bent_img", "gn_hinge_bent_slreg", "gn_hinge_relu_s2",
         "gn_hinge_relu_floatreg", "gn_hinge_fast_small"]
DEPLOYED = ["gn_hinge_dimp_simple_it10", "gn_hinge_dimp_simple_it2", "gn_hinge_rts_clf_it10"]
OTHER = ["gn_rts_small", "gn_rts_cfg5_n32", "tracker_dimp_simple"]      # RTSResidual learner, DiMPSimple closed-loop run
needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_golden_files_are_small():
    for name in SMALL + DEPLOYED + OTHER:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 1 << 20, name


@needs_ref
def test_generator_reproduces_goldens_bit_for_bit(tmp_path):
    env = dict(os.environ, GN_HINGE_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "tools", "make_golden_gn_hinge.py")], check=True, env=env,
                   capture_output=True, timeout=900)
    for name in SMALL + DEPLOYED + OTHER:
        a, b = _load(name), dict(np.load(str(tmp_path / (name + ".npz"))))
        assert sorted(a) == sorted(b), name
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize("name", SMALL)
def test_numpy_restatement_matches_golden(name):
    g = _load(name)
    S = int(g["S"])
    sw = g["sw"] if g["sw"].size else None
    for s in range(S):
        its, losses = gn_hinge(g["w0"][s], g["feat"][:, s], g["label"][:, s], sw, int(g["num_iter"]), str(g["score_act"]),
                               float(g["act_param"]), float(g["hinge_threshold"]), float(g["activation_leak"]),
                               float(g["filter_reg"]), float(g["steplength_reg"]))
        scale = np.abs(g["iterates"][s]).max()
        np.testing.assert_allclose(its, g["iterates"][s], atol=1e-5 * scale, rtol=0)
        if S == 1:
            np.testing.assert_allclose(losses, g["losses"], rtol=1e-5)
    if S > 1:   # the reference's loss over all sequences = the mean of the per-sequence losses (equal sizes)
        per = [gn_hinge(g["w0"][s], g["feat"][:, s], g["label"][:, s], sw, int(g["num_iter"]), str(g["score_act"]),
                        float(g["act_param"]), float(g["hinge_threshold"]), float(g["activation_leak"]), float(g["filter_reg"]),
                        float(g["steplength_reg"]))[1] for s in range(S)]
        np.testing.assert_allclose(np.mean(per, axis=0), g["losses"], rtol=1e-5)


def test_numpy_restatement_matches_deployed_golden():
    from pytracking_amd import synth
    g = _load("gn_hinge_dimp_simple_it2")
    w0, feat, label, sw = synth.gn_hinge_problem(int(g["seed"]), int(g["n"]), int(g["C"]), int(g["H"]), int(g["W"]), int(g["K"]), 1,
                                                 str(g["sw_mode"]))
    its, losses = gn_hinge(w0[0], feat[:, 0], label[:, 0], sw, 2, "relu", 0.0, float(g["hinge_threshold"]),
                           float(g["activation_leak"]), float(g["filter_reg"]), 0.0)
    np.testing.assert_allclose(its[1], g["iterate1"][0], atol=1e-5 * np.abs(its[1]).max(), rtol=0)
    np.testing.assert_allclose(its[-1], g["final"][0], atol=1e-5 * np.abs(its[-1]).max(), rtol=0)
    np.testing.assert_allclose(losses, g["losses"], rtol=1e-5)


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def test_abi_argument_checks_return_before_any_launch(L):
    """Fake (never dereferenced) 256-aligned addresses: every refusal below must happen on the host."""
    vp = ctypes.c_void_p
    P = [vp(0x100000 * (k + 1)) for k in range(6)]
    prm = _lib.GnHingeParams(_lib.PT_ACT_RELU, 0.0, 0.05, 0.1, 0.1, 0.0)
    n, C, H, W, K = 50, 512, 22, 22, 4
    nb = L.pt_gn_hinge_ws_bytes(n, C, H, W, K)
    assert nb > 0 and nb == L.pt_sd_ws_bytes(n, C, H, W, K)
    assert L.pt_gn_hinge_ws_bytes(0, C, H, W, K) == 0

    def call(p=ctypes.byref(prm), w=P[0], feat=P[1], stride=C * H * W, label=P[2], sw=None, dims=(n, C, H, W, K), it=2, wi=P[3],
             ws=P[4], wsb=nb):
        return L.pt_gn_hinge_solve_f32(p, w, feat, stride, label, sw, *dims, it, wi, None, ws, wsb, None)

    assert call(p=None) == _lib.PT_ERR_NULL
    assert call(label=None) == _lib.PT_ERR_NULL
    assert call(w=None) == _lib.PT_ERR_NULL
    assert call(ws=None) == _lib.PT_ERR_NULL
    assert call(dims=(0, C, H, W, K)) == _lib.PT_ERR_SHAPE
    assert call(it=-1) == _lib.PT_ERR_SHAPE
    assert call(stride=C * H * W - 1) == _lib.PT_ERR_SHAPE
    assert call(dims=(n, C, H, W, 5)) == _lib.PT_ERR_UNSUPPORTED
    assert call(it=65) == _lib.PT_ERR_UNSUPPORTED
    bad = _lib.GnHingeParams(7, 0.0, 0.05, 0.1, 0.1, 0.0)
    assert call(p=ctypes.byref(bad)) == _lib.PT_ERR_UNSUPPORTED
    assert call(wsb=nb - 4) == _lib.PT_ERR_WORKSPACE
    assert call(ws=vp(0x100000 + 4)) == _lib.PT_ERR_WORKSPACE
    # routes: the deployed DiMP-simple size is XCD-aligned, the RTS classifier's 15x26 map (H*W % 4 != 0) is not
    assert L.pt_gn_hinge_route(P[1], C * H * W, P[0], P[3], n, C, H, W, K) == 1
    assert L.pt_gn_hinge_route(P[1], C * 15 * 26, P[0], P[3], n, C, 15, 26, K) == 0


@needs_ref
def test_install_routes_hinge_and_rts_residuals():
    ref_harness.install()
    from pytracking import TensorList
    import ltr.models.meta.steepestdescent as smod
    import ltr.models.target_classifier.residual_modules as rm
    from pytracking_amd import install as amd, gn_hinge as GH, steepestdescent as SD
    ref_gn = smod.GNSteepestDescent
    amd.install()
    try:
        res = rm.LinearFilterHinge(init_filter_reg=0.1, hinge_threshold=0.05, activation_leak=0.1, score_act="relu")
        opt = smod.GNSteepestDescent(residual_module=res, num_iter=3, compute_losses=True, residual_batch_dim=1)
        assert isinstance(opt, GH.GNSteepestDescent) and isinstance(opt, torch.nn.Module)
        assert opt.residual_module is res and type(res) is rm.LinearFilterHinge
        assert sorted(opt.state_dict()) == ["residual_module.filter_reg"]
        # residual_batch_dim other than 1: the reference class
        assert not isinstance(smod.GNSteepestDescent(residual_module=res), GH.GNSteepestDescent)
        # CPU tensors take the reference forward and reproduce the golden
        g = _load("gn_hinge_relu_none")
        T = torch.from_numpy
        amd.stats.clear()
        w, its, losses = opt(TensorList([T(g["w0"])]), feat=T(g["feat"][:, 0]), bb=None, train_label=T(g["label"][:, 0])[:, None],
                             sample_weight=None)
        assert amd.stats["GNSteepestDescent.hinge.reference"] == 1 and amd.stats["GNSteepestDescent.hinge.fast"] == 0
        np.testing.assert_array_equal(w[0].detach().numpy(), g["iterates"][:, -1])
        # RTS segmentation learner: an undilated RTSResidual becomes the LWTL mirror -> the LWL fused class
        import ltr.models.rts.loss_residual_modules as rts
        r = rts.RTSResidual(init_filter_reg=0.1)
        assert isinstance(r, SD.LWTLResidual)
        assert isinstance(smod.GNSteepestDescent(residual_module=r, residual_batch_dim=1), SD.GNSteepestDescent)
        assert not isinstance(rts.RTSResidual(init_filter_reg=0.1, filter_dilation_factors=[1, 2]), SD.LWTLResidual)
    finally:
        amd.uninstall()
    assert smod.GNSteepestDescent is ref_gn
    import ltr.models.rts.loss_residual_modules as rts
    assert not isinstance(rts.RTSResidual(), SD.LWTLResidual)
