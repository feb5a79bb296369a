"""KYS response prediction (pytracking_amd.kys, kys.hip) without a GPU: the float64 restatement (tests/kys_np.py) reproduces the goldens
of the unmodified reference (tools/make_golden_kys.py), its brute-force cost volume equals the torch stand-in sampler followed by the
reference's remap_cost_volume, its resampling equals torch's affine_grid / grid_sample, the C ABI refuses bad arguments before any launch,
the header and the loader agree on the entry points, and install(kys=True) makes ltr.models.tracking.kysnet importable."""
import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import kys_np
import kys_standin
from oracle import ref_harness
from pytracking_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CV = ["kys_cv_1x1", "kys_cv_5x7", "kys_cv_6x6", "kys_cv_9x4", "kys_cv_18x18"]
PRED = [f"kys_pred_{s}_{v}" for s in ("5x7", "18x18") for v in "abcd"]
needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_golden_files_are_small():
    for fn in os.listdir(GOLDEN):
        if fn.startswith("kys_"):
            assert os.path.getsize(os.path.join(GOLDEN, fn)) <= 512 << 10, fn


@pytest.mark.parametrize("name", CV)
def test_numpy_cost_volume_matches_golden(name):
    g = _load(name)
    B, C, H, W = (int(v) for v in g["shape"])
    md = int(g["md"])
    cur, prev = synth.kys_features(int(g["seed"]), B, C, H, W)
    small = "out" in g
    disp = kys_np.cost_volume(cur, prev, md, remap=False) if small else kys_np.cost_volume_shifted(cur, prev, md)
    rem = kys_np.remap_cost_volume(disp)
    assert rem.shape == (B, H * W, H, W) and disp.shape == (B, (2 * md + 1) ** 2, H, W)
    tol, tol_d = float(g["ref_fp32_err"]) * 1.0000001, float(g["ref_fp32_err_disp"]) * 1.0000001      # the stored error IS this distance
    if small:
        assert np.abs(rem - g["out"]).max() <= tol and np.abs(disp - g["out_disp"]).max() <= tol_d
        np.testing.assert_allclose(kys_np.cost_volume_shifted(cur, prev, md), disp, atol=1e-12, rtol=0)
        np.testing.assert_allclose(kys_np.cost_volume_gram(cur, prev, md), rem, atol=1e-12, rtol=0)
    else:
        assert np.abs(rem.reshape(-1)[g["sample_idx"]] - g["sample"]).max() <= tol
        assert np.abs(disp.reshape(-1)[g["sample_idx_disp"]] - g["sample_disp"]).max() <= tol_d
        np.testing.assert_allclose(kys_np.cost_volume_gram(cur, prev, md), rem, atol=1e-12, rtol=0)
        # the brute force itself on a few positions of the deployed shape
        r = np.random.default_rng(0)
        P = md + 1
        cp, pp = (np.pad(a.astype(np.float64), ((0, 0), (0, 0), (P, P), (P, P))) for a in (cur, prev))
        for _ in range(50):
            y, x, di, dj = int(r.integers(H)), int(r.integers(W)), int(r.integers(2 * md + 1)), int(r.integers(2 * md + 1))
            y2, x2 = y + di - md, x + dj - md
            v = np.vdot(cp[0, :, y + P - 1:y + P + 2, x + P - 1:x + P + 2], pp[0, :, y2 + P - 1:y2 + P + 2, x2 + P - 1:x2 + P + 2])
            assert abs(disp[0, di * (2 * md + 1) + dj, y, x] - v) < 1e-12


def test_cost_volume_probes():
    """A one-hot pair gives one known block; a constant map shows the border tap counts 4 / 6 / 9."""
    H, W, md = 5, 6, 2
    cur, prev = np.zeros((1, 2, H, W)), np.zeros((1, 2, H, W))
    cur[0, 1, 2, 3], prev[0, 1, 3, 2] = 2.0, 3.0
    rem = kys_np.cost_volume(cur, prev, md).reshape(H, W, H, W)
    # taps (i, j): cur (2, 3) = (r + i, c + j), prev (3, 2) = (r' + i, c' + j)  ->  (r', c') = (r + 1, c - 1), for the 9 (r, c) around (2, 3)
    want = np.zeros_like(rem)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            want[3 - i, 2 - j, 2 - i, 3 - j] = 6.0
    np.testing.assert_array_equal(rem, want)
    ones = np.ones((1, 1, 4, 4))
    rem = kys_np.cost_volume(ones, ones, 1).reshape(4, 4, 4, 4)
    assert rem[0, 0, 0, 0] == 4 and rem[0, 1, 0, 1] == 6 and rem[1, 1, 1, 1] == 9 and rem[3, 3, 3, 3] == 4
    assert rem[0, 0, 1, 1] == 4 and rem[3, 3, 0, 0] == 0            # taps inside BOTH maps; outside the window


@needs_ref
@pytest.mark.parametrize("shape", [(2, 5, 4, 6, 2), (1, 3, 3, 3, 4)])
def test_brute_force_equals_standin_and_reference_remap(shape, monkeypatch):
    ref_harness.install()
    kys_standin.register()
    import ltr.models.kys.cost_volume as cvmod
    from ltr.models.kys.cost_volume import CostVolume, remap_cost_volume
    # an earlier install() in this process may have left the gfx950 class bound in the reference module: this test is about the stand-in
    monkeypatch.setattr(cvmod, "SpatialCorrelationSampler", kys_standin.SpatialCorrelationSampler)
    B, C, H, W, md = shape
    cur, prev = synth.kys_features(7, B, C, H, W)
    layer = kys_standin.SpatialCorrelationSampler(3, 2 * md + 1, 1, 1)
    raw = layer(torch.from_numpy(cur).double(), torch.from_numpy(prev).double())
    disp = kys_np.cost_volume(cur, prev, md, remap=False)
    np.testing.assert_allclose(raw.reshape(B, -1, H, W).numpy(), disp, atol=1e-12, rtol=0)
    np.testing.assert_allclose(remap_cost_volume(raw.reshape(B, -1, H, W)).reshape(B, H * W, H, W).numpy(), kys_np.remap_cost_volume(disp),
                               atol=1e-12, rtol=0)
    ref = CostVolume(3, md, abs_coordinate_output=True)(torch.from_numpy(cur), torch.from_numpy(prev)).numpy()
    np.testing.assert_allclose(ref, kys_np.cost_volume(cur, prev, md), atol=1e-5, rtol=0)


def test_numpy_shift_is_torch_shift_features():
    """utils.py:6-13 at the installed torch's defaults: bilinear, zero padding, a quarter pixel."""
    import torch.nn.functional as F
    from pytracking_amd import kys as K
    assert K.shift_px() == pytest.approx(kys_np.SHIFT_PX, abs=1e-6)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 1, 5, 7)))
    for sign in (-1.0, 1.0):
        t = sign * torch.ones(2, 2, dtype=torch.float64) * 0.5 / torch.tensor([[7.0, 5.0]], dtype=torch.float64)
        theta = torch.cat((torch.eye(2, dtype=torch.float64).repeat(2, 1, 1), t.view(-1, 2, 1)), dim=2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = F.grid_sample(x, F.affine_grid(theta, x.shape))
        np.testing.assert_allclose(kys_np.shift(x.numpy(), sign * kys_np.SHIFT_PX), ref.numpy(), atol=1e-12, rtol=0)


def _pred_case(g):
    B, C, H, W = (int(v) for v in g["shape"])
    cur, prev = synth.kys_features(int(g["feat_seed"]), B, C, H, W)
    inp = synth.kys_frame_inputs(int(g["input_seed"]), B, H, W)
    return cur, prev, inp


@pytest.mark.parametrize("name", PRED)
def test_numpy_predictor_matches_golden(name):
    g = _load(name)
    cur, prev, inp = _pred_case(g)
    conf = str(g["conf_measure"])
    sd = synth.kys_predictor_state(int(g["state_seed"]), conf)
    out = kys_np.predict_response(sd, kys_np.cost_volume_gram(cur, prev, int(g["md"])), inp["dimp_score_cur"],
                                  state_prev=inp["state_prev"] if g["with_state"] else None, label_prev=inp["label_prev"],
                                  dimp_thresh=float(g["dimp_thresh"]) if g["with_thresh"] else None,
                                  window=inp["window"] if g["with_window"] else None, conf_measure=conf)
    assert float(g["thresh_margin"]) > 1e-3
    assert np.abs(out["score_shifted"] - float(g["dimp_thresh"])).min() == pytest.approx(float(g["thresh_margin"]), abs=1e-6)
    np.testing.assert_allclose(out["response"].reshape(g["response"].shape), g["response"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(out["state_cur"], g["state_cur"], atol=1e-5, rtol=0)
    aux = out["auxiliary_outputs"]
    assert sorted(aux) == list(g["aux_keys"])
    assert ("propagation_conf" in aux) == (conf == "max")
    pw = _load("kys_pw_" + name.split("_")[2])["propagation_weights"]
    for k in g["aux_keys"]:
        want = pw if k in ("cost_volume_processed", "propagation_weights") else g["aux_" + k]
        np.testing.assert_allclose(aux[k].reshape(want.shape), want, atol=1e-5, rtol=0, err_msg=k)


def test_numpy_closed_loop_matches_golden():
    g = _load("kys_loop")
    B, C, H, W, md = (int(g[k]) for k in ("B", "C", "H", "W", "md"))
    sd = synth.kys_predictor_state(int(g["state_seed"]), "max")
    for t in (0, int(g["frames"]) - 1):                          # the first frame (label_prev) and the last (golden state of the one before)
        cur, prev = synth.kys_features(int(g["seed"]) + t, B, C, H, W)
        inp = synth.kys_frame_inputs(int(g["seed"]) + 100 + t, B, H, W)
        out = kys_np.predict_response(sd, kys_np.cost_volume_gram(cur, prev, md), inp["dimp_score_cur"],
                                      state_prev=None if t == 0 else g["state_cur"][t - 1], label_prev=inp["label_prev"], window=inp["window"])
        np.testing.assert_allclose(out["response"].reshape(g["response"][t].shape), g["response"][t], atol=1e-5, rtol=0)
        np.testing.assert_allclose(out["state_cur"], g["state_cur"][t], atol=1e-5, rtol=0)


@pytest.fixture(scope="module")
def L():
    if _lib.needs_build():
        _lib.build_library()
    return _lib.lib()


def test_header_symbols_match_exports():
    text = open(os.path.join(ROOT, "include", "pt_hot.h")).read()
    declared = set(re.findall(r"\b(pt_kys_\w+)\s*\(", text))
    assert declared == {n for n in _lib.EXPORTS if n.startswith("pt_kys_")} and len(declared) == 5
    assert f"#define PT_KYS_CV_MAX_HW {_lib.PT_KYS_CV_MAX_HW}\n" in text and f"#define PT_KYS_PRED_MAX_HW {_lib.PT_KYS_PRED_MAX_HW}\n" in text


def test_abi_argument_checks_do_not_launch(L):
    n, one = None, ctypes.c_void_p(256)
    for name in (x for x in _lib.EXPORTS if x.startswith("pt_kys_")):
        assert hasattr(L, name)
    big = 1 << 40

    def cv(cur=one, prev=one, B=1, C=8, H=4, W=4, k=3, md=2, s=1, out=one, ws=one, nbytes=big):
        return L.pt_kys_cost_volume_f32(cur, prev, B, C, H, W, k, md, s, 1, out, ws, nbytes, n)

    assert cv(cur=n) == cv(prev=n) == cv(out=n) == cv(ws=n) == _lib.PT_ERR_NULL
    assert cv(C=0) == cv(H=0) == cv(W=-1) == cv(B=0) == cv(md=0) == _lib.PT_ERR_SHAPE
    assert cv(k=1) == cv(k=5) == cv(s=2) == cv(H=33, W=32) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_kys_cost_volume_ws_bytes(1, 1024, 18, 18) == 8 * 324 * 324 * 4
    assert cv(nbytes=L.pt_kys_cost_volume_ws_bytes(1, 8, 4, 4) - 4) == _lib.PT_ERR_WORKSPACE
    nf = L.pt_kys_weight_floats(8, 64, 32, 3, 1)
    assert nf == 27900 and L.pt_kys_weight_floats(8, 64, 32, 3, 0) == nf - 64 * 9
    assert L.pt_kys_weight_floats(16, 64, 32, 3, 1) == L.pt_kys_weight_floats(8, 32, 32, 3, 1) == L.pt_kys_weight_floats(8, 64, 32, 5, 1) == 0

    def prm(B=1, H=18, W=18, sd=8, r0=64, r1=32, gk=3, conf=1, floats=nf, wstride=0):
        return _lib.KysPredictParams(B, H, W, sd, r0, r1, gk, conf, 0, 0.0, 0.25, wstride, floats)

    def call(p, ptrs=None, nbytes=big):
        ptrs = ptrs or [one] * 16
        return L.pt_kys_predict_response_f32(ctypes.byref(p), *ptrs, nbytes, n)

    assert call(prm(), [n] + [one] * 15) == _lib.PT_ERR_NULL
    assert call(prm(), [one, one, n, n] + [one] * 12) == _lib.PT_ERR_NULL                     # neither state_prev nor label_prev
    assert call(prm(), [one] * 10 + [n] + [one] * 5) == _lib.PT_ERR_NULL                      # conf_measure 'max' without its output
    assert call(prm(H=0)) == call(prm(B=0)) == _lib.PT_ERR_SHAPE
    assert call(prm(H=21, W=20)) == call(prm(sd=16)) == call(prm(r0=32)) == call(prm(gk=5)) == _lib.PT_ERR_UNSUPPORTED
    assert call(prm(floats=nf - 1)) == call(prm(wstride=7)) == _lib.PT_ERR_SHAPE
    assert call(prm(), nbytes=L.pt_kys_predict_ws_bytes(1, 18, 18) - 4) == _lib.PT_ERR_WORKSPACE


def test_product_path_refuses_cpu_tensors():
    from pytracking_amd import kys as K
    x = torch.zeros(1, 4, 3, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        K.cost_volume(x, x, 1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        K.predict_response(None, {"feat1": x, "feat2": x, "dimp_score_cur": x[:, :1], "state_prev": None})
    assert "oracle" not in open(K.__file__).read().replace("oracle/", "")


_IMPORT_PROBE = """
import sys
sys.path.insert(0, {root!r})
from oracle import ref_harness
ref_harness.install()
try:
    import ltr.models.tracking.kysnet
    raise SystemExit("kysnet imported without the sampler")
except ImportError:
    pass
for m in [m for m in sys.modules if m.startswith("ltr.models.kys") or m == "ltr.models.tracking.kysnet"]:
    del sys.modules[m]
from pytracking_amd import install as amd, kys as K
amd.install(kys=True)
import ltr.models.tracking.kysnet as kn
from ltr.models.kys.predictor_wrapper import PredictorWrapper
from ltr.models.kys.cost_volume import CostVolume
assert sys.modules["spatial_correlation_sampler"] is K
assert isinstance(CostVolume(3, 9).correlation_layer, K.SpatialCorrelationSampler)
ref_pr, ref_fw = PredictorWrapper.predict_response.__wrapped__, CostVolume.forward.__wrapped__
amd.uninstall()
assert "spatial_correlation_sampler" not in sys.modules
assert PredictorWrapper.predict_response is ref_pr and CostVolume.forward is ref_fw
# somebody else's module under that name is left alone, by install() and by uninstall()
import types
mine = types.ModuleType("spatial_correlation_sampler")
sys.modules["spatial_correlation_sampler"] = mine
amd.install(kys=True)
amd.uninstall()
assert sys.modules["spatial_correlation_sampler"] is mine
# kys=False leaves the name alone
del sys.modules["spatial_correlation_sampler"]
amd.install(kys=False)
assert "spatial_correlation_sampler" not in sys.modules and PredictorWrapper.predict_response is ref_pr
amd.uninstall()
print("KYS-IMPORT-OK")
"""


@pytest.mark.skipif(not os.path.exists(os.path.join(ref_harness.REFERENCE_ROOT, "ltr", "models", "tracking", "kysnet.py")),
                    reason="full reference tree not mounted (the recipe-built bundle carries ltr/models/kys only)")
def test_install_makes_kysnet_importable_and_uninstall_undoes_it():
    """In a fresh interpreter: the import state of this process may already hold a stand-in."""
    res = subprocess.run([sys.executable, "-B", "-c", _IMPORT_PROBE.format(root=ROOT)], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0 and "KYS-IMPORT-OK" in res.stdout, res.stdout + res.stderr
