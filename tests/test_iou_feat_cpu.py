"""IoU feature extraction (pytracking_amd.iou_feat, iou_feat.hip) without a GPU: the float64 restatement (tests/iou_feat_np.py)
reproduces the goldens of the unmodified reference (tools/make_golden_iou_feat.py), the C ABI refuses bad arguments before any launch, the
pack layout is the documented one, install(iou_feat=True) rebinds exactly one more name than the pinned default set, and calls outside
the hot path take the reference branch."""
import ctypes
import json

import numpy as np
import pytest
import torch

import iou_feat_cases as IC
import iou_feat_np
from oracle import ref_harness
from pytracking_amd import _lib, iou_feat as IF, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
NAME = "ltr.models.bbreg.atom_iou_net.AtomIoUNet.get_iou_feat"


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _dims(name):
    n, t3, t4 = synth.IOU_FEAT_CASES[name]
    return [n, *t3, *t4]


@pytest.mark.parametrize("name", IC.CASES)
def test_float64_restatement_reproduces_golden(name):
    """The golden holds the reference's fp32 output; its distance from the float64 restatement is the recorded ref_fp32_err (+ 1e-12 for the
    summation order of the restatement's own float64 products), and the golden tool held that to <= 2.5e-5, a quarter of the GPU bound."""
    g, n, t3, t4, sd, (f3, f4) = IC.case(name)
    r3, r4 = iou_feat_np.get_iou_feat(sd, f3, f4)
    assert r3.shape == (n, t3[2], t3[3], t3[4]) and r4.shape == (n, t4[2], t4[3], t4[4])
    err = IC.against_golden(g, r3, r4)
    print(f"\niou_feat_{name}: max |float64 - golden| = {err:.3e}, recorded ref_fp32_err = {float(g['ref_fp32_err']):.3e}")
    assert err <= float(g["ref_fp32_err"]) + 1e-12
    assert float(g["ref_fp32_err"]) <= 2.5e-5
    assert ("idx3" in g) == (name in IC.DEPLOYED) and (name not in IC.DEPLOYED or g["c3"].shape == (2000,))


def test_argument_checks_do_not_launch(L):
    n = None
    one = ctypes.c_void_p(256)
    d = _dims("dimp50")
    big = 1 << 30
    for name in IC.CASES[:4] + IC.DEPLOYED:                          # the seven cases of the issue
        assert L.pt_iou_feat_ws_bytes(*_dims(name)) > 0, name
    assert L.pt_iou_feat_ws_bytes(*_dims("wide")) > 0                  # GEMM route
    bad = list(d); bad[1] = 100
    assert L.pt_iou_feat_ws_bytes(*bad) == 0
    for k in range(5):                                                 # every pointer, and the workspace
        ptrs = [one] * 5
        ptrs[k] = n
        assert L.pt_iou_feat_f32(*ptrs, *d, one, big, n) == _lib.PT_ERR_NULL
    assert L.pt_iou_feat_f32(one, one, one, one, one, *d, n, big, n) == _lib.PT_ERR_NULL
    for k in range(11):                                                # every size at zero, and a negative one
        z = list(d); z[k] = 0
        assert L.pt_iou_feat_f32(one, one, one, one, one, *z, one, big, n) == _lib.PT_ERR_SHAPE
        assert L.pt_iou_feat_ws_bytes(*z) == 0
    z = list(d); z[4] = -3
    assert L.pt_iou_feat_f32(one, one, one, one, one, *z, one, big, n) == _lib.PT_ERR_SHAPE
    assert L.pt_iou_feat_f32(one, one, one, one, one, *bad, one, big, n) == _lib.PT_ERR_UNSUPPORTED         # Cin = 100
    for k, v in ((0, 9), (2, 24), (3, 8), (4, 65), (7, 40), (8, 250)):   # n > 8, Cmid % 16, Cout % 16, H * W > 4096, Cmid4, Cout4
        u = list(d); u[k] = v
        if k == 4:
            u[5] = 64
        assert L.pt_iou_feat_f32(one, one, one, one, one, *u, one, big, n) == _lib.PT_ERR_UNSUPPORTED, (k, v)
        assert L.pt_iou_feat_ws_bytes(*u) == 0
    assert L.pt_iou_feat_f32(ctypes.c_void_p(260), one, one, one, one, *d, one, big, n) == _lib.PT_ERR_UNSUPPORTED   # misaligned operand
    need = L.pt_iou_feat_ws_bytes(*d)
    assert L.pt_iou_feat_f32(one, one, one, one, one, *d, one, need - 1, n) == _lib.PT_ERR_WORKSPACE        # one byte short
    assert L.pt_iou_feat_f32(one, one, one, one, one, *d, ctypes.c_void_p(384), need, n) == _lib.PT_ERR_WORKSPACE   # misaligned


def _layout_floats(t3, t4):
    return sum(o * 9 * i + 2 * o for i, o in ((t3[0], t3[1]), (t3[1], t3[2]), (t4[0], t4[1]), (t4[1], t4[2])))


def test_pack_layout(L):
    for name in IC.CASES:
        n, t3, t4 = synth.IOU_FEAT_CASES[name]
        assert L.pt_iou_feat_pack_floats(*t3[:3], *t4[:3]) == _layout_floats(t3, t4), name
    assert L.pt_iou_feat_pack_floats(100, 16, 16, 64, 16, 16) == 0
    assert L.pt_iou_feat_pack_floats(64, 16, 16, 64, 16, 0) == 0
    # the host packer on a CPU module: documented order and values (include/pt_hot.h)
    g, n, t3, t4, sd, _ = IC.case("b")
    net = IC.module("b")
    pack = IF.pack_weights(net).numpy()
    assert pack.dtype == np.float32 and pack.size == _layout_floats(t3, t4)
    at = 0
    for blk in IF.BLOCKS:
        w = sd[blk + ".0.weight"]
        o = w.shape[0]
        np.testing.assert_array_equal(pack[at:at + w.size], w.transpose(0, 2, 3, 1).reshape(-1))
        at += w.size
        scale = sd[blk + ".1.weight"].astype(np.float64) / np.sqrt(sd[blk + ".1.running_var"].astype(np.float64) + 1e-5)
        shift = (sd[blk + ".0.bias"].astype(np.float64) - sd[blk + ".1.running_mean"]) * scale + sd[blk + ".1.bias"]
        np.testing.assert_array_equal(pack[at:at + o], scale.astype(np.float32))
        np.testing.assert_array_equal(pack[at + o:at + 2 * o], shift.astype(np.float32))
        at += 2 * o
    assert at == pack.size


def test_pack_cache_follows_the_module_state():
    net = IC.module("a")
    p0 = IF.packed_weights(net)
    assert IF.packed_weights(net) is p0                                 # unchanged state: the cached pack
    with torch.no_grad():
        net.conv4_2t[1].running_var.mul_(2.0)                           # in-place: the version counter moves
    p1 = IF.packed_weights(net)
    assert p1 is not p0 and not torch.equal(p0, p1)
    net.load_state_dict(IC.state_tensors(IC.case("a")[4]))
    assert torch.equal(IF.packed_weights(net), p0)
    net.conv3_1t[0].bias.data = net.conv3_1t[0].bias.data + 1.0         # through .data: a new tensor, the data_ptr moves
    assert not torch.equal(IF.packed_weights(net), p0)
    IF.refresh(net)
    assert net not in IF._PACKS


def test_covered_refuses_what_the_kernels_do_not_serve():
    net = IC.module("b")
    _, n, t3, t4, _, (f3, f4) = IC.case("b")
    feats = [torch.from_numpy(f3), torch.from_numpy(f4)]
    with torch.no_grad():
        assert not IF.covered(net, feats)                               # CPU tensors
        with pytest.raises(RuntimeError, match="MI355X"):
            IF.get_iou_feat(net, feats)
    assert IF._blocks(net) is not None
    net.train()
    assert not IF.covered(net, feats)                                   # training mode
    net.eval()
    dil = IC.Towers(t3, t4)
    dil.conv3_2t = IC.conv(t3[1], t3[2], dilation=2)
    assert IF._blocks(dil.eval()) is None and not IF.covered(dil, feats)   # a Conv2d with dilation 2
    nobn = IC.Towers(t3, t4).eval()
    nobn.conv4_1t[1] = torch.nn.BatchNorm2d(t4[1], track_running_stats=False)
    assert IF._blocks(nobn) is None                                     # a BatchNorm without running statistics
    assert not IF.covered(net, feats[:1]) and not IF.covered(net, [f.double() for f in feats])


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip, as tests/test_install_ledger.py does; uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(iou_feat=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_reference
def test_install_switch_rebinds_one_more_name(amd):
    import test_install_ledger as TL
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    ref = AtomIoUNet.__dict__["get_iou_feat"]
    before = TL.snapshot()
    amd.install()                                                       # default: off
    assert AtomIoUNet.__dict__["get_iou_feat"] is ref
    with open(TL.REBOUND) as fh:
        pinned = json.load(fh)
    assert TL.changed(before, TL.snapshot()) == pinned
    amd.uninstall()
    amd.install(iou_feat=True)
    assert TL.changed(before, TL.snapshot()) == sorted(pinned + [NAME])
    assert AtomIoUNet.get_iou_feat.__wrapped__ is ref and amd.original(AtomIoUNet, "get_iou_feat") is ref
    amd.uninstall()
    assert AtomIoUNet.__dict__["get_iou_feat"] is ref and TL.changed(before, TL.snapshot()) == []


@needs_reference
def test_cpu_tensors_take_the_reference_branch(amd):
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    g, n, t3, t4, sd, (f3, f4) = IC.case("atom18")
    f3, f4 = f3[:, :, :6, :5], f4[:, :, :3, :4]
    amd.install(iou_feat=True)
    net = AtomIoUNet(input_dim=(t3[0], t4[0]), pred_input_dim=(t3[2], t4[2]))
    net.load_state_dict(IC.state_tensors(sd), strict=False)
    net.eval()
    amd.stats.clear()
    with torch.no_grad():
        c3, c4 = net.get_iou_feat([torch.from_numpy(f3), torch.from_numpy(f4)])
    assert amd.stats["AtomIoUNet.get_iou_feat.reference"] == 1 and amd.stats["AtomIoUNet.get_iou_feat.fast"] == 0
    r3, r4 = iou_feat_np.get_iou_feat(sd, f3, f4)
    assert np.abs(c3.numpy() - r3).max() < 1e-4 and np.abs(c4.numpy() - r4).max() < 1e-4
    amd.uninstall()
    amd.install(strict=True, iou_feat=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="get_iou_feat"):
        net.get_iou_feat([torch.from_numpy(f3), torch.from_numpy(f4)])
