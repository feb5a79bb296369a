"""Mask label encoder (pytracking_amd.label_encoder, label_enc.hip) without a GPU: the restatement of the folded-pack arithmetic
(tests/label_enc_cases.py: pack -> conv -> scale / shift -> pool ...) reproduces the goldens of the unmodified reference
(tools/make_golden_label_enc.py), which pins the pack layout and the BatchNorm fold; the C ABI refuses bad arguments before any launch;
install(label_encoder=True) rebinds both ResidualDS16SW classes and nothing else beyond the pinned default set; calls outside the hot
path take the reference branch."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import label_enc_cases as LC
from oracle import ref_harness
from pytracking_amd import _lib, label_encoder as LE, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
NAMES = ["ltr.models.lwl.label_encoder.ResidualDS16SW.forward", "ltr.models.rts.label_encoder.ResidualDS16SW.forward"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _layout_floats(dims):
    c0, c1, c2, f = dims
    return sum(o * 9 * i + 2 * o for i, o in ((1, c0), (c0, 2 * c1), (c1, c1), (c1, 2 * c2), (c2, c2), (c2, 2 * f)))


@pytest.mark.parametrize("name", LC.CASES)
def test_pack_arithmetic_reproduces_golden(name, L):
    """float64 arithmetic on the fp32 pack against the reference's fp32 output: the distance is the reference's own rounding
    (ref_fp32_err, float64 module vs fp32 module) plus the rounding of the folded scale / shift to fp32 -- at most one part in 2^24 of
    values of magnitude max_abs per folded layer, of which a path crosses six."""
    g, n, H, W, dims, use_bn, sd, masks = LC.case(name)
    assert all(np.array_equal(v, sd[k]) for k, v in synth.label_enc_state(int(g["state_seed"]), dims, use_bn).items())
    net = LC.module(name)
    pack = LE.pack_weights(net).numpy()
    assert pack.dtype == np.float32 and pack.size == _layout_floats(dims)
    enc, sw = LC.from_pack(pack, dims, masks)
    h, w = LC.out_hw(H, W)
    assert enc.shape == (n, dims[3], h, w) and sw.shape == enc.shape and g["label_enc"].shape == enc.shape
    err = LC.against_golden(g, enc, sw)
    bound = float(g["ref_fp32_err"]) + 6 * float(g["max_abs"]) * 2.0 ** -24 + 1e-12
    print(f"\nlabel_enc_{name}: max |pack arithmetic (float64) - golden| = {err:.3e}, bound {bound:.3e}, ref_fp32_err {float(g['ref_fp32_err']):.3e}")
    assert err <= bound
    assert float(g["ref_fp32_err"]) <= 1e-5
    assert np.abs(sd["samp_w_pred.weight"]).min() > 0 and (g["label_enc"] == 0).any() and (g["sample_w"] < 0).any()


def test_pack_layout_and_fold():
    for name in ("odd", "bn_odd", "dims"):
        g, n, H, W, dims, use_bn, sd, _ = LC.case(name)
        c0, c1, c2, f = dims
        pack = LE.pack_weights(LC.module(name)).numpy()
        at = 0

        def fold(conv, bn, o):
            bias = sd[conv + ".bias"].astype(np.float64) if conv + ".bias" in sd else np.zeros(o)
            if not (use_bn and bn):
                return np.ones(o), bias
            s = sd[bn + ".weight"].astype(np.float64) / np.sqrt(sd[bn + ".running_var"].astype(np.float64) + 1e-5)
            return s, (bias - sd[bn + ".running_mean"]) * s + sd[bn + ".bias"]

        layers = ([("conv_block.0", "conv_block.1")], [("res1.conv1", "res1.bn1"), ("res1.downsample", None)], [("res1.conv2", "res1.bn2")],
                  [("res2.conv1", "res2.bn1"), ("res2.downsample", None)], [("res2.conv2", "res2.bn2")],
                  [("label_pred.0", "label_pred.1"), ("samp_w_pred", None)])
        for group in layers:
            ws = [sd[c + ".weight"] for c, _ in group]
            wcat = np.concatenate([w.transpose(0, 2, 3, 1).reshape(-1) for w in ws])
            np.testing.assert_array_equal(pack[at:at + wcat.size], wcat)
            at += wcat.size
            folded = [fold(c, b, w.shape[0]) for (c, b), w in zip(group, ws)]
            scale, shift = np.concatenate([s for s, _ in folded]), np.concatenate([b for _, b in folded])
            np.testing.assert_array_equal(pack[at:at + scale.size], scale.astype(np.float32))
            np.testing.assert_array_equal(pack[at + scale.size:at + 2 * scale.size], shift.astype(np.float32))
            at += 2 * scale.size
        assert at == pack.size


def test_sizes_and_argument_checks_do_not_launch(L):
    none, one, big = None, ctypes.c_void_p(256), 1 << 40
    for name in LC.CASES:
        n, H, W, dims, _ = synth.LABEL_ENC_CASES[name]
        assert L.pt_label_enc_pack_floats(*dims) == _layout_floats(dims), name
        assert L.pt_label_enc_ws_bytes(n, H, W, *dims) > 0, name
    assert L.pt_label_enc_ws_bytes(32, 480, 832, 16, 32, 64, 16) > 0 and L.pt_label_enc_ws_bytes(1, 1, 1, 64, 64, 64, 64) > 0
    for k in range(4):                                                  # unsupported channel counts, one position at a time
        for v in (8, 24, 80, 128):
            dims = [16, 32, 64, 16]
            dims[k] = v
            assert L.pt_label_enc_pack_floats(*dims) == 0 and L.pt_label_enc_ws_bytes(2, 40, 72, *dims) == 0, dims
            assert L.pt_label_enc_f32(one, one, one, one, 2, 40, 72, *dims, one, big, none) == _lib.PT_ERR_UNSUPPORTED
        dims = [16, 32, 64, 16]
        dims[k] = 0
        assert L.pt_label_enc_pack_floats(*dims) == 0 and L.pt_label_enc_ws_bytes(2, 40, 72, *dims) == 0
        assert L.pt_label_enc_f32(one, one, one, one, 2, 40, 72, *dims, one, big, none) == _lib.PT_ERR_SHAPE
    d = (2, 40, 72, 16, 32, 64, 16)
    for k in range(3):                                                  # n, H, W at zero and negative
        for v in (0, -3):
            z = list(d)
            z[k] = v
            assert L.pt_label_enc_ws_bytes(*z) == 0 and L.pt_label_enc_f32(one, one, one, one, *z, one, big, none) == _lib.PT_ERR_SHAPE
    assert L.pt_label_enc_ws_bytes(2, 9000, 72, 16, 32, 64, 16) == 0 and L.pt_label_enc_ws_bytes(70000, 40, 72, 16, 32, 64, 16) == 0
    for k in range(4):                                                  # every pointer, and the workspace
        ptrs = [one] * 4
        ptrs[k] = none
        assert L.pt_label_enc_f32(*ptrs, *d, one, big, none) == _lib.PT_ERR_NULL
    assert L.pt_label_enc_f32(one, one, one, one, *d, none, big, none) == _lib.PT_ERR_NULL
    assert L.pt_label_enc_f32(one, ctypes.c_void_p(260), one, one, *d, one, big, none) == _lib.PT_ERR_UNSUPPORTED      # misaligned pack
    need = L.pt_label_enc_ws_bytes(*d)
    assert L.pt_label_enc_f32(one, one, one, one, *d, one, need - 1, none) == _lib.PT_ERR_WORKSPACE                    # one byte short
    assert L.pt_label_enc_f32(one, one, one, one, *d, ctypes.c_void_p(384), need, none) == _lib.PT_ERR_WORKSPACE       # misaligned


def test_exports_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "pt_hot.h")) as fh:
        header = fh.read()
    for sym in ("pt_label_enc_pack_floats", "pt_label_enc_ws_bytes", "pt_label_enc_f32"):
        assert sym in _lib.EXPORTS and re.search(r"\b(size_t|int)\s+" + sym + r"\s*\(", header), sym
    assert "label_enc.hip" in _lib.SOURCES


def test_pack_cache_follows_the_module_state():
    net = LC.module("bn_odd")
    p0 = LE.packed_weights(net)
    assert LE.packed_weights(net) is p0                                 # unchanged state: the cached pack
    with torch.no_grad():
        net.res2.bn1.running_var.mul_(2.0)                              # in-place: the version counter moves
    p1 = LE.packed_weights(net)
    assert p1 is not p0 and not torch.equal(p0, p1)
    net.load_state_dict(LC.state_tensors(LC.case("bn_odd")[6]))
    assert torch.equal(LE.packed_weights(net), p0)
    net.samp_w_pred.bias.data = net.samp_w_pred.bias.data + 1.0         # through .data: a new tensor, the data_ptr moves
    assert not torch.equal(LE.packed_weights(net), p0)
    LE.refresh(net)
    assert net not in LE._PACKS


def test_covered_refuses_what_the_kernels_do_not_serve():
    net = LC.module("odd")
    masks = torch.from_numpy(LC.case("odd")[7])[:, None]
    with torch.no_grad():
        assert LE._layers(net) is not None and not LE.covered(net, masks)           # CPU tensor
        with pytest.raises(RuntimeError, match="MI355X"):
            LE.forward(net, masks)
    dims = synth.LABEL_ENC_DIMS
    other = LC.ResidualDS16SW(dims, False).eval()
    other.res1.conv2 = torch.nn.Conv2d(dims[1], dims[1], 3, padding=2, dilation=2, bias=False)
    assert LE._layers(other) is None                                                # a dilated convolution
    other = LC.ResidualDS16SW(dims, False).eval()
    other.res2.downsample = torch.nn.Conv2d(dims[1], dims[2], 3, stride=2, padding=1, bias=False)
    assert LE._layers(other) is None                                                # a bias-free downsample
    other = LC.ResidualDS16SW(dims, False).eval()
    other.conv_block[0] = torch.nn.Conv2d(1, dims[0], 3, stride=2, padding=1, padding_mode="replicate")
    assert LE._layers(other) is None
    other = LC.ResidualDS16SW(dims, True).eval()
    other.label_pred[1] = torch.nn.BatchNorm2d(dims[3], track_running_stats=False)
    assert LE._layers(other) is None                                                # a BatchNorm without running statistics
    assert LE._layers(LC.ResidualDS16SW((16, 24, 64, 16), False).eval()) is not None
    with pytest.raises(NotImplementedError):
        LE.pack_weights(LC.ResidualDS16SW((16, 24, 64, 16), False).eval())          # the structure, but 24 channels
    assert LE._layers(torch.nn.Sequential()) is None


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip, as tests/test_install_ledger.py does; uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(label_encoder=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


def _classes():
    from ltr.models.lwl.label_encoder import ResidualDS16SW as A
    from ltr.models.rts.label_encoder import ResidualDS16SW as B
    return A, B


@needs_reference
def test_install_switch_rebinds_both_classes_and_uninstall_restores(amd):
    import test_install_ledger as TL
    A, B = _classes()
    refs = [c.__dict__["forward"] for c in (A, B)]
    before = TL.snapshot()
    amd.install()                                                       # default: off
    assert [c.__dict__["forward"] for c in (A, B)] == refs
    with open(TL.REBOUND) as fh:
        pinned = json.load(fh)
    base = TL.changed(before, TL.snapshot())
    # the pinned default set; a test module that ran earlier in the session may have left its own stand-in under the sampler's name, which
    # install() then leaves alone (tests/test_install_ledger.py pins the set itself, in a fresh state)
    assert set(base) <= set(pinned) and set(pinned) - set(base) <= {"sys.modules[spatial_correlation_sampler]"}
    amd.uninstall()
    amd.install(label_encoder=True)
    assert TL.changed(before, TL.snapshot()) == sorted(base + NAMES)
    for c, ref in zip((A, B), refs):
        assert c.forward.__wrapped__ is ref and amd.original(c, "forward") is ref
    amd.uninstall()
    assert [c.__dict__["forward"] for c in (A, B)] == refs and TL.changed(before, TL.snapshot()) == []


@needs_reference
@pytest.mark.parametrize("which", [0, 1])
def test_cpu_tensors_take_the_reference_branch(amd, which):
    g, n, H, W, dims, use_bn, sd, masks = LC.case("bn_odd")
    cls = _classes()[which]
    net = cls(layer_dims=dims, use_bn=use_bn)
    net.load_state_dict(LC.state_tensors(sd))
    net.eval()
    m = torch.from_numpy(masks)[:, None]
    with torch.no_grad():
        want = net(m)                                                   # not installed: the reference's own forward
    amd.install(label_encoder=True)
    amd.stats.clear()
    with torch.no_grad():
        got = net(m)
    assert amd.stats["ResidualDS16SW.forward.reference"] == 1 and amd.stats["ResidualDS16SW.forward.fast"] == 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])             # the reference's bits
    assert LC.against_golden(g, got[0].numpy(), got[1].numpy()) <= 1e-5              # another host's fp32 summation order at most
    amd.uninstall()
    amd.install(strict=True, label_encoder=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="ResidualDS16SW"):
        net(m)
