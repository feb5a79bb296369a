"""RTS instance-score encoder and learners fusion (pytracking_amd.rts_fusion, rts_fusion.hip) without a GPU: the exports exist and refuse
bad arguments before any launch; the float64 restatement of the folded-pack arithmetic (tests/rts_fusion_cases.py) on `pack_weights` of the
stand-in reproduces the goldens of the unmodified reference (tools/make_golden_rts_fusion.py) within 4 x their ref_fp32_err, which pins the
pack layout, the BatchNorm fold and the order of the concatenation; the resize restatement equals F.interpolate in float64; calls outside
the hot path are not covered; install(rts_fusion=True) rebinds exactly ResidualDS16SW_Clf.forward and RTSNet.segment_target."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f64_bound
import label_enc_cases as LC
import rts_fusion_cases as RC
from oracle import ref_harness
from pytracking_amd import _lib, rts_fusion as RF, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
NAMES = ["ltr.models.rts.label_encoder.ResidualDS16SW_Clf.forward", "ltr.models.rts.rts_net.RTSNet.segment_target"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADD, CONCAT = _lib.PT_FUSE_ADD, _lib.PT_FUSE_CONCAT


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _layout_floats(dims):
    c0, c1, c2, f = dims
    return sum(o * 9 * i + 2 * o for i, o in ((1, c0), (c0, 2 * c1), (c1, c1), (c1, 2 * c2), (c2, c2), (c2, 2 * f)))


def test_exports_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "pt_hot.h")) as fh:
        header = fh.read()
    for sym in ("pt_score_enc_pack_floats", "pt_score_enc_ws_bytes", "pt_score_enc_f32", "pt_learners_fuse_pack_floats",
                "pt_learners_fuse_f32"):
        assert sym in _lib.EXPORTS and re.search(r"\b(size_t|int)\s+" + sym + r"\s*\(", header), sym
    assert "rts_fusion.hip" in _lib.SOURCES


def test_encoder_sizes_and_argument_checks_do_not_launch(L):
    none, one, big = None, ctypes.c_void_p(256), 1 << 40
    for name in RC.ENC_CASES:
        n, H, W, dims, _ = synth.SCORE_ENC_CASES[name]
        assert L.pt_score_enc_pack_floats(*dims) == _layout_floats(dims), name
        assert L.pt_score_enc_ws_bytes(n, H, W, *dims) > 0, name
    assert L.pt_score_enc_ws_bytes(1024, 1024, 1024, 64, 64, 64, 64) > 0
    for k in range(4):                                                  # unsupported channel counts, one position at a time
        for v in (8, 24, 80, 128):
            dims = [16, 32, 64, 16]
            dims[k] = v
            assert L.pt_score_enc_pack_floats(*dims) == 0 and L.pt_score_enc_ws_bytes(2, 16, 27, *dims) == 0, dims
            assert L.pt_score_enc_f32(one, one, one, one, 2, 16, 27, *dims, one, big, none) == _lib.PT_ERR_UNSUPPORTED
        dims = [16, 32, 64, 16]
        dims[k] = 0
        assert L.pt_score_enc_pack_floats(*dims) == 0 and L.pt_score_enc_ws_bytes(2, 16, 27, *dims) == 0
        assert L.pt_score_enc_f32(one, one, one, one, 2, 16, 27, *dims, one, big, none) == _lib.PT_ERR_SHAPE
    d = (2, 16, 27, 16, 32, 64, 16)
    for k in range(3):                                                  # n, H, W at zero and negative, then beyond the documented bound
        for v in (0, -3):
            z = list(d)
            z[k] = v
            assert L.pt_score_enc_ws_bytes(*z) == 0 and L.pt_score_enc_f32(one, one, one, one, *z, one, big, none) == _lib.PT_ERR_SHAPE
        z = list(d)
        z[k] = 1025
        assert L.pt_score_enc_ws_bytes(*z) == 0 and L.pt_score_enc_f32(one, one, one, one, *z, one, big, none) == _lib.PT_ERR_UNSUPPORTED
    for k in range(3):                                                  # scores, pack, label_enc; sample_w may be null
        ptrs = [one] * 4
        ptrs[k] = none
        assert L.pt_score_enc_f32(*ptrs, *d, one, big, none) == _lib.PT_ERR_NULL
    assert L.pt_score_enc_f32(one, one, one, one, *d, none, big, none) == _lib.PT_ERR_NULL
    need = L.pt_score_enc_ws_bytes(*d)
    for sw in (one, none):                                              # with a null sample_w the checks go on to the workspace
        assert L.pt_score_enc_f32(one, one, one, sw, *d, one, need - 1, none) == _lib.PT_ERR_WORKSPACE                    # one byte short
        assert L.pt_score_enc_f32(one, one, one, sw, *d, ctypes.c_void_p(384), need, none) == _lib.PT_ERR_WORKSPACE       # misaligned
    assert L.pt_score_enc_f32(one, ctypes.c_void_p(260), one, one, *d, one, big, none) == _lib.PT_ERR_UNSUPPORTED          # misaligned pack


def test_fuse_sizes_and_argument_checks_do_not_launch(L):
    none, one = None, ctypes.c_void_p(256)
    for f in (16, 32, 48, 64):
        assert L.pt_learners_fuse_pack_floats(f) == f * 9 * 2 * f + f
    for f in (0, -16, 8, 24, 80):
        assert L.pt_learners_fuse_pack_floats(f) == 0
    d = (1, 16, 16, 27, 30, 52)
    for mode in (ADD, CONCAT):
        for k in (0, 1, 3):                                             # seg_enc, clf_enc, out
            ptrs = [one] * 4
            ptrs[k] = none
            assert L.pt_learners_fuse_f32(*ptrs, *d, mode, none) == _lib.PT_ERR_NULL
        for k in range(6):
            for v in (0, -2):
                z = list(d)
                z[k] = v
                assert L.pt_learners_fuse_f32(one, one, one, one, *z, mode, none) == _lib.PT_ERR_SHAPE
            z = list(d)
            z[k] = 1025
            assert L.pt_learners_fuse_f32(one, one, one, one, *z, mode, none) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_learners_fuse_f32(one, one, none, one, *d, CONCAT, none) == _lib.PT_ERR_NULL               # concat reads the pack
    assert L.pt_learners_fuse_f32(one, one, one, one, *d, 2, none) == _lib.PT_ERR_UNSUPPORTED               # no such mode
    assert L.pt_learners_fuse_f32(one, one, one, one, 1, 24, 16, 27, 30, 52, CONCAT, none) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_learners_fuse_f32(one, one, ctypes.c_void_p(260), one, *d, CONCAT, none) == _lib.PT_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", RC.ENC_CASES)
def test_encoder_pack_arithmetic_reproduces_golden(name, L):
    g, n, H, W, dims, use_bn, sd, scores = RC.enc_case(name)
    assert all(np.array_equal(v, sd[k]) for k, v in synth.label_enc_state(int(g["state_seed"]), dims, use_bn).items())
    pack = RF.pack_weights(RC.enc_module(name)).numpy()
    assert pack.dtype == np.float32 and pack.size == _layout_floats(dims)
    enc, sw = RC.from_pack(pack, dims, scores)
    assert enc.shape == (n, dims[3], H, W) and sw.shape == enc.shape and g["label_enc"].shape == enc.shape
    err = max(float(np.abs(enc - g["label_enc"]).max()), float(np.abs(sw - g["sample_w"]).max()))
    bound = f64_bound.bound(float(g["ref_fp32_err"]))
    print(f"\nrts_fusion_enc_{name}: max |pack arithmetic (float64) - golden| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float(g["ref_fp32_err"]) <= 1e-5
    assert np.abs(sd["samp_w_pred.weight"]).min() > 0 and (g["label_enc"] == 0).any() and (g["sample_w"] < 0).any()
    assert -0.2 <= scores.min() and scores.max() <= 1.0 and (H * W < 35 or (scores.min() < 0 and scores.max() > 0.5))


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
@pytest.mark.parametrize("name", RC.FUSE_CASES)
def test_fuse_pack_arithmetic_reproduces_golden(name, kind, L):
    g, n, f, source, target, sds, seg, clf = RC.fuse_case(name)
    assert all(np.array_equal(v, sds[kind][k]) for k, v in synth.learners_fusion_state(int(g["state_seed"]), f, kind).items())
    pack = RF.pack_fusion(RC.fuse_module(name, kind)).numpy() if kind == "concat" else None
    out = RC.fuse_from_pack(kind, pack, seg[0], clf[0])
    assert out.shape == g["out." + kind].shape == (n, f) + target
    err = float(np.abs(out - g["out." + kind]).max())
    bound = f64_bound.bound(float(g["ref_fp32_err." + kind]))
    print(f"\nrts_fusion_fuse_{name} {kind}: max |float64 restatement - golden| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound and float(g["ref_fp32_err." + kind]) <= 1e-5


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
def test_chain_pack_arithmetic_reproduces_golden(kind, L):
    g, sd_enc, sds, scores, seg = RC.chain_case()
    enc_net, fusion = RC.chain_modules(kind)
    dims = synth.RTS_CHAIN_CASE["dims"]
    enc, _ = RC.from_pack(RF.pack_weights(enc_net).numpy(), dims, scores[0])
    pack = RF.pack_fusion(fusion).numpy() if kind == "concat" else None
    out = RC.fuse_from_pack(kind, pack, seg[0], enc)
    err = float(np.abs(out - g["out." + kind]).max())
    bound = f64_bound.bound(float(g["ref_fp32_err." + kind]))
    print(f"\nrts_fusion_{RC.CHAIN} {kind}: max |float64 restatement - golden| = {err:.3e}, bound {bound:.3e}")
    assert out.shape == (1, dims[3]) + synth.RTS_CHAIN_CASE["target"] and err <= bound


def test_fusion_pack_layout():
    net = RC.fuse_module("f32", "concat")
    pack = RF.pack_fusion(net).numpy()
    w = net.fusion_conv1.weight.detach().numpy()
    np.testing.assert_array_equal(pack[:w.size], w.transpose(0, 2, 3, 1).reshape(-1))
    np.testing.assert_array_equal(pack[w.size:], net.fusion_conv1.bias.detach().numpy())
    with pytest.raises(NotImplementedError):
        RF.pack_fusion(RC.fuse_module("same", "add"))
    with pytest.raises(NotImplementedError):
        RF.pack_fusion(RC.LearnersFusion("concat", 24).eval())


@pytest.mark.parametrize("name", RC.FUSE_CASES)
def test_resize_restatement_equals_interpolate_in_float64(name):
    _, n, f, source, target, _, _, clf = RC.fuse_case(name)
    x = torch.from_numpy(clf[0]).double()
    want = RC.resize(x, target).numpy()
    got = RC.resize_f64(x.numpy(), target)
    err = float(np.abs(got - want).max())
    print(f"\n{name}: {source} -> {target}  max |restatement - F.interpolate (float64)| = {err:.3e}")
    assert got.shape == want.shape == (n, f) + target and err <= 1e-12
    if source == target:
        assert got is not None and np.array_equal(got, x.numpy())
    else:                                                               # no antialiasing: F.interpolate's default
        assert np.array_equal(want, F.interpolate(x, target, mode="bilinear", align_corners=False, antialias=False).numpy())


def test_pack_cache_follows_the_module_state():
    net = RC.enc_module("bn")
    p0 = RF.packed_weights(net)
    assert RF.packed_weights(net) is p0                                 # unchanged state: the cached pack
    with torch.no_grad():
        net.res2.bn1.running_var.mul_(2.0)                              # in-place: the version counter moves
    p1 = RF.packed_weights(net)
    assert p1 is not p0 and not torch.equal(p0, p1)
    net.load_state_dict(RC.state_tensors(RC.enc_case("bn")[6]))
    assert torch.equal(RF.packed_weights(net), p0)
    net.samp_w_pred.bias.data = net.samp_w_pred.bias.data + 1.0         # through .data: a new tensor, the data_ptr moves
    assert not torch.equal(RF.packed_weights(net), p0)
    RF.refresh(net)
    assert net not in RF._PACKS
    fusion = RC.fuse_module("same", "concat")
    q0 = RF.packed_fusion(fusion)
    assert RF.packed_fusion(fusion) is q0
    with torch.no_grad():
        fusion.fusion_conv1.bias.add_(0.5)
    assert not torch.equal(RF.packed_fusion(fusion), q0)


def test_encoder_covered_refuses_what_the_kernels_do_not_serve():
    net = RC.enc_module("odd")
    scores = torch.from_numpy(RC.enc_case("odd")[7])[:, None]
    with torch.no_grad():
        assert RF._layers(net) is not None and not RF.encoder_covered(net, scores)  # CPU tensor
        with pytest.raises(RuntimeError, match="MI355X"):
            RF.encode(net, scores)
    net.train()
    assert not RF.encoder_covered(net, scores)                                      # training mode
    net.eval()
    assert not RF.encoder_covered(net, scores.requires_grad_(True))                 # grad
    assert RF._layers(LC.module("odd")) is None                                     # the stride-2 ResidualDS16SW
    dims = synth.LABEL_ENC_DIMS
    other = RC.ResidualDS16SW_Clf(dims, False).eval()
    other.pool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    assert RF._layers(other) is None                                                # a stride-2 pool
    other = RC.ResidualDS16SW_Clf(dims, False).eval()
    other.res1.conv1 = torch.nn.Conv2d(dims[0], dims[1], 3, stride=2, padding=1, bias=False)
    assert RF._layers(other) is None                                                # a stride-2 convolution
    other = RC.ResidualDS16SW_Clf(dims, False).eval()
    other.res2.downsample = torch.nn.Conv2d(dims[1], dims[2], 3, padding=1, bias=False)
    assert RF._layers(other) is None                                                # a bias-free downsample
    other = RC.ResidualDS16SW_Clf(dims, True).eval()
    other.label_pred[1] = torch.nn.BatchNorm2d(dims[3], track_running_stats=False)
    assert RF._layers(other) is None                                                # a BatchNorm without running statistics
    assert RF._layers(torch.nn.Sequential()) is None                                # a foreign structure
    assert RF._layers(RC.ResidualDS16SW_Clf((16, 24, 64, 16), False).eval()) is not None
    with pytest.raises(NotImplementedError):
        RF.pack_weights(RC.ResidualDS16SW_Clf((16, 24, 64, 16), False).eval())      # the structure, but 24 channels
    with pytest.raises(NotImplementedError):
        RF.pack_weights(LC.module("odd"))


class _Net(torch.nn.Module):
    """The three members RTSNet.segment_target reads."""

    def __init__(self, fusion):
        super().__init__()
        self.target_model, self.decoder, self.fusion_module = torch.nn.Identity(), torch.nn.Identity(), fusion


def test_segment_covered_refuses_what_the_kernels_do_not_serve():
    f = 16
    filt, feat, enc = torch.zeros(1, f, 32, 3, 3), torch.zeros(1, 32, 6, 9), torch.zeros(1, 1, f, 3, 5)
    feats = {"layer1": torch.zeros(1, 8, 24, 36)}
    for kind in RC.FUSION_TYPES:
        net = _Net(RC.LearnersFusion(kind, f)).eval()
        with torch.no_grad():
            assert RF._fusion_kind(net.fusion_module) == kind
            assert not RF.segment_covered(net, filt, feat, feats, enc)              # CPU tensors
            assert not RF.segment_covered(net, filt, feat, feats, None)             # no encoded scores: nothing to fuse
            with pytest.raises(NotImplementedError):
                RF.segment_target(net, filt, feat, feats, enc)
    net = _Net(RC.LearnersFusion("add", f)).eval()
    with torch.no_grad():
        assert not RF.segment_covered(net, filt.repeat(2, 1, 1, 1, 1), feat, feats, enc.repeat(1, 2, 1, 1, 1))        # two sequences
        assert not RF.segment_covered(_Net(torch.nn.Identity()).eval(), filt, feat, feats, enc)                     # a foreign fusion module
        assert not RF.segment_covered(net.train(), filt, feat, feats, enc)                                          # training mode
    assert not RF.segment_covered(net.eval(), filt.clone().requires_grad_(True), feat, feats, enc)                  # grad
    other = RC.LearnersFusion("add", f)
    other.fusion_type = "mul"
    assert RF._fusion_kind(other) is None and RF._fusion_kind(torch.nn.Identity()) is None
    other = RC.LearnersFusion("concat", f)
    other.fusion_conv1 = torch.nn.Conv2d(2 * f, f, 1)
    assert RF._fusion_kind(other) is None                                           # not a 3x3 convolution
    seg, clf = torch.zeros(1, 1, f, 6, 9), torch.zeros(1, 1, f, 3, 5)
    assert not RF.fuse_covered(RC.LearnersFusion("add", f).eval(), seg, clf)        # CPU tensors
    with pytest.raises(RuntimeError, match="MI355X"):
        RF.fuse(RC.LearnersFusion("add", f).eval(), seg, clf)


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip, as tests/test_install_ledger.py does; uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(rts_fusion=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


def _owners():
    from ltr.models.rts.label_encoder import ResidualDS16SW_Clf
    from ltr.models.rts.rts_net import RTSNet
    return (ResidualDS16SW_Clf, "forward"), (RTSNet, "segment_target")


@needs_reference
def test_install_switch_rebinds_exactly_the_two_symbols_and_uninstall_restores(amd):
    import test_install_ledger as TL
    owners = _owners()
    refs = [c.__dict__[a] for c, a in owners]
    before = TL.snapshot()
    amd.install()                                                       # default: off
    assert [c.__dict__[a] for c, a in owners] == refs
    with open(TL.REBOUND) as fh:
        pinned = json.load(fh)
    base = TL.changed(before, TL.snapshot())
    # the pinned default set; a test module that ran earlier in the session may have left its own stand-in under the sampler's name, which
    # install() then leaves alone (tests/test_install_ledger.py pins the set itself, in a fresh state)
    assert set(base) <= set(pinned) and set(pinned) - set(base) <= {"sys.modules[spatial_correlation_sampler]"}
    amd.uninstall()
    amd.install(rts_fusion=True)
    assert TL.changed(before, TL.snapshot()) == sorted(base + NAMES)
    for (c, a), ref in zip(owners, refs):
        assert getattr(c, a).__wrapped__ is ref and amd.original(c, a) is ref
    amd.uninstall()
    assert [c.__dict__[a] for c, a in owners] == refs and TL.changed(before, TL.snapshot()) == []


@needs_reference
def test_cpu_tensors_take_the_reference_branch(amd):
    g, n, H, W, dims, use_bn, sd, scores = RC.enc_case("bn")
    (cls, _), _ = _owners()
    net = cls(layer_dims=dims, use_bn=use_bn)
    net.load_state_dict(RC.state_tensors(sd))
    net.eval()
    s = torch.from_numpy(scores)[:, None]
    with torch.no_grad():
        want = net(s)                                                   # not installed: the reference's own forward
    amd.install(rts_fusion=True)
    amd.stats.clear()
    with torch.no_grad():
        got = net(s)
    assert amd.stats["ResidualDS16SW_Clf.forward.reference"] == 1 and amd.stats["ResidualDS16SW_Clf.forward.fast"] == 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])             # the reference's bits
    err = max(float(np.abs(got[0][:, 0].numpy() - g["label_enc"]).max()), float(np.abs(got[1][:, 0].numpy() - g["sample_w"]).max()))
    assert err <= 1e-5                                                               # another host's fp32 summation order at most
    amd.uninstall()
    amd.install(strict=True, rts_fusion=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="ResidualDS16SW_Clf"):
        net(s)
