"""The LWL / RTS feature heads without a GPU: the C ABI's argument checks (pt_feat_head_ws_bytes / pt_feat_head_f32), the plain-torch
stand-in of tests/feat_head_cases.py against the reference's own constructors and against the committed goldens, what
`install(feature_heads=True)` rebinds and what a default `install()` leaves alone, and the sensitivity of the float64 bound the GPU tests
use: a head with 10-bit weights and a head whose taps start one pixel further must both leave FACTOR x ref_err on every small case.

Every test that measures prints its figures before it asserts (run with -s)."""
import ctypes

import numpy as np
import pytest
import torch

import f64_bound
import feat_head_cases as FC
from oracle import ref_harness
from pytracking_amd import _lib, features as FM, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")


# ------------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------------
def test_workspace_query():
    L = _lib.lib()
    assert L.pt_feat_head_ws_bytes(1, 1024, 512, 30, 52, 2) > 0
    assert L.pt_feat_head_ws_bytes(1, 64, 16, 1, 1, 2) > 0
    assert L.pt_feat_head_ws_bytes(1, 1024, 512, 30, 52, 3) == 0
    assert L.pt_feat_head_ws_bytes(1, 1024, 512, 30, 52, 0) == 0
    assert L.pt_feat_head_ws_bytes(1, 1000, 512, 30, 52, 2) == 0
    assert L.pt_feat_head_ws_bytes(1, 1024, 510, 30, 52, 2) == 0
    for bad in ((0, 1024, 512, 30, 52), (1, 0, 512, 30, 52), (1, 1024, 0, 30, 52), (1, 1024, 512, -1, 52), (1, 1024, 512, 30, 0)):
        assert L.pt_feat_head_ws_bytes(*bad, 2) == 0 and L.pt_feat_head_ws_bytes(*bad, 1) == 0
    for dims in ((1, 1024, 512, 30, 52), (1, 1024, 512, 18, 18), (3, 64, 16, 5, 22), (1, 64, 16, 1, 1)):
        assert L.pt_feat_head_ws_bytes(*dims, 1) == L.pt_clf_head_ws_bytes(*dims) > 0
    # stride 2 holds the input as tokens, nine partial products, their sum and the slice statistics: less than stride 1 at the same map
    assert L.pt_feat_head_ws_bytes(1, 1024, 512, 30, 52, 2) < L.pt_feat_head_ws_bytes(1, 1024, 512, 30, 52, 1)


@pytest.mark.parametrize("stride", [1, 2])
def test_status_codes_come_out_in_order_before_anything_is_queued(stride):
    """NULL pointer, bad shape, unsupported configuration, workspace: -1, -2, -3, -4 (no device is touched: this runs without one)."""
    L = _lib.lib()
    one, n = ctypes.c_void_p(256), ctypes.c_void_p(0)
    args = (1, 1024, 512, 30, 52, stride, 1.0, 1e-5)
    assert L.pt_feat_head_f32(n, one, one, *args, one, 1 << 30, n) == _lib.PT_ERR_NULL == -1
    assert L.pt_feat_head_f32(one, n, one, *args, one, 1 << 30, n) == -1
    assert L.pt_feat_head_f32(one, one, n, *args, one, 1 << 30, n) == -1
    assert L.pt_feat_head_f32(one, one, one, *args, n, 1 << 30, n) == -1
    assert L.pt_feat_head_f32(one, one, one, 0, 1024, 512, 30, 52, stride, 1.0, 1e-5, one, 1 << 30, n) == _lib.PT_ERR_SHAPE == -2
    assert L.pt_feat_head_f32(one, one, one, 1, 1000, 512, 30, 52, stride, 1.0, 1e-5, one, 1 << 30, n) == _lib.PT_ERR_UNSUPPORTED == -3
    assert L.pt_feat_head_f32(one, one, one, 1, 1024, 512, 30, 52, 3, 1.0, 1e-5, one, 1 << 30, n) == -3
    assert L.pt_feat_head_f32(one, one, one, *args, one, 0, n) == _lib.PT_ERR_WORKSPACE == -4
    assert L.pt_feat_head_f32(one, one, one, *args, ctypes.c_void_p(260), 1 << 30, n) == -4          # workspace not 256-byte aligned
    # a bad shape outranks a bad stride, a bad stride a short workspace
    assert L.pt_feat_head_f32(one, one, one, 0, 1024, 512, 30, 52, 3, 1.0, 1e-5, one, 0, n) == -2
    assert L.pt_feat_head_f32(one, one, one, 1, 1024, 512, 30, 52, 3, 1.0, 1e-5, one, 0, n) == -3


def test_exports_and_header_agree():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_hot.h")).read()
    for sym in ("pt_feat_head_ws_bytes", "pt_feat_head_f32"):
        assert sym in _lib.EXPORTS and sym + "(" in hdr
    assert _lib.lib().pt_abi_version() == 1


# ------------------------------------------------------------------------------------------------------
# the stand-in, the reference and the goldens
# ------------------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("name", FC.CASES)
def test_stand_in_is_the_reference_bit_for_bit(name):
    ref_harness.install()
    import ltr.models.target_classifier.features as rfeat
    n, Cin, Cout, H, W = synth.FEAT_HEAD_CASES[name]
    x, w = FC.problem(name)
    s2 = rfeat.residual_bottleneck(feature_dim=Cout, num_blocks=0, l2norm=True, final_conv=True, norm_scale=FC.SCALE, out_dim=Cout,
                                   input_dim=Cin, final_stride=2)
    s1 = rfeat.residual_basic_block(feature_dim=Cin, num_blocks=0, l2norm=True, final_conv=True, norm_scale=FC.SCALE, out_dim=Cout)
    for net, stride in ((s2, 2), (s1, 1)):
        assert list(net.state_dict()) == ["0.weight"]
        net.load_state_dict({"0.weight": w.clone()}, strict=True)
        with torch.no_grad():
            want = net.eval()(x)
        got = FC.standin(x, w, stride)
        assert got.shape == (n, Cout, *FC.out_hw(H, W, stride)) and torch.equal(got, want), (name, stride)


@pytest.mark.parametrize("name", FC.CASES)
def test_goldens_reproduce_from_the_stand_in(name):
    """On any host the golden's stored fp32 output is ref_fp32_err away from the float64 stand-in (to 1e-6 relative: the float64 run's own
    order of summation moves its values by 2^-53 relative); the fp32 stand-in of this host and the golden both lie inside the bound."""
    g = FC.golden(name)
    n, Cin, Cout, H, W = synth.FEAT_HEAD_CASES[name]
    assert tuple(int(g[k]) for k in ("n", "Cin", "Cout", "H", "W")) == (n, Cin, Cout, H, W) and int(g["stride"]) == 2
    assert int(g["seed"]) == FC.SEED + FC.CASES.index(name) and float(g["norm_scale"]) == FC.SCALE and float(g["eps"]) == FC.EPS
    x, w, a = FC.small(name)
    assert np.array_equal(g["weight"], w.numpy()) and (x.numel() <= FC.X_STORED_MAX) == ("x" in g)
    if "x" in g:
        assert np.array_equal(g["x"], x.numpy())
    recorded = float(g["ref_fp32_err"])
    dist = float(np.abs(g["out"].astype(np.float64) - a.want).max())
    here = f64_bound.errors(a.want, FC.standin(x, w, 2))[""]
    print(f"\nfeat_head_{name}: golden ref_fp32_err {recorded:.6e}, max |golden - float64| {dist:.6e}, this host's fp32 stand-in {here:.3e}, "
          f"ref_err {a.ref_err:.3e}, max |v| {np.abs(a.want).max():.3f}")
    assert abs(dist / recorded - 1) <= 1e-6
    assert 0.25 * recorded <= a.ref_err <= 4 * recorded and here <= f64_bound.bound(a.ref_err)
    assert float(np.abs(FC.standin(x, w, 2).numpy() - g["out"]).max()) <= 1e-6


# ------------------------------------------------------------------------------------------------------
# host modules and install dispatch
# ------------------------------------------------------------------------------------------------------
def test_mirror_constructors():
    bb = FM.residual_basic_block(feature_dim=64, num_blocks=0, l2norm=True, final_conv=True, norm_scale=0.5, out_dim=8)
    s2 = FM.residual_bottleneck(feature_dim=16, num_blocks=0, l2norm=True, final_conv=True, out_dim=8, final_stride=2)
    for head, cin, stride in ((bb, 64, 1), (s2, 64, 2)):
        assert isinstance(head, FM.ClfHead) and list(head.state_dict()) == ["0.weight"]
        conv = head[0]
        assert (conv.in_channels, conv.out_channels, conv.stride, conv.padding, conv.bias) == (cin, 8, (stride, stride), (1, 1), None)
    assert bb[1].scale == 0.5
    for kw in (dict(num_blocks=1), dict(l2norm=False), dict(final_conv=False), dict(interp_cat=True), dict(final_relu=True),
               dict(init_pool=True), dict(feature_dim=48), dict(out_dim=6)):
        with pytest.raises(NotImplementedError):
            FM.residual_basic_block(**{**dict(feature_dim=64, num_blocks=0, l2norm=True, final_conv=True, out_dim=8), **kw})
    with pytest.raises(NotImplementedError):
        FM.residual_bottleneck(feature_dim=16, num_blocks=0, final_conv=True, out_dim=8, final_stride=3)
    # the predicate of the default install() still wants stride 1
    kw = dict(feature_dim=16, num_blocks=0, l2norm=True, final_conv=True, out_dim=8)
    assert FM.covered(**kw) and not FM.covered(**kw, final_stride=2)
    assert FM.covered_strided(**kw) and FM.covered_strided(**kw, final_stride=2) and not FM.covered_strided(**kw, final_stride=3)
    assert not FM.covered_strided(**{**kw, "final_pool": True}, final_stride=2)


class _Block(torch.nn.Module):
    """Stands in for torchvision's BasicBlock / Bottleneck where the harness has no torchvision: the constructors only append it."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv = torch.nn.Conv2d(inplanes, planes, 1)


@needs_reference
def test_feature_heads_install_dispatch(monkeypatch):
    """After install(feature_heads=True) both constructors build the fused head around the reference's own layers for the covered
    arguments (same state_dict, CPU call = the reference's nn.Sequential) and return the reference module otherwise; uninstall() restores
    both functions.  A default install() leaves `residual_basic_block` and the stride-2 bottleneck alone."""
    ref_harness.install()
    import ltr.models.target_classifier.features as rfeat
    from pytracking_amd import install as amd
    amd.uninstall()
    for block in ("BasicBlock", "Bottleneck"):
        if not (isinstance(getattr(rfeat, block), type) and issubclass(getattr(rfeat, block), torch.nn.Module)):
            monkeypatch.setattr(rfeat, block, _Block)
    ref_bb, ref_bn = rfeat.residual_basic_block, rfeat.residual_bottleneck
    kw_bb = dict(feature_dim=64, num_blocks=0, final_conv=True, out_dim=8)
    kw_bn = dict(feature_dim=16, num_blocks=0, final_conv=True, out_dim=8, final_stride=2)
    refs = (ref_bb(**kw_bb), ref_bn(**kw_bn))
    amd.install(feature_heads=True)
    try:
        assert rfeat.residual_basic_block.__wrapped__ is ref_bb and rfeat.residual_bottleneck.__wrapped__ is ref_bn
        assert amd.original(rfeat, "residual_basic_block") is ref_bb
        heads = (rfeat.residual_basic_block(**kw_bb), rfeat.residual_bottleneck(**kw_bn))
        amd.stats.clear()
        for head, ref, name in zip(heads, refs, ("residual_basic_block", "residual_bottleneck")):
            assert isinstance(head, FM.ClfHead) and type(head[0]) is torch.nn.Conv2d and type(head[1]).__module__.startswith("ltr.")
            assert list(head.state_dict().keys()) == list(ref.state_dict().keys()) == ["0.weight"]
            head.load_state_dict(ref.state_dict(), strict=True)
            x = torch.randn(2, 64, 5, 6)
            with torch.no_grad():
                assert torch.equal(head.eval()(x), ref.eval()(x))                     # CPU tensor -> the reference's layers
            assert amd.stats[name + ".reference"] == 1 and amd.stats[name + ".fast"] == 0
        assert isinstance(rfeat.residual_bottleneck(feature_dim=16, num_blocks=0, final_conv=True, out_dim=8), FM.ClfHead)   # stride 1 as before
        for fn, base in ((rfeat.residual_basic_block, kw_bb), (rfeat.residual_bottleneck, kw_bn)):
            for kw in (dict(num_blocks=1), dict(l2norm=False), dict(final_relu=True)):
                other = fn(**{**base, **kw})
                assert type(other) is torch.nn.Sequential, (fn.__name__, kw)
    finally:
        amd.uninstall()
    assert rfeat.residual_basic_block is ref_bb and rfeat.residual_bottleneck is ref_bn
    amd.install()
    try:
        assert rfeat.residual_basic_block is ref_bb
        assert type(rfeat.residual_bottleneck(**kw_bn)) is torch.nn.Sequential
        assert isinstance(rfeat.residual_bottleneck(feature_dim=16, num_blocks=0, final_conv=True, out_dim=8), FM.ClfHead)
    finally:
        amd.uninstall()


@needs_reference
def test_strict_install_raises_outside_the_hot_path():
    ref_harness.install()
    import ltr.models.target_classifier.features as rfeat
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(strict=True, feature_heads=True)
    try:
        with pytest.raises(NotImplementedError):
            rfeat.residual_basic_block(feature_dim=64, num_blocks=0, final_conv=True, out_dim=8, l2norm=False)
        with pytest.raises(NotImplementedError):
            rfeat.residual_bottleneck(feature_dim=16, num_blocks=0, final_conv=True, out_dim=8, final_stride=2, final_relu=True)
    finally:
        amd.uninstall()


# ------------------------------------------------------------------------------------------------------
# the bound of the GPU tests catches a wrong head
# ------------------------------------------------------------------------------------------------------
def _ten_bit(w):
    """Weights rounded to nearest at 10 mantissa bits (exact in float64 afterwards)."""
    bits = w.float().contiguous().view(torch.int32)
    return ((bits + 0x1000) & ~0x1FFF).view(torch.float32)


def test_factor_is_the_projects_or_the_tomp_tests():
    """F starts from f64_bound.FACTOR = 4 and may be raised once, to the 6 of the ToMP route tests; no further."""
    assert FC.FACTOR in (4, 6)


@pytest.mark.parametrize("name", FC.CASES)
def test_the_fp32_stand_in_is_inside_the_bound(name):
    x, w, a = FC.small(name)
    f64_bound.held(f"feat_head_{name}, fp32 CPU", FC.standin(x, w, 2), a.want, a.ref_err)


@pytest.mark.parametrize("which", ["weights", "origin"])
@pytest.mark.parametrize("name", FC.CASES)
def test_the_bound_catches_the_mutant(name, which):
    """Both mutants run in float64, so that nothing but the mutation separates them from `want`."""
    x, w, a = FC.small(name)
    if which == "weights":
        got = FC.standin(x.double(), _ten_bit(w).double(), 2)
    else:
        got = FC.standin(x.double(), w.double(), 2, origin=0)
    err = f64_bound.errors(a.want, got)[""]
    print(f64_bound.report(f"feat_head_{name}, mutant {which}", {"": err}, a.ref_err) + f"  (under the flat 1e-4: {err <= 1e-4})")
    assert err > f64_bound.bound(a.ref_err)
    assert err > 6 * a.ref_err                                   # also at the one value FACTOR may be raised to
