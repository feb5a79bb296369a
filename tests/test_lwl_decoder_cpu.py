"""Segmentation decoder (pytracking_amd.lwl_decoder, lwl_decoder.hip) without a GPU: the exports and their size functions, the pack layout
against a numpy re-derivation of the float64 fold, the goldens' own error and size, seeded inputs, what covered() refuses, the install
switch, and the two resize rules the kernels follow against F.interpolate."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lwl_decoder_cases as DC
from oracle import ref_harness
from pytracking_amd import _lib, lwl_decoder as LD, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
NAMES = ["ltr.models.lwl.decoder.LWTLDecoder.forward", "ltr.models.rts.decoder.RTSDecoder.forward"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pt_lwl_decoder_pack_floats", "pt_lwl_decoder_ws_bytes", "pt_lwl_decoder_f32")


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def test_exports_are_declared_in_the_header(L):
    with open(os.path.join(ROOT, "include", "pt_hot.h")) as fh:
        header = fh.read()
    for sym in SYMS:
        assert sym in _lib.EXPORTS and hasattr(L, sym) and re.search(r"\b(size_t|int)\s+" + sym + r"\s*\(", header), sym
    assert "lwl_decoder.hip" in _lib.SOURCES


@pytest.mark.parametrize("name", DC.CASES)
def test_pack_floats_ws_bytes_and_layout(name, L):
    g, c, sd, _, _ = DC.case(name)
    net = DC.module(name)
    pack = LD.pack_weights(net).numpy()
    n, levels, fc, hw, shw, ihw, ic, mdim = DC.c_args(c)
    assert L.pt_lwl_decoder_pack_floats(levels, fc, ic, mdim, int(c["use_bn"])) == pack.size
    assert L.pt_lwl_decoder_ws_bytes(n, levels, fc, hw, shw, ihw, ic, mdim) > 0
    want = DC.pack_np(c, sd)                                              # the float64 fold, re-derived from the state dict
    assert pack.dtype == np.float32 and pack.shape == want.shape
    assert np.array_equal(pack, want)


def test_ws_bytes_is_zero_for_what_is_not_covered(L):
    c = synth.LWL_DECODER_CASES["tiny"]

    def ws(n=None, ic=None, mdim=None, levels=None):
        cc = dict(c, levels=c["levels"] if levels is None else levels)
        a = list(DC.c_args(cc, n))
        a[6] = a[6] if ic is None else ic
        a[7] = a[7] if mdim is None else mdim
        return L.pt_lwl_decoder_ws_bytes(*a)

    lv = c["levels"]
    assert ws() > 0 and ws(n=8) > 0
    assert ws(n=9) == 0 and ws(n=0) == 0
    assert ws(ic=8) == 0 and ws(ic=24) == 0
    assert ws(mdim=16) == 0 and ws(mdim=48) == 0
    assert ws(levels=lv[:2]) == 0                                                     # two levels
    assert ws(levels=(("layer4", 24, 2, 2),) + lv[1:]) == 0                           # fc % 16
    assert ws(levels=(("layer4", 32, 0, 2),) + lv[1:]) == 0
    assert ws(levels=lv[:3] + (("layer1", 16, 30000, 30000),)) == 0                   # beyond 32-bit byte offsets
    a = DC.c_args(c)
    assert L.pt_lwl_decoder_pack_floats(2, a[2], 16, 32, 1) == 0 and L.pt_lwl_decoder_pack_floats(4, a[2], 16, 40, 1) == 0


@pytest.mark.parametrize("name", DC.CASES)
def test_goldens_are_small_accurate_and_regenerate(name):
    g, c, sd, s, feats = DC.case(name)
    assert float(g["ref_fp32_err"]) <= 1e-5
    assert os.path.getsize(os.path.join(DC.GOLDEN, f"lwl_decoder_{name}.npz")) < (1 << 20)
    s2, f2 = synth.lwl_decoder_inputs(int(g["input_seed"]), c["n"], c["ic"], c["levels"], c["scores"])
    sd2 = synth.lwl_decoder_state(int(g["state_seed"]), c["mdim"], c["ic"], c["use_bn"], c["levels"])
    assert np.array_equal(s, s2) and all(np.array_equal(feats[k], f2[k]) for k in feats)
    assert sd.keys() == sd2.keys() and all(np.array_equal(sd[k], sd2[k]) for k in sd)
    H, W = c["image"]
    want = (c["n"], 1, (H + 3) // 4, (W + 3) // 4) if name == "deployed" else (c["n"], 1, H, W)
    assert g["mask"].shape == want
    stored = [q for q in DC.level_names(c) if q in g]
    assert stored == (DC.level_names(c)[:1] if name == "deployed" else DC.level_names(c))
    # the plain-torch module of tests/lwl_decoder_cases.py computes what the reference computed (another host's summation order at most)
    if name != "deployed":
        with torch.no_grad():
            mask, outs = DC.module(name)(*DC.inputs(name), c["image"], DC.level_names(c))
        assert float(np.abs(mask.numpy() - g["mask"]).max()) <= 1e-5
        assert all(float(np.abs(outs[q].numpy() - g[q]).max()) <= 1e-5 for q in stored)


def test_covered_refuses_what_the_kernels_do_not_serve():
    c = synth.LWL_DECODER_CASES["tiny"]
    net = DC.module("tiny")
    s, feats = DC.inputs("tiny")
    assert LD._structure(net) is not None
    with torch.no_grad():
        assert not LD.covered(net, s, feats, c["image"])                                       # CPU tensors
        with pytest.raises(RuntimeError, match="MI355X"):
            LD.forward(net, s, feats, c["image"])
        assert not LD.covered(net, s, feats, c["image"], num_objects=2)
        assert not LD.covered(net, s[:, :, None], feats, c["image"])                           # 6-D scores
    assert not LD.covered(net.train(), s, feats, c["image"])
    net.eval()
    assert not LD.covered(net, s, feats, c["image"])                                           # grad enabled, parameters require it
    assert LD._structure(torch.nn.Sequential()) is None and not LD.covered(torch.nn.Conv2d(1, 1, 1), s, feats, c["image"])
    other = DC.module("tiny")
    other.RRB1["layer2"].bblock[0] = torch.nn.Conv2d(64, 64, 3, padding=2, dilation=2)
    assert LD._structure(other) is None                                                        # a dilated convolution
    other = DC.module("tiny")
    other.TSE["layer1"].transform[1] = torch.nn.LeakyReLU(0.1)
    assert LD._structure(other) is None                                                        # a leaky activation
    other = DC.module("tiny")
    other.CAB["layer4"].deepest = False
    assert LD._structure(other) is None
    with pytest.raises(NotImplementedError):
        LD.pack_weights(torch.nn.Sequential())


def test_pack_cache_follows_the_module_state():
    net = DC.module("tiny")
    p0 = LD.packed_weights(net)
    assert LD.packed_weights(net) is p0
    with torch.no_grad():
        net.RRB2["layer1"].bblock[1].running_var.mul_(2.0)
    p1 = LD.packed_weights(net)
    assert p1 is not p0 and not torch.equal(p0, p1)
    net.load_state_dict(DC.state_tensors(DC.case("tiny")[2]))
    assert torch.equal(LD.packed_weights(net), p0)
    LD.refresh(net)
    assert net not in LD._PACKS


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip, as tests/test_install_ledger.py does; uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(decoder=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


def _classes():
    from ltr.models.lwl.decoder import LWTLDecoder
    from ltr.models.rts.decoder import RTSDecoder
    return LWTLDecoder, RTSDecoder


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
    assert set(base) <= set(pinned) and set(pinned) - set(base) <= {"sys.modules[spatial_correlation_sampler]"}
    amd.uninstall()
    amd.install(decoder=True)
    assert TL.changed(before, TL.snapshot()) == sorted(base + NAMES)
    for c, ref in zip((A, B), refs):
        assert c.forward.__wrapped__ is ref and amd.original(c, "forward") is ref
    amd.uninstall()
    assert [c.__dict__["forward"] for c in (A, B)] == refs and TL.changed(before, TL.snapshot()) == []


@needs_reference
@pytest.mark.parametrize("which", [0, 1])
def test_reference_classes_are_recognised_and_cpu_calls_take_the_reference_branch(amd, which):
    from collections import OrderedDict
    g, c, sd, _, _ = DC.case("tiny")
    net = _classes()[which](c["ic"], c["mdim"], OrderedDict((L, fc) for L, fc, _, _ in c["levels"]), use_bn=c["use_bn"])
    net.load_state_dict(DC.state_tensors(sd))
    net.eval()
    st = LD._structure(net)
    assert st is not None and st["levels"] == tuple(L for L, _, _, _ in c["levels"]) and (st["ic"], st["mdim"]) == (c["ic"], c["mdim"])
    assert np.array_equal(LD.pack_weights(net).numpy(), DC.pack_np(c, sd))
    s, feats = DC.inputs("tiny")
    names = DC.level_names(c)
    with torch.no_grad():
        want = net(s, feats, c["image"], names)
    amd.install(decoder=True)
    amd.stats.clear()
    key = type(net).__name__ + ".forward"
    with torch.no_grad():
        got = net(s, feats, c["image"], names)
    assert amd.stats[key + ".reference"] == 1 and amd.stats[key + ".fast"] == 0
    assert torch.equal(got[0], want[0]) and all(torch.equal(got[1][q], want[1][q]) for q in names)
    assert float(np.abs(got[0].numpy() - g["mask"]).max()) <= 1e-5
    amd.uninstall()
    amd.install(strict=True, decoder=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="Decoder"):
        net(s, feats, c["image"], names)


@needs_reference
@pytest.mark.parametrize("name", ["tiny", "ratio"])
def test_resize_rules_match_interpolate(name):
    """The coordinate conventions the kernels follow, on every (input size -> output size) pair the case runs."""
    c = synth.LWL_DECODER_CASES[name]
    rng = np.random.default_rng(7)
    sizes = [(H, W) for _, _, H, W in c["levels"]]
    pairs = [(c["scores"], hw) for hw in sizes] + [(sizes[k], sizes[k + 1]) for k in range(len(sizes) - 1)]
    for src, dst in pairs:
        x = rng.uniform(-0.5, 0.5, (2, 3) + tuple(src)).astype(np.float32)
        want = x if tuple(src) == tuple(dst) else F.interpolate(torch.from_numpy(x), tuple(dst), mode="bilinear", align_corners=False).numpy()
        err = float(np.abs(DC.bilinear_np(x, dst) - want).max())
        print(f"\nbilinear {src} -> {dst}: {err:.2e}")
        assert err <= 1e-6
    last = sizes[-1]
    up = (2 * last[0], 2 * last[1])
    for src, dst in ((last, up), (up, c["image"])):
        x = rng.uniform(-0.5, 0.5, (2, 3) + tuple(src)).astype(np.float32)
        want = F.interpolate(torch.from_numpy(x), tuple(dst), mode="bicubic", align_corners=False).numpy()
        err = float(np.abs(DC.bicubic_np(x, dst) - want).max())
        print(f"\nbicubic {src} -> {dst}: {err:.2e}")
        assert err <= 1e-6
