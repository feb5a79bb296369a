"""Box label encoders (pytracking_amd.box_encoder, box_enc.hip) without a GPU: the restatement of the pack arithmetic
(tests/box_enc_cases.py) reproduces the goldens of the unmodified reference (tools/make_golden_box_enc.py), which pins the pack layout,
the [feat | trunk] permutation, the zero padding and the BatchNorm fold; pt_box_slice is Python's slice; the stand-ins' rasteriser is the
reference's; the C ABI refuses bad arguments before any launch; install(box_encoder=True) rebinds the four forwards and nothing else
beyond the pinned default set; the float64 bound of tests/test_gpu_box_enc.py rejects three perturbations; k_bx_conv's resources are what
DESIGN.md says."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import box_enc_cases as BC
import f64_bound
from oracle import ref_harness
from pytracking_amd import _lib, box_encoder as BE, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(f"ltr.models.{pkg}.label_encoder.{cls}.forward" for pkg in ("lwl", "rts") for cls in (BE.BOX, BE.CAT))
LABEL_NAMES = ["ltr.models.lwl.label_encoder.ResidualDS16SW.forward", "ltr.models.rts.label_encoder.ResidualDS16SW.forward"]


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _ceil16(v):
    return -(-v // 16) * 16


def _layout_floats(kind, c):
    """The header's layout formula: per layer Cout * 9 * Cin (padded to 16 behind the trunk) weights, Cout scales, Cout shifts."""
    d, fd = c["dims"], c["feat_dim"]
    if kind == BC.BOX:
        c0, c1, c2, c3, f = d
        trunk = [(1, c0), (c0, 2 * c1), (c1, c1), (c1, 2 * c2), (c2, c2)]
        rest = [(fd + c2, 2 * c3), (c3, c3), (c3, 2 * f if c["use_sample_w"] else f)]
        return sum(o * 9 * i + 2 * o for i, o in trunk) + sum(o * 9 * _ceil16(i) + 2 * o for i, o in rest)
    layers, cin = [], fd + 1
    for width in d[:-1]:
        layers += [(cin, 2 * width), (width, width)]
        cin = width
    layers.append((cin, d[-1]))
    return sum(o * 9 * _ceil16(i) + 2 * o for i, o in layers)


def _layers_crossed(kind, c):
    """Folded layers on the longest path from the input to an output."""
    return 8 if kind == BC.BOX else 2 * (len(c["dims"]) - 1) + 1


@pytest.mark.parametrize("kind,name", BC.ALL)
def test_pack_arithmetic_reproduces_golden(kind, name, L):
    """float64 arithmetic on the fp32 pack against the reference's fp32 output: the distance is the reference's own rounding
    (ref_fp32_err) plus the rounding of the folded scale / shift to fp32 -- at most one part in 2^24 of values of magnitude max_abs per
    folded layer a path crosses (tests/test_label_enc_cpu.py)."""
    g, c, sd, boxes, feat = BC.case(kind, name)
    net = BC.module(kind, name)
    pack = BE.pack_weights(net).numpy()
    assert pack.dtype == np.float32 and pack.size == _layout_floats(kind, c)
    out = BC.from_pack(kind, pack, c, boxes, feat)
    assert list(out) == list(BC.outputs(kind, c))
    err = max(float(np.abs(out[q] - g[q]).max()) for q in out)
    bound = float(g["ref_fp32_err"]) + _layers_crossed(kind, c) * float(g["max_abs"]) * 2.0 ** -24 + 1e-12
    print(f"\n{kind}_{name}: max |pack arithmetic (float64) - golden| = {err:.3e}, bound {bound:.3e}, ref_fp32_err {float(g['ref_fp32_err']):.3e}")
    assert err <= bound
    assert float(g["ref_fp32_err"]) <= 1e-5 and float(np.abs(g["label_enc"]).max()) > 0.1


def test_pack_permutes_res3_and_pads_the_mask_channel():
    g, c, sd, _, _ = BC.case(BC.BOX, "odd")
    c2, fd, c3 = c["dims"][2], c["feat_dim"], c["dims"][3]
    pack = BE.pack_weights(BC.module(BC.BOX, "odd")).numpy()
    at = L_trunk = sum(o * 9 * i + 2 * o for i, o in ((1, c["dims"][0]), (c["dims"][0], 2 * c["dims"][1]), (c["dims"][1], c["dims"][1]),
                                                      (c["dims"][1], 2 * c2), (c2, c2)))
    w = pack[at:at + 2 * c3 * 9 * (fd + c2)].reshape(2 * c3, 3, 3, fd + c2)
    for half, key in ((slice(0, c3), "res3.conv1.weight"), (slice(c3, 2 * c3), "res3.downsample.weight")):
        ref = sd[key].transpose(0, 2, 3, 1)                                         # (Cout, 3, 3, [trunk | feat])
        np.testing.assert_array_equal(w[half][..., :fd], ref[..., c2:])
        np.testing.assert_array_equal(w[half][..., fd:], ref[..., :c2])
    assert L_trunk > 0
    g, c, sd, _, _ = BC.case(BC.CAT, "blocks1")
    fd, width = c["feat_dim"], c["dims"][0]
    pack = BE.pack_weights(BC.module(BC.CAT, "blocks1")).numpy()
    cinp = _ceil16(fd + 1)
    w = pack[:2 * width * 9 * cinp].reshape(2 * width, 3, 3, cinp)
    np.testing.assert_array_equal(w[:width, ..., :fd + 1], sd["res.0.conv1.weight"].transpose(0, 2, 3, 1))
    assert not w[..., fd + 1:].any()
    scale = pack[2 * width * 9 * cinp:2 * width * 9 * cinp + 2 * width]
    want = sd["res.0.bn1.weight"].astype(np.float64) / np.sqrt(sd["res.0.bn1.running_var"].astype(np.float64) + 1e-5)
    np.testing.assert_array_equal(scale[:width], want.astype(np.float32))
    np.testing.assert_array_equal(scale[width:], np.ones(width, np.float32))      # the downsample has no BatchNorm


@pytest.mark.parametrize("clamp", [0, 1])
def test_box_slice_is_pythons_slice(L, clamp):
    lo, hi = ctypes.c_int(), ctypes.c_int()
    for length in (1, 5, 8):
        for start in range(-12, 13):
            for extent in range(-12, 13):
                assert L.pt_box_slice(start, extent, length, clamp, ctypes.byref(lo), ctypes.byref(hi)) == 0
                got = list(range(lo.value, hi.value))
                want = list(range(length))[(max(0, start) if clamp else start):start + extent]
                assert got == want, (length, start, extent, clamp, got, want)
                assert BC.slice_rule(start, extent, length, bool(clamp)) == (lo.value, hi.value)
    assert L.pt_box_slice(0, 1, 0, clamp, ctypes.byref(lo), ctypes.byref(hi)) == _lib.PT_ERR_SHAPE
    assert L.pt_box_slice(0, 1, 4, clamp, None, ctypes.byref(hi)) == _lib.PT_ERR_NULL
    assert L.pt_box_slice(1 << 30, 1, 4, clamp, ctypes.byref(lo), ctypes.byref(hi)) == _lib.PT_ERR_UNSUPPORTED


@needs_reference
@pytest.mark.parametrize("kind,name", BC.ALL)
def test_standin_rasteriser_is_the_references(kind, name):
    ref_harness.install()
    from ltr.models.lwl import label_encoder as M
    _, c, _, boxes, _ = BC.case(kind, name)
    cls = M.ResidualDS16FeatSWBox if kind == BC.BOX else M.ResidualDS16FeatSWBoxCatMultiBlock
    bb = torch.from_numpy(boxes)
    want = cls.bbox_to_mask(None, bb, c["image"])
    assert torch.equal(BC.box_mask(bb, c["image"], kind == BC.BOX), want)
    assert torch.equal(BC.mask_from_rule(bb, c["image"], kind == BC.BOX, torch.float32), want)


def test_sizes_and_argument_checks_do_not_launch(L):
    none, one, big = None, ctypes.c_void_p(256), 1 << 40
    for kind, name in BC.ALL:
        c = BC.config(kind, name)
        (H, W), (h, w) = c["image"], c["feat"]
        if kind == BC.BOX:
            assert L.pt_box_enc_pack_floats(*c["dims"], c["feat_dim"], int(c["use_sample_w"])) == _layout_floats(kind, c), name
            assert L.pt_box_enc_ws_bytes(c["n"], H, W, h, w, *c["dims"], c["feat_dim"]) > 0, name
        else:
            dims = (ctypes.c_int * len(c["dims"]))(*c["dims"])
            assert L.pt_box_cat_enc_pack_floats(len(c["dims"]) - 1, dims, c["feat_dim"]) == _layout_floats(kind, c), name
            assert L.pt_box_cat_enc_ws_bytes(c["n"], H, W, h, w, len(c["dims"]) - 1, dims, c["feat_dim"]) > 0, name
    # ---- FeatSWBox: (n, H, W, h, w, c0, c1, c2, c3, f, feat_dim)
    d = [2, 33, 50, 3, 4, 16, 32, 64, 128, 16, 512]

    def box(args, ptrs=(one,) * 5, img=None, ws=one, nbytes=big, relu=1):
        img = args[10] * args[3] * args[4] if img is None else img
        return L.pt_box_enc_f32(ptrs[0], ptrs[1], img, ptrs[2], ptrs[3], ptrs[4], *args, relu, ws, nbytes, none)

    need = L.pt_box_enc_ws_bytes(*d)
    assert need > 0 and L.pt_box_enc_f32.argtypes is not None
    for k in range(4):                                                  # boxes, feat, pack, label_enc; a null sample_w is allowed
        ptrs = [one] * 5
        ptrs[k] = none
        assert box(d, ptrs) == _lib.PT_ERR_NULL
    assert box(d, ws=none) == _lib.PT_ERR_NULL
    for k in range(11):
        for v in (0, -3):
            z = list(d)
            z[k] = v
            assert L.pt_box_enc_ws_bytes(*z) == 0 and box(z, img=1 << 30) == _lib.PT_ERR_SHAPE, (k, v)
    assert box(d, img=d[10] * d[3] * d[4] - 1) == _lib.PT_ERR_SHAPE     # an image stride below one image
    for k, values in ((5, (8, 24, 80)), (6, (8, 80)), (7, (24, 128)), (8, (8, 24, 144)), (9, (8, 136)), (10, (8, 520, 1040))):
        for v in values:
            z = list(d)
            z[k] = v
            assert L.pt_box_enc_ws_bytes(*z) == 0 and box(z) == _lib.PT_ERR_UNSUPPORTED, (k, v)
            assert L.pt_box_enc_pack_floats(*z[5:], 1) == 0
    for hw in ((3, 5), (2, 4), (30, 52)):                               # the feature size must be the trunk's output size
        z = list(d)
        z[3:5] = hw
        assert L.pt_box_enc_ws_bytes(*z) == 0 and box(z) == _lib.PT_ERR_UNSUPPORTED
    assert L.pt_box_enc_ws_bytes(2000, *d[1:]) == 0 and L.pt_box_enc_ws_bytes(2, 9000, 50, 563, 4, *d[5:]) == 0
    assert box(d, (one, one, ctypes.c_void_p(260), one, one)) == _lib.PT_ERR_UNSUPPORTED      # misaligned pack
    assert box(d, (one, ctypes.c_void_p(258), one, one, one)) == _lib.PT_ERR_UNSUPPORTED      # a feature off a 4-byte boundary
    assert box(d, nbytes=need - 1) == _lib.PT_ERR_WORKSPACE and box(d, ws=ctypes.c_void_p(384), nbytes=need) == _lib.PT_ERR_WORKSPACE
    assert box(d, (one, one, one, one, none), nbytes=need - 1) == _lib.PT_ERR_WORKSPACE       # without sample_w: the same workspace
    # ---- Cat: (n, H, W, h, w, nblocks, dims, feat_dim)
    def cat(n=2, H=33, W=50, h=5, w=7, dims=(64, 64, 16), fd=512, ptrs=(one,) * 4, img=None, ws=one, nbytes=big, nb=None, dims_ptr=True):
        arr = (ctypes.c_int * len(dims))(*dims) if dims_ptr else None
        nb = len(dims) - 1 if nb is None else nb
        img = fd * h * w if img is None else img
        return (L.pt_box_cat_enc_f32(ptrs[0], ptrs[1], img, ptrs[2], ptrs[3], n, H, W, h, w, nb, arr, fd, 1, ws, nbytes, none),
                L.pt_box_cat_enc_ws_bytes(n, H, W, h, w, nb, arr, fd))

    rc, need = cat()
    assert need > 0 and cat(nbytes=need - 1)[0] == _lib.PT_ERR_WORKSPACE and cat(ws=ctypes.c_void_p(384), nbytes=need)[0] == _lib.PT_ERR_WORKSPACE
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = none
        assert cat(ptrs=ptrs)[0] == _lib.PT_ERR_NULL
    assert cat(ws=none)[0] == _lib.PT_ERR_NULL and cat(dims_ptr=False) == (_lib.PT_ERR_NULL, 0)
    for kw in (dict(n=0), dict(H=-1), dict(W=0), dict(h=0), dict(w=-2), dict(fd=0), dict(dims=(64, 0, 16)), dict(nb=0), dict(img=100)):
        got = cat(**kw)
        assert got[0] == _lib.PT_ERR_SHAPE and (got[1] == 0 or "img" in kw), kw
    for kw in (dict(dims=(1, 16)), dict(dims=(64, 24, 16)), dict(dims=(144, 16)), dict(dims=(64, 8)), dict(fd=520), dict(fd=1040),
               dict(dims=(16,) * 6), dict(n=2000), dict(h=1025), dict(W=9000)):
        assert cat(**kw) == (_lib.PT_ERR_UNSUPPORTED, 0), kw            # the class's default layer_dims has a 1-channel block
    assert cat(ptrs=(one, one, ctypes.c_void_p(264), one))[0] == _lib.PT_ERR_UNSUPPORTED
    for nb in (1, 2, 3, 4):
        assert cat(dims=(32,) * nb + (16,))[1] > 0


def test_exports_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "pt_hot.h")) as fh:
        header = fh.read()
    for sym in ("pt_box_enc_pack_floats", "pt_box_enc_ws_bytes", "pt_box_enc_f32", "pt_box_cat_enc_pack_floats", "pt_box_cat_enc_ws_bytes",
                "pt_box_cat_enc_f32", "pt_box_slice"):
        assert sym in _lib.EXPORTS and re.search(r"\b(size_t|int)\s+" + sym + r"\s*\(", header), sym
    assert "box_enc.hip" in _lib.SOURCES and "box_slice.h" in _lib.HEADERS


def test_recogniser_and_covered_refuse_what_the_kernels_do_not_serve():
    for kind, name in ((BC.BOX, "odd"), (BC.CAT, "odd")):
        _, c, _, boxes, feat = BC.case(kind, name)
        net = BC.module(kind, name)
        args = BC.call_args(kind, c, boxes, feat)
        with torch.no_grad():
            assert BE._recognise(net) is not None and not BE.covered(net, *args)                 # CPU tensors
            with pytest.raises(RuntimeError, match="MI355X"):
                BE.forward(net, *args)
        gauss = copy.deepcopy(net)
        gauss.use_gauss = True
        assert BE._recognise(gauss) is None
        with pytest.raises(NotImplementedError, match="use_gauss=False"):
            BE.pack_weights(gauss)
        renamed = type("Other" + type(net).__name__, (type(net),), {})
        other = copy.deepcopy(net)
        other.__class__ = renamed
        assert BE._recognise(other) is None                                                      # a wrong class name
    c = BC.config(BC.BOX, "odd")
    broken = BC.build(BC.BOX, c).eval()
    broken.res3 = BC.BasicBlock(c["dims"][2] + c["feat_dim"], c["dims"][3] + 16, 1, False)
    assert BE._recognise(broken) is None                                                         # res3 -> label_pred does not chain
    broken = BC.build(BC.BOX, c).eval()
    broken.res2.conv2 = torch.nn.Conv2d(c["dims"][2], c["dims"][2], 3, padding=2, dilation=2, bias=False)
    assert BE._recognise(broken) is None
    c = BC.config(BC.CAT, "blocks3")
    broken = BC.build(BC.CAT, c).eval()
    broken.res[1] = BC.BasicBlock(c["dims"][0] + 16, c["dims"][1], 1, True)
    assert BE._recognise(broken) is None
    default = BC.ResidualDS16FeatSWBoxCatMultiBlock((64, 1, 16), 32).eval()                      # a 1-channel block: the structure, not the dims
    assert BE._recognise(default) is not None
    with pytest.raises(NotImplementedError):
        BE.pack_weights(default)
    assert BE._recognise(torch.nn.Sequential()) is None
    assert BE._recognise(BC.build(BC.BOX, BC.config(BC.BOX, "nosw")).eval()).with_sw is False


def test_pack_cache_follows_the_module_state():
    net = BC.module(BC.CAT, "blocks1")
    p0 = BE.packed_weights(net)
    assert BE.packed_weights(net) is p0
    with torch.no_grad():
        net.res[0].bn1.running_var.mul_(2.0)
    p1 = BE.packed_weights(net)
    assert p1 is not p0 and not torch.equal(p0, p1)
    net.res[0].conv1.weight.data[0, 0, 0, 0] += 1.0                     # through .data: no version counter moves
    assert BE.packed_weights(net) is p1
    BE.refresh(net)
    assert net not in BE._PACKS and not torch.equal(BE.packed_weights(net), p1)


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 bound of the GPU test discriminates

def _perturbed(kind, name, what):
    net = copy.deepcopy(BC.module(kind, name)).double()
    if what == "eps":
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eps *= 2
    elif what == "weights":
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.Conv2d):
                    mant, exp = torch.frexp(m.weight)
                    m.weight.copy_(torch.ldexp(torch.round(mant * 2048) / 2048, exp))          # 10 bits behind the leading one
    else:
        net.box_shift = 1
    return net


@pytest.mark.parametrize("kind,name", [kn for kn in BC.ALL if BC.shift_visible(*kn)])
def test_bound_rejects_perturbed_standins(kind, name):
    """At FACTOR x max(ref_err, one ulp of the range) a stand-in with every BatchNorm eps doubled, one with 10-bit weights and one with
    the box moved by a pixel all fail, on every case whose input can show a moved box (box_enc_cases.shift_visible)."""
    _, c, _, boxes, feat = BC.case(kind, name)
    a = BC.anchor(kind, name)
    bound = f64_bound.bound(a.ref_err, floor=f64_bound.spacing_of_max(a.want))
    for what in ("eps", "weights", "box"):
        out = BC.run(kind, _perturbed(kind, name, what), BC.call_args(kind, c, boxes, feat, dtype=torch.float64), c)
        err = max(f64_bound.errors(a.want, {q: t.numpy() for q, t in out.items()}).values())
        print(f"\n{kind}_{name} {what}: max |perturbed - float64| = {err:.3e} ({err / bound:.1f} x the bound {bound:.3e})")
        assert err > bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# install(box_encoder=True)

@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(box_encoder=True, label_encoder=True)                   # warm-up: every module either switch imports
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


def _classes():
    from ltr.models.lwl import label_encoder as A
    from ltr.models.rts import label_encoder as B
    return [getattr(m, n) for m in (A, B) for n in (BE.BOX, BE.CAT)]


@needs_reference
def test_install_switch_rebinds_the_four_forwards_and_uninstall_restores(amd):
    import test_install_ledger as TL
    classes = _classes()
    refs = [c.__dict__["forward"] for c in classes]
    before = TL.snapshot()
    amd.install()                                                       # default: off
    assert [c.__dict__["forward"] for c in classes] == refs
    with open(TL.REBOUND) as fh:
        pinned = json.load(fh)
    base = TL.changed(before, TL.snapshot())
    assert set(base) <= set(pinned) and set(pinned) - set(base) <= {"sys.modules[spatial_correlation_sampler]"}
    amd.uninstall()
    amd.install(box_encoder=True)
    assert TL.changed(before, TL.snapshot()) == sorted(base + NAMES)
    for c, ref in zip(classes, refs):
        assert c.forward.__wrapped__ is ref and amd.original(c, "forward") is ref
    amd.uninstall()
    amd.install(label_encoder=True)                                     # the older switch still rebinds exactly its two names
    assert TL.changed(before, TL.snapshot()) == sorted(base + LABEL_NAMES)
    amd.uninstall()
    assert [c.__dict__["forward"] for c in classes] == refs and TL.changed(before, TL.snapshot()) == []


@needs_reference
@pytest.mark.parametrize("which", range(4))
def test_cpu_tensors_take_the_reference_branch(amd, which):
    kind = (BC.BOX, BC.CAT)[which % 2]
    name = "bn" if kind == BC.BOX else "blocks3"
    g, c, sd, boxes, feat = BC.case(kind, name)
    cls = _classes()[which]
    kw = dict(layer_dims=c["dims"], feat_dim=c["feat_dim"], use_final_relu=c["final_relu"], use_gauss=False, use_bn=c["use_bn"])
    net = cls(use_sample_w=c["use_sample_w"], **kw) if kind == BC.BOX else cls(final_bn=c["final_bn"], **kw)
    net.load_state_dict(BC.state_tensors(sd))
    net.eval()
    args = BC.call_args(kind, c, boxes, feat)
    want = BC.run(kind, net, args, c)                                   # not installed: the reference's own forward
    amd.install(box_encoder=True)
    amd.stats.clear()
    got = BC.run(kind, net, args, c)
    cname = type(net).__name__
    assert amd.stats[cname + ".forward.reference"] == 1 and amd.stats[cname + ".forward.fast"] == 0
    assert all(torch.equal(got[q], want[q]) for q in want)              # the reference's bits
    assert max(float(np.abs(got[q].numpy() - g[q]).max()) for q in got) <= 1e-5
    amd.uninstall()
    amd.install(strict=True, box_encoder=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match=cname):
        net(*args)


# ---------------------------------------------------------------------------------------------------------------------------
# compiled code

def test_bx_conv_resources(tmp_path_factory):
    """Every k_bx_conv instantiation: no scratch, and the LDS size (16 planes of 120 floats) and occupancy DESIGN.md section 7k states
    for it (the two register sets of weight pieces cost occupancy; the deployed grids are one workgroup per CU)."""
    import test_isa_properties as ISA
    res = ISA._resources("box_enc", tmp_path_factory)
    conv = ISA._pick(res, "k_bx_conv")
    assert len(conv) == 3, sorted(conv)
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    claimed = {int(t): (int(lds), int(occ)) for t, lds, occ in
               re.findall(r"`k_bx_conv<(\d)>` \| (\d+) B of LDS, occupancy (\d+), no scratch", design)}
    assert sorted(claimed) == [1, 2, 4], "DESIGN.md section 7k states LDS size and occupancy of every instantiation"
    for k, v in conv.items():
        t = int(re.search(r"k_bx_convILi(\d)E", k).group(1))
        print(k, v)
        assert v["scratch"] == 0, (k, v)
        assert (v["lds"], v["occupancy"]) == claimed[t] and v["lds"] == 16 * 120 * 4, (k, v, claimed[t])
    for k, v in ISA._pick(res, "k_bx_mask").items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)
