"""IoU modulation vectors (pytracking_amd.iou_mod, iou_mod.hip) without a GPU: the float64 restatement (tests/iou_mod_np.py) reproduces
the goldens of the unmodified reference (tools/make_golden_iou_mod.py), the pack layout is the documented one, the C ABI refuses bad
arguments before any launch, pt_iou_mod_window holds every pixel PrRoIPool touches and at most one more on each side, every seeded defect
of the restatement misses the GPU tests' bound by F_MAX, `covered` refuses what the kernels do not serve, install(iou_mod=True) rebinds
exactly one more name than the pinned default set, and calls outside the hot path take the reference branch."""
import ctypes
import json

import numpy as np
import pytest
import torch

import f64_bound
import iou_mod_cases as IC
import iou_mod_np
from oracle import ref_harness
from pytracking_amd import _lib, iou_mod as IM, synth

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
NAME = "ltr.models.bbreg.atom_iou_net.AtomIoUNet.get_modulation"
F_MAX = IC.F_MAX


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _dims(name):
    """the twelve sizes of pt_iou_mod_ws_bytes"""
    n, (c3, h3, w3), (c4, h4, w4), (A, B, D, P3, P4) = synth.IOU_MOD_CASES[name]
    return [n, c3, A, B, c4, D, P3, P4, h3, w3, h4, w4]


@pytest.mark.parametrize("name", IC.CASES)
def test_float64_restatement_reproduces_golden(name):
    """Against the reference's float64 run only the order of summation differs (<= 1e-10); against its fp32 run the distance is the
    recorded ref_fp32_err, which the golden tool held to <= 2.5e-5."""
    g, n, l3, l4, dims, sd, (f3, f4, bb) = IC.case(name)
    o3, o4 = iou_mod_np.get_modulation(sd, f3, f4, bb, IC.S3, IC.S4)
    assert o3.shape == (n, dims[3]) == g["out3"].shape and o4.shape == (n, dims[4]) == g["out4"].shape
    assert g["out3"].dtype == np.float32 and g["out3_f64"].dtype == np.float64
    e64 = max(float(np.abs(o3 - g["out3_f64"]).max()), float(np.abs(o4 - g["out4_f64"]).max()))
    e32 = max(float(np.abs(o3 - g["out3"]).max()), float(np.abs(o4 - g["out4"]).max()))
    print(f"\niou_mod_{name}: max |restatement - reference float64| = {e64:.3e}, - reference fp32 = {e32:.3e}, "
          f"recorded ref_fp32_err = {float(g['ref_fp32_err']):.3e}")
    assert e64 <= 1e-10
    assert e32 <= float(g["ref_fp32_err"]) + 1e-10
    assert float(g["ref_fp32_err"]) <= 2.5e-5
    assert float(np.abs(g["out3_f64"]).max()) > 0.1 and float(np.abs(g["out4_f64"]).max()) > 0.1      # ReLU left something to compare


def test_wholly_outside_and_zero_width_boxes_give_the_tails_response_to_zero():
    g, n, l3, l4, dims, sd, (f3, f4, bb) = IC.case("edges")
    zero = iou_mod_np.get_modulation(sd, np.zeros_like(f3[:1]), np.zeros_like(f4[:1]), np.array([[200.0, 200.0, 10.0, 10.0]]))
    for k in (2, 3):
        assert np.abs(g["out3_f64"][k] - zero[0][0]).max() <= 1e-12 and np.abs(g["out4_f64"][k] - zero[1][0]).max() <= 1e-12
    assert np.abs(g["out3_f64"][0] - zero[0][0]).max() > 1e-2


def _layout(name):
    n, (c3, _, _), (c4, _, _), (A, B, D, P3, P4) = synth.IOU_MOD_CASES[name]
    return [("conv3_1r", A, 9 * c3), ("conv4_1r", D, 9 * c4), ("fc3_1r", B, 9 * A), ("fc34_3r", P3, B + D), ("fc34_4r", P4, B + D)]


def test_pack_layout(L):
    for name in IC.CASES:
        d = _dims(name)
        assert L.pt_iou_mod_pack_floats(*d[1:8]) == sum(o * k + 2 * o for _, o, k in _layout(name)), name
    assert L.pt_iou_mod_pack_floats(100, 16, 16, 64, 16, 16, 16) == 0
    assert L.pt_iou_mod_pack_floats(64, 16, 16, 64, 16, 16, 0) == 0
    # the host packer on a CPU module: documented order and values (include/pt_hot.h)
    g, n, l3, l4, dims, sd, _ = IC.case("chan")
    pack = IM.pack_weights(IC.module("chan")).numpy()
    assert pack.dtype == np.float32 and IM.BLOCKS == tuple(b for b, _, _ in _layout("chan"))
    at = 0
    for blk, o, k in _layout("chan"):
        w = sd[blk + ".0.weight"]
        assert w.shape[0] == o and w.size == o * k
        np.testing.assert_array_equal(pack[at:at + w.size], w.transpose(0, 2, 3, 1).reshape(-1))
        at += w.size
        scale = sd[blk + ".1.weight"].astype(np.float64) / np.sqrt(sd[blk + ".1.running_var"].astype(np.float64) + 1e-5)
        shift = (sd[blk + ".0.bias"].astype(np.float64) - sd[blk + ".1.running_mean"]) * scale + sd[blk + ".1.bias"]
        np.testing.assert_array_equal(pack[at:at + o], scale.astype(np.float32))
        np.testing.assert_array_equal(pack[at + o:at + 2 * o], shift.astype(np.float32))
        at += 2 * o
    assert at == pack.size


def test_pack_cache_follows_the_module_state():
    net = IC.module("one")
    p0 = IM.packed_weights(net)
    assert IM.packed_weights(net) is p0                                 # unchanged state: the cached pack
    with torch.no_grad():
        net.fc34_4r[1].running_var.mul_(2.0)                            # in-place: the version counter moves
    p1 = IM.packed_weights(net)
    assert p1 is not p0 and not torch.equal(p0, p1)
    net.load_state_dict(IC.state_tensors(IC.case("one")[5]))
    assert torch.equal(IM.packed_weights(net), p0)
    net.fc3_1r[0].bias.data = net.fc3_1r[0].bias.data + 1.0             # through .data: a new tensor, the data_ptr moves
    assert not torch.equal(IM.packed_weights(net), p0)
    IM.refresh(net)
    assert net not in IM._PACKS


def test_argument_checks_do_not_launch(L):
    none = None
    one = ctypes.c_void_p(256)
    d = _dims("dimp50")
    big = 1 << 32

    def call(ptrs=None, dims=None, s=(IC.S3, IC.S4), ws=one, ws_bytes=big):
        return L.pt_iou_mod_f32(*([one] * 6 if ptrs is None else ptrs), *(d if dims is None else dims), *s, ws, ws_bytes, none)

    for name in IC.CASES:
        assert L.pt_iou_mod_ws_bytes(*_dims(name)) > 0, name
    for k in range(6):                                                 # every pointer, and the workspace
        ptrs = [one] * 6
        ptrs[k] = none
        assert call(ptrs=ptrs) == _lib.PT_ERR_NULL, k
    assert call(ws=none) == _lib.PT_ERR_NULL
    for k in range(12):                                                # every size at zero, and a negative one
        z = list(d); z[k] = 0
        assert call(dims=z) == _lib.PT_ERR_SHAPE, k
        assert L.pt_iou_mod_ws_bytes(*z) == 0
    z = list(d); z[9] = -3
    assert call(dims=z) == _lib.PT_ERR_SHAPE
    assert call(s=(0.0, IC.S4)) == _lib.PT_ERR_SHAPE and call(s=(IC.S3, -1.0)) == _lib.PT_ERR_SHAPE
    # n > 32, Cin3 % 64, A, B % 16, Cin4 % 64, D, P3, P4 % 16, H3 * W3 > 4096 (65 x 64), H4 * W4 > 4096
    for k, v in ((0, 33), (1, 96), (2, 24), (3, 40), (4, 1000), (5, 8), (6, 250), (7, 72), (8, 65), (10, 65)):
        u = list(d); u[k] = v
        if k in (8, 10):
            u[k + 1] = 64
        assert call(dims=u) == _lib.PT_ERR_UNSUPPORTED, (k, v)
        assert L.pt_iou_mod_ws_bytes(*u) == 0, (k, v)
    for k in range(6):                                                 # every operand misaligned
        ptrs = [one] * 6
        ptrs[k] = ctypes.c_void_p(260)
        assert call(ptrs=ptrs) == _lib.PT_ERR_UNSUPPORTED, k
    need = L.pt_iou_mod_ws_bytes(*d)
    assert call(ws_bytes=need - 1) == _lib.PT_ERR_WORKSPACE            # one byte short
    assert call(ws=ctypes.c_void_p(384), ws_bytes=need) == _lib.PT_ERR_WORKSPACE      # misaligned
    out = (ctypes.c_int * 4)()
    box = (ctypes.c_float * 4)(1, 2, 3, 4)
    assert L.pt_iou_mod_window(None, 0.125, 4, 4, out) == _lib.PT_ERR_NULL and L.pt_iou_mod_window(box, 0.125, 4, 4, None) == _lib.PT_ERR_NULL
    assert L.pt_iou_mod_window(box, 0.125, 0, 4, out) == _lib.PT_ERR_SHAPE and L.pt_iou_mod_window(box, 0.0, 4, 4, out) == _lib.PT_ERR_SHAPE


def _touched(box, P, s, H, W):
    """Brute force, float64: (columns, rows) of the pixels whose bilinear hat (support i - 1 < x < i + 1) overlaps a bin of the P x P grid of
    the xywh box with positive measure in BOTH directions; empty where no bin has an area."""
    x, y, w, h = (float(v) for v in box)
    axes = []
    for lo, ext, size in ((x * s, max(w * s, 0.0), W), (y * s, max(h * s, 0.0), H)):
        hit = set()
        for q in range(P):
            a, b = lo + q * ext / P, lo + (q + 1) * ext / P
            if b > a:
                hit |= {i for i in range(size) if i - 1 < b and i + 1 > a}
        axes.append(hit)
    return (axes[0], axes[1]) if axes[0] and axes[1] else (set(), set())


def test_window_holds_what_the_pooling_touches(L):
    rng = np.random.default_rng(5)
    boxes = [(b, s, H, W, P) for name in IC.CASES for b in IC.case(name)[6][2]
             for s, (_, H, W), P in ((IC.S3, synth.IOU_MOD_CASES[name][1], 3), (IC.S4, synth.IOU_MOD_CASES[name][2], 1))]
    # 1000 seeded boxes, many partly or wholly outside the map; coordinates in quarter pixels, so that x + w is exact in fp32 and the
    # float64 brute force sees the very box the fp32 window arithmetic sees
    for k in range(1000):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        s, P = ((IC.S3, 3), (IC.S4, 1))[k % 2]
        xy = rng.uniform(-0.6, 1.3, 2) * (W, H) / s
        wh = rng.uniform(0.0, 0.9, 2) * (W, H) / s * (rng.random(2) > 0.03)
        boxes.append(((np.round(np.concatenate([xy, wh]) * 4) / 4).astype(np.float32), s, H, W, P))
    empty = 0
    for box, s, H, W, P in boxes:
        win = IM.window(box, s, H, W)
        assert win == (None if (lambda w: w[2] < w[0] or w[3] < w[1])(iou_mod_np.window(box, s, H, W)) else iou_mod_np.window(box, s, H, W)), box
        cols, rows = _touched(box, P, s, H, W)
        if win is None:
            empty += 1
            assert not cols and not rows, (box, s, H, W)
            continue
        x0, y0, x1, y1 = win
        assert 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H
        if cols:
            assert x0 <= min(cols) and max(cols) <= x1 and y0 <= min(rows) and max(rows) <= y1, (box, win, cols, rows)      # every touched pixel
            assert min(cols) - x0 <= 1 and x1 - max(cols) <= 1 and min(rows) - y0 <= 1 and y1 - max(rows) <= 1, (box, win, cols, rows)
    assert empty > 50
    assert IM.window((8, 8, 40, 30), IC.S3, 9, 11) == (1, 1, 6, 5) and IM.window((200, 200, 10, 10), IC.S3, 9, 11) is None
    assert IM.window((10, 20, 120, 60), IC.S3, 20, 19) == (1, 2, 17, 10)          # `tiles`: 17 columns


@pytest.mark.parametrize("defect", iou_mod_np.DEFECTS)
def test_seeded_defects_miss_the_bound(defect):
    """Each defect of the restatement lies more than F_MAX x max(ref_fp32_err, 2^-23 max|want|) from the reference's float64 output on at
    least one small case: the bound of the GPU tests (f64_bound.held with floor=ulp_of_max) rejects it at any factor raised_factor may
    give."""
    best = {}
    for name in IC.SMALL:
        g, n, l3, l4, dims, sd, (f3, f4, bb) = IC.case(name)
        want = IC.want(g)
        got = dict(zip(("out3", "out4"), iou_mod_np.get_modulation(sd, f3, f4, bb, IC.S3, IC.S4, defect=defect)))
        unit = max(float(g["ref_fp32_err"]), f64_bound.ulp_of_max(want))
        best[name] = max(f64_bound.errors(want, got).values()) / unit
        assert not f64_bound.within(f64_bound.errors(want, got), float(g["ref_fp32_err"]), f64_bound.FACTOR, f64_bound.ulp_of_max(want)) \
            or (defect, name) == ("box0_everywhere", "one")            # one image: its own box
    print(f"\n{defect}: err / max(ref_err, floor) per case " + "  ".join(f"{k} {v:.3g}" for k, v in best.items()))
    assert max(best.values()) > F_MAX, best
    assert f64_bound.raised_factor(0.0, F_MAX) == f64_bound.FACTOR


def test_covered_refuses_what_the_kernels_do_not_serve():
    net = IC.module("edges")
    _, n, l3, l4, dims, _, (f3, f4, bb) = IC.case("edges")
    feats, boxes = [torch.from_numpy(f3.copy()), torch.from_numpy(f4.copy())], torch.from_numpy(bb.copy())
    with torch.no_grad():
        assert not IM.covered(net, feats, boxes)                        # CPU tensors
        with pytest.raises(RuntimeError, match="MI355X"):
            IM.get_modulation(net, feats, boxes)
    assert IM._blocks(net) is not None and IM._scales(net) == (IC.S3, IC.S4) and IM._channels(IM._blocks(net)) == (64, 16, 32, 64, 16, 32, 16)
    net.train()
    assert not IM.covered(net, feats, boxes)                            # training mode
    net.eval()
    assert not IM.covered(net, [f.double() for f in feats], boxes.double())         # not fp32
    assert not IM.covered(net, feats[:1], boxes) and not IM.covered(net, feats, boxes[:, :3]) and not IM.covered(net, feats, boxes[0])
    assert not IM.covered(net, feats, boxes[:4])                        # maps whose batch is not n
    for attr, repl in (("fc3_1r", IC.conv(16, 32, padding=1)),          # fc3_1r with padding
                       ("fc34_3r", IC.conv(48, 32, kernel_size=3)),      # a 3x3 fc34
                       ("conv3_1r", IC.conv(64, 16, padding=2, dilation=2)),
                       ("prroi_pool3r", IC.Pool(5, IC.S3)), ("prroi_pool4r", IC.Pool(3, IC.S4)),
                       ("conv4_1r", torch.nn.Sequential(torch.nn.Conv2d(64, 16, 3, padding=1), torch.nn.ReLU()))):
        bad = IC.module("edges")
        setattr(bad, attr, repl)
        assert (IM._blocks(bad.eval()) is None or IM._scales(bad) is None) and not IM.covered(bad, feats, boxes), attr
    nobn = IC.module("edges")
    nobn.fc34_4r[1] = torch.nn.BatchNorm2d(16, track_running_stats=False)
    assert IM._blocks(nobn.eval()) is None


def test_covered_refuses_grad_enabled_calls_and_a_box_on_another_device(monkeypatch):
    """The checks behind `is_cuda`: run with every tensor reporting the device, so that they are reached without a GPU."""
    net = IC.module("edges")
    _, n, l3, l4, dims, _, (f3, f4, bb) = IC.case("edges")
    feats, boxes = [torch.from_numpy(f3.copy()), torch.from_numpy(f4.copy())], torch.from_numpy(bb.copy())
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with torch.no_grad():
        assert IM.covered(net, feats, boxes)                            # the same call, covered once the tensors count as device tensors
        assert not IM.covered(net, feats, boxes.to("meta"))             # bb on another device
        assert not IM.covered(net, feats, boxes.long())
    assert not IM.covered(net, feats, boxes)                            # grad-enabled parameters
    for p in net.parameters():
        p.requires_grad_(False)
    assert IM.covered(net, feats, boxes)
    assert not IM.covered(net, [feats[0].clone().requires_grad_(True), feats[1]], boxes)     # a grad-enabled input
    assert not IM.covered(net, feats, boxes.clone().requires_grad_(True))


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip, as tests/test_install_ledger.py does; uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(iou_mod=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_reference
def test_install_switch_rebinds_one_more_name(amd):
    import test_install_ledger as TL
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    ref = AtomIoUNet.__dict__["get_modulation"]
    before = TL.snapshot()
    amd.install()                                                       # default: off
    assert AtomIoUNet.__dict__["get_modulation"] is ref
    with open(TL.REBOUND) as fh:
        pinned = json.load(fh)
    assert TL.changed(before, TL.snapshot()) == pinned
    amd.uninstall()
    amd.install(iou_mod=True)
    assert TL.changed(before, TL.snapshot()) == sorted(pinned + [NAME])
    assert AtomIoUNet.get_modulation.__wrapped__ is ref and amd.original(AtomIoUNet, "get_modulation") is ref
    amd.uninstall()
    assert AtomIoUNet.__dict__["get_modulation"] is ref and TL.changed(before, TL.snapshot()) == []


@needs_reference
def test_cpu_tensors_take_the_reference_branch(amd):
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    g, n, l3, l4, dims, sd, (f3, f4, bb) = IC.case("atom18")
    f3, f4, bb = f3[:2, :, :6, :5], f4[:2, :, :3, :3], np.array([[4, 6, 20, 30], [-3, 10, 30, 20]], dtype=np.float32)
    amd.install(iou_mod=True)
    net = AtomIoUNet(input_dim=(l3[0], l4[0]), pred_input_dim=(dims[3], dims[4]))
    net.load_state_dict(IC.state_tensors(sd), strict=False)
    net.eval()
    amd.stats.clear()
    args = ([torch.from_numpy(f3.copy()), torch.from_numpy(f4.copy())], torch.from_numpy(bb))
    with torch.no_grad():
        o3, o4 = net.get_modulation(*args)
    assert amd.stats["AtomIoUNet.get_modulation.reference"] == 1 and amd.stats["AtomIoUNet.get_modulation.fast"] == 0
    r3, r4 = iou_mod_np.get_modulation(sd, f3, f4, bb, IC.S3, IC.S4)
    assert o3.shape == (2, dims[3], 1, 1) and np.abs(o3.numpy().reshape(2, -1) - r3).max() < 1e-4 and np.abs(o4.numpy().reshape(2, -1) - r4).max() < 1e-4
    amd.uninstall()
    amd.install(strict=True, iou_mod=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="get_modulation"):
        net.get_modulation(*args)
