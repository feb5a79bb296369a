"""Segmentation read-out, object merge and mask patch (pytracking_amd.seg_readout, seg_readout.hip) without a GPU: the exports exist and
refuse bad arguments before any launch; the float64 restatements of tests/seg_readout_cases.py reproduce the goldens of the unmodified
reference (tools/make_golden_seg_readout.py) within FACTOR x their ref_fp32_err (tests/f64_bound.py) (measured by the generator against float64 torch code of its own, not against these restatements);
the restated fp32 nearest indices reproduce the golden mask patches bit for bit, where the float64 formula does not; the host placement
rule reproduces the reference's window; install(seg_readout=True) rebinds exactly five symbols and hands CPU tensors to the reference."""
import ctypes
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import f64_bound
import seg_readout_cases as SC
from oracle import ref_harness
from pytracking_amd import _lib, seg_readout as SR

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pytracking.tracker.lwl.lwl.LWL.convert_scores_crop_to_image", "pytracking.tracker.lwl.lwl.LWL.merge_results",
         "pytracking.tracker.rts.rts.RTS.convert_seg_scores_crop_to_image", "pytracking.tracker.rts.rts.RTS.merge_results",
         "pytracking.tracker.rts.sta_helper.STAHelper.convert_scores_crop_to_image"]
SYMBOLS = ("pt_seg_readout_ws_bytes", "pt_seg_readout_f32", "pt_seg_state_ws_bytes", "pt_seg_state_f32", "pt_seg_merge_ws_bytes",
           "pt_seg_merge_f32", "pt_sample_mask_patch_f32")


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def test_exports_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "pt_hot.h")) as fh:
        header = fh.read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and re.search(r"\b(size_t|int)\s+" + sym + r"\s*\(", header), sym
    assert "seg_readout.hip" in _lib.SOURCES
    for name, value in (("PT_SEG_STATS_FLOATS", SR.STATS), ("PT_SEG_MAX_OBJECTS", SR.MAX_OBJECTS), ("PT_SEG_MAX_DIM", SR.MAX_DIM)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name


def test_bad_arguments_are_refused_before_any_launch(L):
    none, one, big = None, ctypes.c_void_p(256), 1 << 40
    NULL, SHAPE, UNSUP, WS = _lib.PT_ERR_NULL, _lib.PT_ERR_SHAPE, _lib.PT_ERR_UNSUPPORTED, _lib.PT_ERR_WORKSPACE
    top = SR.MAX_DIM
    # read-out: scores, Hc, Wc, scale, Hr, Wr, r1, c1, Hi, Wi, scores_im, prob_im, mask_im, stats, ws, ws_bytes, stream
    d = [12, 20, 0.61, 7, 12, 4, 2, 16, 16]
    ok = [one, *d, one, one, one, one, one, big, none]
    assert L.pt_seg_readout_ws_bytes(16, 16) > 0 and L.pt_seg_readout_ws_bytes(0, 16) == 0 and L.pt_seg_readout_ws_bytes(16, top + 1) == 0
    for k in (0, 13, 14):                                               # scores, stats, workspace; the three images may be null
        a = list(ok)
        a[k] = none
        assert L.pt_seg_readout_f32(*a) == NULL
    for k in (1, 2, 4, 5, 8, 9):
        for v in (0, -3):
            a = list(ok)
            a[k] = v
            assert L.pt_seg_readout_f32(*a) == SHAPE
        a = list(ok)
        a[k] = top + 1
        assert L.pt_seg_readout_f32(*a) == UNSUP
    for v in (0.0, -1.0, float("nan")):
        a = list(ok)
        a[3] = v
        assert L.pt_seg_readout_f32(*a) == SHAPE
    for k in (6, 7):
        for v in (top + 1, -top - 1):
            a = list(ok)
            a[k] = v
            assert L.pt_seg_readout_f32(*a) == UNSUP
    need = L.pt_seg_readout_ws_bytes(16, 16)
    a = list(ok)
    a[15] = need - 1
    assert L.pt_seg_readout_f32(*a) == WS
    a = list(ok)
    a[14] = ctypes.c_void_p(384)
    assert L.pt_seg_readout_f32(*a) == WS
    # state: prob, mask, H, W, stats, ws, ws_bytes, stream
    assert L.pt_seg_state_ws_bytes(16, 16) == need and L.pt_seg_state_ws_bytes(-1, 16) == 0
    for k in (0, 4, 5):
        a = [one, one, 16, 16, one, one, big, none]
        a[k] = none
        assert L.pt_seg_state_f32(*a) == NULL
    for k in (2, 3):
        for v, rc in ((0, SHAPE), (-1, SHAPE), (top + 1, UNSUP)):
            a = [one, none, 16, 16, one, one, big, none]
            a[k] = v
            assert L.pt_seg_state_f32(*a) == rc
    assert L.pt_seg_state_f32(one, none, 16, 16, one, one, need - 1, none) == WS
    # merge: scores, N, H, W, prob, labels, stats, ws, ws_bytes, stream
    assert L.pt_seg_merge_ws_bytes(3, 16, 16) == 3 * need
    assert L.pt_seg_merge_ws_bytes(0, 16, 16) == 0 and L.pt_seg_merge_ws_bytes(SR.MAX_OBJECTS + 1, 16, 16) == 0
    for k in (0, 4, 5, 6, 7):
        a = [one, 3, 16, 16, one, one, one, one, big, none]
        a[k] = none
        assert L.pt_seg_merge_f32(*a) == NULL
    for n, rc in ((0, SHAPE), (-2, SHAPE), (SR.MAX_OBJECTS + 1, UNSUP)):
        assert L.pt_seg_merge_f32(one, n, 16, 16, one, one, one, one, big, none) == rc
    for k in (2, 3):
        for v, rc in ((0, SHAPE), (top + 1, UNSUP)):
            a = [one, 3, 16, 16, one, one, one, one, big, none]
            a[k] = v
            assert L.pt_seg_merge_f32(*a) == rc
    assert L.pt_seg_merge_f32(one, 3, 16, 16, one, one, one, one, 3 * need - 1, none) == WS
    # mask patch: im, C, H, W, geom, out, OH, OW, stream
    g = (_lib.PatchGeom * 1)(_lib.PatchGeom(1, 0, 0, -2, -3, 30, 50))
    for k in (0, 4, 5):
        a = [one, 1, 37, 53, g, one, 24, 40, none]
        a[k] = none
        assert L.pt_sample_mask_patch_f32(*a) == NULL
    for k in (1, 2, 3, 6, 7):
        a = [one, 1, 37, 53, g, one, 24, 40, none]
        a[k] = 0
        assert L.pt_sample_mask_patch_f32(*a) == SHAPE
    for bad in (_lib.PatchGeom(0, 0, 0, 0, 0, 30, 50), _lib.PatchGeom(2, 2, 0, 0, 0, 30, 50), _lib.PatchGeom(1, 0, 0, 0, 0, 0, 50)):
        assert L.pt_sample_mask_patch_f32(one, 1, 37, 53, (_lib.PatchGeom * 1)(bad), one, 24, 40, none) == SHAPE
    assert L.pt_sample_mask_patch_f32(one, 1, 37, top + 1, g, one, 24, 40, none) == UNSUP


@pytest.mark.parametrize("name", SC.READOUT_CASES)
def test_readout_restatement_reproduces_golden(name):
    g = SC.golden("readout", name)
    crop, image, scale, pos, seed = SC.READOUT_CASES[name]
    assert tuple(g["crop"]) == crop and tuple(g["image"]) == image and float(g["scale"]) == scale and int(g["seed"]) == seed
    want = SC.readout_f64(SC.readout_input(name), image, scale, pos)
    sub = int(g["subsample"])
    st = want["stats"]
    got = OrderedDict(scores_im=want["scores_im"][::sub, ::sub], prob_sum=st["prob_sum"])
    for kind in ("lwl", "rts"):
        got[kind + "_pos"], got[kind + "_sz"] = SC.target_state_f64(st, kind)
    for k, v in got.items():
        err, b = float(np.abs(np.asarray(v) - g[k]).max()), f64_bound.bound(g["ref_fp32_err." + k])
        print(f"\nreadout_{name} {k}: |float64 restatement - golden| = {err:.3e}, bound {b:.3e}")
        assert err <= b, k
    assert int(g["near_zero"]) == 0                                     # no pixel of the reference sits on the zero crossing
    mask = want["scores_im"] > 0
    assert float(mask.sum()) == float(g["mask_count"]) == st["mask_count"] and np.array_equal(st["bbox"], g["bbox"])
    assert np.array_equal(mask[::sub, ::sub], g["scores_im"] > 0)
    outside = want["scores_im"] == SC.FILL
    assert np.array_equal(want["prob_im"][outside] < 1e-40, np.ones(int(outside.sum()), dtype=bool))


@pytest.mark.parametrize("name", SC.READOUT_CASES)
def test_host_placement_rule_reproduces_the_reference_window(name):
    g = SC.golden("readout", name)
    crop, image, scale, pos, _ = SC.READOUT_CASES[name]
    pl = SR.placement(crop, image, scale, pos)
    assert (pl.Hr, pl.Wr, pl.r1, pl.c1) == SC.placement(crop, image, scale, pos)
    # the window of the golden's score image: rows / columns that are not all -100
    full = SC.readout_f64(SC.readout_input(name), image, scale, pos)["scores_im"]
    sub = int(g["subsample"])
    rows, cols = np.nonzero((g["scores_im"] != SC.FILL).any(1))[0], np.nonzero((g["scores_im"] != SC.FILL).any(0))[0]
    wrows, wcols = np.nonzero((full[::sub, ::sub] != SC.FILL).any(1))[0], np.nonzero((full[::sub, ::sub] != SC.FILL).any(0))[0]
    assert np.array_equal(rows, wrows) and np.array_equal(cols, wcols)
    assert SR.intersects(pl, image)
    # RTS: its own sample location from the stored coordinates, then the same rule
    stub = type("S", (), {"img_sample_sz": torch.Tensor(list(crop))})()
    rpos, rscale = SR.sample_location(stub, torch.from_numpy(g["rts_coords"]))
    rpl = SR.placement(crop, image, rscale.item(), (rpos[0].item(), rpos[1].item()))
    assert [rpl.r1 + rpl.r1_pad, rpl.c1 + rpl.c1_pad, rpl.Hr, rpl.Wr] == [int(v) for v in g["rts_window"]]


def test_placement_truncates_towards_zero_where_floor_differs():
    crop, image, scale, pos, _ = SC.READOUT_CASES["topleft"]
    pl = SR.placement(crop, image, scale, pos)
    assert (pl.Hr, pl.Wr) == (6, 9)
    assert pos[0] - 0.5 * pl.Hr == pytest.approx(-1.8) and pos[1] - 0.5 * pl.Wr == pytest.approx(-2.2)
    assert (pl.r1, pl.c1) == (-1, -2) and (int(np.floor(-1.8)), int(np.floor(-2.2))) == (-2, -3)
    assert (pl.r1_pad, pl.c1_pad, pl.r2_pad, pl.c2_pad) == (1, 2, 0, 0)
    g = SC.golden("readout", "topleft")                                # the reference pasted rows 0..4 and columns 0..6: r2 = 5, c2 = 7
    inside = g["scores_im"] != SC.FILL
    assert np.nonzero(inside.any(1))[0].max() == pl.r1 + pl.Hr - 1 == 4 and np.nonzero(inside.any(0))[0].max() == pl.c1 + pl.Wr - 1 == 6
    crop, image, scale, pos, _ = SC.MISS
    assert not SR.intersects(SR.placement(crop, image, scale, pos), image)


@pytest.mark.parametrize("name", SC.MERGE_CASES)
def test_merge_restatement_reproduces_golden(name):
    g = SC.golden("merge", name)
    N, (H, W), seed = SC.MERGE_CASES[name]
    scores, entries = SC.merge_input(name)
    assert scores.shape == (N, H, W) and scores.dtype == np.float32 and (scores == SC.FILL).any()
    assert N == 1 or set(np.unique(scores[0])) == {-100.0, 100.0}      # the GT-mask convention
    want = SC.merge_f64(scores)
    err, b = float(np.abs(want["prob"][1:] - g["prob"]).max()), f64_bound.bound(g["ref_fp32_err.prob"])
    print(f"\nmerge_{name}: |float64 restatement - golden| = {err:.3e}, bound {b:.3e} (ref_fp32_err {float(g['ref_fp32_err.prob']):.2e})")
    assert err <= b and float(g["ref_fp32_err.prob"]) <= 2e-7 and not np.isnan(want["prob"]).any()
    assert np.abs(want["prob"].sum(0) - 1).max() <= 1e-6               # the aggregation is a distribution over background + objects
    ids = np.array([0] + SC.merge_ids(N), dtype=np.uint8)
    assert int(g["near_tie"]) == 0 and np.array_equal(ids[want["labels"]], g["segmentation"])
    for i, st in enumerate(want["stats"]):
        p, s = SC.target_state_f64(st, "lwl")
        box = np.array([p[1] - (s[1] - 1) / 2, p[0] - (s[0] - 1) / 2, s[1], s[0]])
        assert np.abs(box - g["lwl_boxes"][i]).max() <= f64_bound.bound(g["ref_fp32_err.lwl_boxes"])
        x0, y0, x1, y1 = st["bbox"]
        assert np.array_equal(np.array([x0, y0, x1 - x0 + 1, y1 - y0 + 1]), g["rts_boxes"][i])
    # the reference's fp32 boxes are within a few ulp of their largest coordinate of float64
    assert float(g["ref_fp32_err.lwl_boxes"]) <= 4 * f64_bound.ULP * float(np.abs(g["lwl_boxes"]).max())


@pytest.mark.parametrize("name", SC.PATCH_CASES)
def test_fp32_nearest_indices_equal_the_golden_patches(name):
    g = SC.golden("patch", name)
    geom, coord = SC.patch_geometry(name)
    osz = SC.PATCH_CASES[name][3]
    got = SC.mask_patch(SC.patch_input(name), geom, osz)
    assert got.dtype == np.float32 and np.array_equal(got, g["patch"])
    assert np.array_equal(np.asarray(coord, dtype=np.float32), g["coord"].reshape(-1))
    if name in ("df2", "df2_odd", "p30_22"):                            # the float64 formula picks another source pixel there
        assert not np.array_equal(SC.mask_patch(SC.patch_input(name), geom, osz, index=SC.nearest_index_f64), g["patch"])
    if name == "same":
        assert (geom.crop_h, geom.crop_w) == osz


def test_fp32_index_rule_on_the_known_size_pairs():
    pairs = {(26, 22), (30, 22), (30, 26)}
    for n_in, n_out in pairs:
        want = torch.nn.functional.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), (1, n_out), mode="nearest")
        assert np.array_equal(SC.nearest_index(n_in, n_out), want.view(-1).numpy().astype(np.int64))
        assert not np.array_equal(SC.nearest_index_f64(n_in, n_out), SC.nearest_index(n_in, n_out))
    crops = {(SC.patch_geometry(n)[0].crop_h, SC.PATCH_CASES[n][3][0]) for n in SC.PATCH_CASES if SC.PATCH_CASES[n][3]}
    crops |= {(SC.patch_geometry(n)[0].crop_w, SC.PATCH_CASES[n][3][1]) for n in SC.PATCH_CASES if SC.PATCH_CASES[n][3]}
    assert pairs <= crops                                               # the cases carry them on the crop-to-output axes
    assert {SC.patch_geometry(n)[0].df for n in SC.PATCH_CASES} == {1, 2}


def test_target_state_carries_the_host_side_decisions():
    pos, sz = torch.Tensor([3.0, 4.0]), torch.Tensor([5.0, 6.0])
    st = torch.zeros(SR.STATS)
    st[:5] = torch.tensor([50.0, 7.0, 9.0, 4.0, 9.0])
    st[5:10] = torch.tensor([60.0, 8.0, 10.0, 16.0, 25.0])
    p, s = SR.target_state(st, "lwl", pos, sz)
    assert p.tolist() == [7.0, 9.0] and s.tolist() == [8.0, 12.0]
    p, s = SR.target_state(st, "rts", pos, sz, sz_factor=2)
    assert p.tolist() == [8.0, 10.0] and s.tolist() == [8.0, 10.0]      # the moments of max(p, 0)
    assert SR.target_state(st, "lwl", pos, sz, min_mask_area=51) == (pos, sz)          # lwl.py:280
    assert SR.target_state(st, "rts", pos, sz, min_mask_area=51)[0].tolist() == [8.0, 10.0]
    flat = st.clone()
    flat[8] = 0.0
    assert SR.target_state(flat, "rts", pos, sz) == (pos, sz)           # rts.py:424
    flat[8] = float("nan")
    assert SR.target_state(flat, "rts", pos, sz) == (pos, sz)
    with pytest.raises(Exception, match="seg_to_bb_mode"):
        SR.target_state(st, "lwl", pos, sz, seg_to_bb_mode="box")
    st[11:15] = torch.tensor([2.0, 3.0, 6.0, 4.0])
    assert SR.mask_bbox(st, "t") == [2.0, 3.0, 5.0, 2.0] and SR.mask_bbox(st, "v") == [2.0, 3.0, 6.0, 4.0]
    assert SR.mask_bbox(torch.zeros(SR.STATS), "t") == [0.0, 0.0, 1.0, 1.0]            # masks_to_bboxes on an empty mask


def test_cpu_tensors_are_not_served():
    with pytest.raises(RuntimeError, match="MI355X"):
        SR.crop_to_image(torch.zeros(1, 1, 5, 7), (9, 11), 1.37, (1.2, 2.3))
    with pytest.raises(RuntimeError, match="MI355X"):
        SR.merge(torch.zeros(2, 5, 7))
    with pytest.raises(RuntimeError, match="MI355X"):
        SR.sample_mask_patch(torch.zeros(1, 1, 37, 53), (18.0, 26.0), (30.0, 50.0), (24, 40))
    assert not SR.convert_covered(torch.zeros(1, 1, 5, 7), torch.zeros(1, 3, 9, 11), 1.37, (1.2, 2.3))


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip, as tests/test_install_ledger.py does; uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install(seg_readout=True)
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


def _owners():
    from pytracking.tracker.lwl.lwl import LWL
    from pytracking.tracker.rts.rts import RTS
    from pytracking.tracker.rts.sta_helper import STAHelper
    return ((LWL, "convert_scores_crop_to_image"), (LWL, "merge_results"), (RTS, "convert_seg_scores_crop_to_image"), (RTS, "merge_results"),
            (STAHelper, "convert_scores_crop_to_image"))


@needs_reference
def test_install_switch_rebinds_exactly_the_five_symbols_and_uninstall_restores(amd):
    import test_install_ledger as TL
    owners = _owners()
    refs = [c.__dict__[a] for c, a in owners]
    before = TL.snapshot()
    amd.install()                                                       # default: off
    assert [c.__dict__[a] for c, a in owners] == refs
    with open(TL.REBOUND) as fh:
        pinned = json.load(fh)
    base = TL.changed(before, TL.snapshot())
    assert set(base) <= set(pinned) and set(pinned) - set(base) <= {"sys.modules[spatial_correlation_sampler]"}
    amd.uninstall()
    amd.install(seg_readout=True)
    assert TL.changed(before, TL.snapshot()) == sorted(base + NAMES)
    for (c, a), ref in zip(owners, refs):
        assert getattr(c, a).__wrapped__ is ref and amd.original(c, a) is ref
    amd.uninstall()
    assert [c.__dict__[a] for c, a in owners] == refs and TL.changed(before, TL.snapshot()) == []


class _Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def get(self, name, default=None):
        return self.__dict__.get(name, default)


def tracker_stub(cls, img_sample_sz=(480.0, 832.0), device="cpu"):
    """What the rebound methods read from a tracker: params, pos, target_sz, img_sample_sz and the class's own methods."""
    self = cls.__new__(cls)
    self.params = _Params(seg_to_bb_mode="var", seg_to_bb_sz_factor=SC.SZ_FACTOR, min_mask_area=-10, device=device)
    self.pos, self.target_sz = torch.Tensor([3.0, 4.0]), torch.Tensor([5.0, 6.0])
    self.img_sample_sz = torch.Tensor(list(img_sample_sz))
    return self


@needs_reference
def test_cpu_tensors_take_the_reference_branch(amd):
    (LWL, _), _, (RTS, _), _, (STA, _) = _owners()
    name = "bottomright"
    g = SC.golden("readout", name)
    crop, image, scale, pos, _ = SC.READOUT_CASES[name]
    scores, im = torch.from_numpy(SC.readout_input(name))[None, None], torch.empty(1, 3, *image)
    s_t, p_t = torch.tensor(scale, dtype=torch.float32), torch.tensor(pos, dtype=torch.float64)
    amd.install(seg_readout=True)
    amd.stats.clear()
    for cls in (LWL, STA):
        out = cls.convert_scores_crop_to_image(tracker_stub(cls), scores, im, s_t, p_t)
        assert not out.is_cuda and np.abs(out.numpy() - g["scores_im"]).max() <= 1e-5
        key = cls.__name__ + ".convert_scores_crop_to_image"
        assert amd.stats[key + ".reference"] == 1 and amd.stats[key + ".fast"] == 0
    out = RTS.convert_seg_scores_crop_to_image(tracker_stub(RTS, crop), scores, im, torch.from_numpy(g["rts_coords"]))
    assert len(out) == 5 and [int(v) for v in out[1:]] == [int(v) for v in g["rts_window"]]
    assert amd.stats["RTS.convert_seg_scores_crop_to_image.reference"] == 1
    mscores, entries = SC.merge_input("n3")
    gm = SC.golden("merge", "n3")
    out_all = OrderedDict((i, dict(e, target_bbox=[0.0, 0.0, 1.0, 1.0], time=0.0)) for i, e in zip(SC.merge_ids(3), entries))
    for cls in (LWL, RTS):                                              # a tracker on the CPU: the reference's own merge
        merged = cls.merge_results(tracker_stub(cls), out_all)
        assert np.array_equal(merged["segmentation"], gm["segmentation"]) and list(merged.keys()) == list(gm["keys"])
        assert amd.stats[cls.__name__ + ".merge_results.reference"] == 1 and amd.stats[cls.__name__ + ".merge_results.fast"] == 0
    amd.uninstall()
    amd.install(strict=True, seg_readout=True)
    with pytest.raises(NotImplementedError, match="convert_scores_crop_to_image"):
        LWL.convert_scores_crop_to_image(tracker_stub(LWL), scores, im, s_t, p_t)
