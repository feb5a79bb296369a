"""Segmentation read-out, object merge and mask patch on the MI355X (seg_readout.hip through pytracking_amd.seg_readout) against the goldens
of the unmodified reference (tools/make_golden_seg_readout.py) and the float64 restatements of tests/seg_readout_cases.py.

Bounds.  Every fp32 output is held to FACTOR x max(ref_fp32_err, 2^-23 max|want|) of float64 -- the bound of tests/f64_bound.py with its ulp_of_max floor;
ref_fp32_err is the reference's own fp32 distance from float64 on that output, the floor is one fp32 ulp of the output's range -- and to the
project's 1e-4 of the golden, absolute (1e-4 of the magnitude only where FACTOR fp32 ulp of the quantity already exceed 1e-4: prob_sum
above 200, the moments of the 720 x 1280 image -- see golden_tol).  Masks,
boxes and label maps are compared exactly wherever the float64 decision has a margin of 1e-5; at most 0.5 % of the pixels may be excluded
(the reference itself excludes none on these inputs).  Mask patches are compared exactly.  The measured ratios are printed and, when
SEG_READOUT_F64_OUT names a file, written there as a table (profiles/seg_readout_f64.txt is the table of such a run).

Every test prints its measured figures before it asserts (run with -s)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import f64_bound
import seg_readout_cases as SC
from f64_bound import dev, needs_bundle
from oracle import ref_harness
from pytracking_amd import seg_readout as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
MARGIN, EXCLUDED_MAX = 1e-5, 0.005
TABLE = f64_bound.Table("SEG_READOUT_F64_OUT",
                        "Segmentation read-out, object merge and their statistics on the MI355X against float64 (tests/test_gpu_seg_readout.py):\n"
                        "per output max |out - float64| and its ratio to max(ref_fp32_err, 2^-23 max|want|) -- the reference's own fp32\n"
                        f"distance from float64 on that output, floored at one fp32 ulp of its range; bound = {f64_bound.FACTOR} x that.")
_WANT = {}


def hold_rows(tag, rows, table=TABLE):
    """rows: [(output, error, want, ref_err)], each output held to its own ref_err and the ulp of its own range."""
    for q, e, w, r in rows:
        f64_bound.held(tag, {q: float(e)}, None, r, floor=f64_bound.ulp_of_max(w), table=table)


def golden_tol(golden):
    """The project's absolute 1e-4 against a golden; for a quantity so large that FACTOR fp32 ulp of it exceed 1e-4 (prob_sum and the
    moments of the 720 x 1280 image: both sides are fp32 numbers, each a few ulp from float64) 1e-4 of its magnitude instead."""
    top = float(np.abs(golden).max())
    return ATOL if f64_bound.FACTOR * f64_bound.ULP * top <= ATOL else ATOL * top


def readout_want(name):
    if ("readout", name) not in _WANT:
        crop, image, scale, pos, _ = SC.READOUT_CASES[name] if name != "miss" else SC.MISS
        _WANT[("readout", name)] = SC.readout_f64(SC.readout_input(name), image, scale, pos)
    return _WANT[("readout", name)]


def merge_want(name):
    if ("merge", name) not in _WANT:
        _WANT[("merge", name)] = SC.merge_f64(SC.merge_input(name)[0])
    return _WANT[("merge", name)]


def run_readout(name, outputs=SR.OUTPUTS):
    crop, image, scale, pos, _ = SC.READOUT_CASES[name] if name != "miss" else SC.MISS
    return SR.crop_to_image(dev(SC.readout_input(name))[None, None], image, scale, pos, outputs=outputs)


def _stat_rows(got, want, ref):
    """Statistics of a device block against a float64 dict: [(name, error, want, ref_err)] for the moments as the trackers read them."""
    rows = []
    for key in ("prob_sum", "e_y", "e_x"):
        rows.append((key, abs(got[key] - want[key]), want[key], ref.get(key, 0.0)))
    for key in ("var_y", "var_x"):                                      # held as the size the reference returns: sqrt(var) * factor
        g, w = SC.SZ_FACTOR * np.sqrt(got[key]), SC.SZ_FACTOR * np.sqrt(want[key])
        rows.append(("sz" + key[3:], abs(g - w), w, ref.get("sz", 0.0)))
    return rows


@pytest.mark.parametrize("name", SC.READOUT_CASES)
def test_readout_against_float64_and_golden(name):
    g, want = SC.golden("readout", name), readout_want(name)
    out = run_readout(name)
    torch.cuda.synchronize()
    host = out.to_host()
    sub = int(g["subsample"])
    scores, prob, mask = host.scores_im.numpy(), host.prob_im.numpy(), host.mask_im.numpy()
    st = SC.stats_dict(host.stats.numpy())
    ref = {"prob_sum": float(g["ref_fp32_err.prob_sum"]), "e_y": float(g["ref_fp32_err.lwl_pos"]), "e_x": float(g["ref_fp32_err.lwl_pos"]),
           "sz": float(g["ref_fp32_err.lwl_sz"])}
    rows = [("scores_im", float(np.abs(scores - want["scores_im"]).max()), want["scores_im"], float(g["ref_fp32_err.scores_im"])),
            ("prob_im", float(np.abs(prob - want["prob_im"]).max()), want["prob_im"], float(g["ref_fp32_err.scores_im"]) / 4)]   # sigmoid' <= 1/4
    hold_rows("readout_" + name, rows + _stat_rows(st, want["stats"], ref))
    # the golden, within the project's 1e-4 (golden_tol: relative only where fp32 cannot resolve 1e-4)
    assert np.abs(scores[::sub, ::sub] - g["scores_im"]).max() <= ATOL
    gprob = 1.0 / (1.0 + np.exp(-g["scores_im"].astype(np.float64)))   # the reference's next line: sigmoid of its score image
    perr = float(np.abs(prob[::sub, ::sub] - gprob).max())
    print(f"readout_{name}: max |prob_im - sigmoid(golden scores_im)| = {perr:.3e}")
    assert perr <= ATOL
    lp, ls = SR.target_state(host.stats, "lwl", sz_factor=SC.SZ_FACTOR)
    rp, rs = SR.target_state(host.stats, "rts", sz_factor=SC.SZ_FACTOR)
    for got, key in ((lp, "lwl_pos"), (ls, "lwl_sz"), (rp, "rts_pos"), (rs, "rts_sz")):
        err = float(np.abs(got.numpy() - g[key]).max())
        print(f"readout_{name}: max |{key} - golden| = {err:.3e} (tolerance {golden_tol(g[key]):.1e})")
        assert err <= golden_tol(g[key]), key
    print(f"readout_{name}: |prob_sum - golden| = {abs(st['prob_sum'] - float(g['prob_sum'])):.3e} (tolerance {golden_tol(g['prob_sum']):.1e})")
    assert abs(st["prob_sum"] - float(g["prob_sum"])) <= golden_tol(g["prob_sum"])
    for k in ("prob_sum", "e_y", "e_x", "var_y", "var_x"):              # sigmoid >= 0: the clamped moments are the plain ones
        assert st[k + "_c"] == st[k]
    # mask and box: exact on the kernel's own scores, and the reference's wherever the float64 score is clear of zero
    assert np.array_equal(mask, (scores > 0).astype(np.float32)) and st["mask_count"] == float(mask.sum())
    clear = np.abs(want["scores_im"]) >= MARGIN
    excluded = 1.0 - float(clear.mean())
    print(f"readout_{name}: excluded share {excluded:.5f}, mask {int(st['mask_count'])} px, box {st['bbox'].tolist()}")
    assert excluded <= EXCLUDED_MAX
    assert np.array_equal(mask[clear], want["mask_im"][clear].astype(np.float32))
    assert np.array_equal((mask[::sub, ::sub] > 0)[clear[::sub, ::sub]], (g["scores_im"] > 0)[clear[::sub, ::sub]])
    assert clear[want["scores_im"] > 0].all() or excluded == 0.0        # no box decided by an excluded pixel
    assert np.array_equal(st["bbox"], g["bbox"]) and st["mask_count"] == float(g["mask_count"])
    outside = want["scores_im"] == SC.FILL
    assert (scores[outside] == SC.FILL).all() and (prob[outside] == 0).all()
    # two runs are bit-equal
    again = run_readout(name)
    assert again.equal(out)


def test_readout_window_that_misses_the_image():
    out = run_readout("miss").to_host()
    st = SC.stats_dict(out.stats.numpy())
    assert (out.scores_im == SC.FILL).all() and (out.prob_im == 0).all() and (out.mask_im == 0).all()
    assert st["mask_count"] == 0 and st["prob_sum"] == 0 and st["bbox"].tolist() == [0, 0, 0, 0]


def test_readout_optional_outputs_and_input_views():
    name = "ragged_b"
    full = run_readout(name)
    only = run_readout(name, outputs=("prob",))
    assert only.scores_im is None and only.mask_im is None and torch.equal(only.prob_im, full.prob_im) and torch.equal(only.stats, full.stats)
    none = run_readout(name, outputs=())
    assert torch.equal(none.stats, full.stats)
    crop, image, scale, pos, _ = SC.READOUT_CASES[name]
    s = dev(SC.readout_input(name))
    padded = torch.zeros(crop[0] + 3, crop[1] + 5, device=DEV)
    padded[1:crop[0] + 1, 2:crop[1] + 2] = s
    view = padded[1:crop[0] + 1, 2:crop[1] + 2]                         # a non-contiguous view of the same values
    assert not view.is_contiguous()
    for x in (view, s[None, None], s):
        assert SR.crop_to_image(x, image, scale, pos).equal(full)


@pytest.mark.parametrize("name", SC.READOUT_CASES)
def test_state_repeats_the_readout_statistics_bit_for_bit(name):
    out = run_readout(name)
    st = SR.state(out.prob_im, out.mask_im)
    assert torch.equal(st, out.stats)
    assert torch.equal(SR.state(out.prob_im[None, None], out.mask_im[None, None]), out.stats)
    # without a mask image the mask is prob > 0.5: the same pixels unless a score rounds to sigmoid = 0.5
    free = SC.stats_dict(SR.state(out.prob_im).cpu().numpy())
    assert free["mask_count"] == float((out.prob_im > 0.5).sum()) and free["prob_sum"] == float(out.stats[0])


def test_state_of_a_signed_image_separates_the_clamped_moments():
    img = (SC.blob_scores(4401, 45, 70) / 6.0).astype(np.float32)      # values in about [-0.6, 0.6]
    want = SC.state_f64(img, img > 0.5)
    got = SC.stats_dict(SR.state(dev(img)).cpu().numpy())
    for k in SC.STAT_KEYS[:10]:                                         # blocked fp32 sums of 3150 terms of magnitude <= 0.6: well inside 2e-5 relative
        assert abs(got[k] - want[k]) <= 2e-5 * max(1.0, abs(want[k])), (k, got[k], want[k])
    assert got["prob_sum_c"] > got["prob_sum"]
    assert got["mask_count"] == want["mask_count"] and np.array_equal(got["bbox"], want["bbox"])


@pytest.mark.parametrize("name", SC.MERGE_CASES)
def test_merge_against_float64_and_golden(name):
    g, want = SC.golden("merge", name), merge_want(name)
    N, (H, W), _ = SC.MERGE_CASES[name]
    scores = dev(SC.merge_input(name)[0])
    out = SR.merge(scores)
    host = out.to_host()
    prob, labels = host.prob.numpy(), host.labels.numpy()
    assert prob.shape == (N + 1, H, W) and labels.shape == (H, W) and labels.dtype == np.uint8 and host.stats.shape == (N, SR.STATS)
    assert not np.isnan(prob).any() and not np.isnan(host.stats.numpy()[:, :1]).any()
    ref = float(g["ref_fp32_err.prob"])
    hold_rows("merge_" + name, [("prob", float(np.abs(prob - want["prob"]).max()), want["prob"], ref)])
    box_ref = float(g["ref_fp32_err.lwl_boxes"])
    for i in range(N):
        st, w = SC.stats_dict(host.stats[i].numpy()), want["stats"][i]
        srows = _stat_rows(st, w, {"prob_sum": box_ref, "e_y": box_ref, "e_x": box_ref, "sz": box_ref})
        hold_rows("merge_" + name, [(f"{q}[{i}]", e, v, r) for q, e, v, r in srows], table=TABLE if N <= 3 else None)   # the table keeps the small cases' rows
    assert np.abs(prob[1:] - g["prob"]).max() <= ATOL
    # 0 and 1 where the reference has them
    assert np.array_equal(prob[1:] == 0, g["prob"] == 0) and np.array_equal(prob[1:] == 1, g["prob"] == 1)
    # label map: the reference's wherever the two largest float64 probabilities are 1e-5 apart
    clear = want["gap"] >= MARGIN
    excluded = 1.0 - float(clear.mean())
    ids = np.array([0] + SC.merge_ids(N), dtype=np.uint8)
    print(f"merge_{name}: excluded share {excluded:.5f}")
    assert excluded <= EXCLUDED_MAX and np.array_equal(ids[labels][clear], g["segmentation"][clear])
    assert np.array_equal(labels[clear], want["labels"][clear])
    for i in range(N):
        st = host.stats[i]
        assert float(st[SR.MASK_COUNT]) == float((labels == i + 1).sum())
        if excluded == 0.0:
            assert SR.mask_bbox(st, "t") == g["rts_boxes"][i].tolist()
        p, s = SR.target_state(st, "lwl", torch.Tensor([3.0, 4.0]), torch.Tensor([5.0, 6.0]), sz_factor=SC.SZ_FACTOR)
        box = torch.cat((p[[1, 0]] - (s[[1, 0]] - 1) / 2, s[[1, 0]])).numpy()
        assert np.abs(box - g["lwl_boxes"][i]).max() <= golden_tol(g["lwl_boxes"][i])
    assert SR.merge(scores).equal(out)                 # two runs are bit-equal
    assert SR.merge(scores[:, None]).equal(out)        # (N, 1, H, W)


def test_merge_extreme_scores_end_in_zero_and_one():
    s = torch.tensor([[100.0, -100.0, 100.0, -100.0, 0.0, 88.0, -88.0, 50.0],
                      [-100.0, -100.0, 100.0, 3.0, 0.0, -88.0, 88.0, -50.0]], device=DEV).view(2, 1, 8)
    m = SR.merge(s).to_host()
    want = SC.merge_f64(s.cpu().numpy())
    p = m.prob.numpy()
    print("\nmerge extremes:\n", p.reshape(3, 8))
    assert not np.isnan(p).any() and np.abs(p - want["prob"]).max() <= 4 * f64_bound.ULP
    assert p[1, 0, 0] == 1.0 and p[2, 0, 0] == 0.0 and p[0, 0, 0] == 0.0                 # +100 against -100
    assert p[0, 0, 1] == 1.0 and p[1, 0, 1] == 0.0 and p[2, 0, 1] == 0.0                 # both at -100: background
    assert p[1, 0, 2] == 0.5 and p[2, 0, 2] == 0.5 and m.labels[0, 2] == 1               # a tie: the first maximum wins
    assert m.labels[0].tolist()[:4] == [1, 0, 1, 2]


@pytest.mark.parametrize("name", SC.PATCH_CASES)
def test_mask_patch_equals_golden(name):
    g = SC.golden("patch", name)
    _, pos, ssz, osz, mode, _ = SC.PATCH_CASES[name]
    im = dev(SC.patch_input(name))[None, None]
    patch, coord = SR.sample_mask_patch(im, torch.Tensor(list(pos)), torch.Tensor(list(ssz)), None if osz is None else torch.Tensor(list(osz)),
                                        mode=mode)
    assert patch.shape == (1, 1) + g["patch"].shape and np.array_equal(patch[0, 0].cpu().numpy(), g["patch"])
    assert np.array_equal(coord.numpy(), g["coord"])
    two = torch.cat([im, 1 - im], 1)                                    # channels; an odd output width takes the scalar stores
    p2, _ = SR.sample_mask_patch(two, torch.Tensor(list(pos)), torch.Tensor(list(ssz)), None if osz is None else torch.Tensor(list(osz)),
                                 mode=mode)
    assert torch.equal(p2[:, 0], patch[:, 0])
    geom, _ = SC.patch_geometry(name)
    assert np.array_equal(p2[0, 1].cpu().numpy(), SC.mask_patch(1 - SC.patch_input(name), geom, osz))


def test_graph_capture_of_readout_then_merge_replays_the_eager_bits():
    name = "ragged_a"
    crop, image, scale, pos, _ = SC.READOUT_CASES[name]
    s = dev(SC.readout_input(name))
    other = dev(SC.blob_scores(4500, *image))

    def chain():
        r = SR.crop_to_image(s, image, scale, pos)
        return r, SR.merge(torch.stack([r.scores_im, other]))

    r0, m0 = chain()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                         # warm-up: kernels loaded before the capture (the workspace is per stream:
    torch.cuda.current_stream().wait_stream(side)                       # the capture stream takes its own from the graph's pool)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r1, m1 = chain()
    graph.replay()
    torch.cuda.synchronize()
    assert r1.equal(r0) and m1.equal(m0)


class _Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def get(self, name, default=None):
        return self.__dict__.get(name, default)


def _tracker(cls, img_sample_sz=(480.0, 832.0)):
    self = cls.__new__(cls)
    self.params = _Params(seg_to_bb_mode="var", seg_to_bb_sz_factor=SC.SZ_FACTOR, min_mask_area=-10, device=DEV)
    self.pos, self.target_sz = torch.Tensor([3.0, 4.0]), torch.Tensor([5.0, 6.0])
    self.img_sample_sz = torch.Tensor(list(img_sample_sz))
    return self


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(seg_readout=True, decoder=True)
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
def test_installed_methods_keep_the_reference_contract(amd):
    from pytracking.tracker.lwl.lwl import LWL
    from pytracking.tracker.rts.rts import RTS
    from pytracking.tracker.rts.sta_helper import STAHelper
    name = "bottomright"
    g = SC.golden("readout", name)
    crop, image, scale, pos, _ = SC.READOUT_CASES[name]
    cpu_scores = torch.from_numpy(SC.readout_input(name))[None, None]
    scores, im = cpu_scores.to(DEV), torch.empty(1, 3, *image)
    s_t, p_t = torch.tensor(scale, dtype=torch.float32), torch.tensor(pos, dtype=torch.float64)
    b = f64_bound.bound(g["ref_fp32_err.scores_im"], floor=f64_bound.ulp_of_max(g["scores_im"])) + 4 * float(g["ref_fp32_err.scores_im"])      # both sides against float64
    amd.stats.clear()
    for cls in (LWL, STAHelper):
        key = cls.__name__ + ".convert_scores_crop_to_image"
        got = cls.convert_scores_crop_to_image(_tracker(cls), scores, im, s_t, p_t)
        want = amd.original(cls, "convert_scores_crop_to_image")(_tracker(cls), cpu_scores, im, s_t, p_t)
        assert amd.stats[key + ".fast"] == 1 and amd.stats[key + ".reference"] == 0, dict(amd.stats)
        assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == want.dtype and got.shape == want.shape
        err = float((got - want).abs().max())
        print(f"\n{key}: max |fused - original| = {err:.3e} (bound {b:.3e})")
        assert err <= b
    coords = torch.from_numpy(g["rts_coords"])
    got = RTS.convert_seg_scores_crop_to_image(_tracker(RTS, crop), scores, im, coords)
    want = amd.original(RTS, "convert_seg_scores_crop_to_image")(_tracker(RTS, crop), cpu_scores, im, coords)
    assert amd.stats["RTS.convert_seg_scores_crop_to_image.fast"] == 1
    assert len(got) == 5 and not got[0].is_cuda and [type(v) for v in got[1:]] == [type(v) for v in want[1:]] and got[1:] == want[1:]
    assert float((got[0] - want[0]).abs().max()) <= b
    # a window that misses the image is the reference's call (it raises)
    miss = torch.tensor(SC.MISS[3], dtype=torch.float64)
    with pytest.raises(Exception):
        LWL.convert_scores_crop_to_image(_tracker(LWL), scores, im, s_t, miss)
    assert amd.stats["LWL.convert_scores_crop_to_image.reference"] == 1
    for mname in ("n3", "n6"):
        gm = SC.golden("merge", mname)
        N = int(gm["N"])
        _, entries = SC.merge_input(mname)
        out_all = OrderedDict((i, dict(e, target_bbox=[0.0, 0.0, 1.0, 1.0], time=0.0)) for i, e in zip(SC.merge_ids(N), entries))
        for cls in (LWL, RTS):
            key = cls.__name__ + ".merge_results"
            before = amd.stats[key + ".fast"]
            got = cls.merge_results(_tracker(cls), out_all)
            want = amd.original(cls, "merge_results")(_tracker(cls), out_all)
            assert amd.stats[key + ".fast"] == before + 1 and amd.stats[key + ".reference"] == 0
            assert type(got) is type(want) and list(got.keys()) == list(want.keys())
            assert got["segmentation"].dtype == want["segmentation"].dtype and np.array_equal(got["segmentation"], want["segmentation"])
            assert type(got["segmentation_raw"]) is type(want["segmentation_raw"]) and list(got["segmentation_raw"]) == list(want["segmentation_raw"])
            for i in got["segmentation_raw"]:
                a, w = got["segmentation_raw"][i], want["segmentation_raw"][i]
                assert isinstance(a, np.ndarray) and a.dtype == w.dtype and a.shape == w.shape
                assert np.abs(a - w).max() <= f64_bound.bound(gm["ref_fp32_err.prob"], floor=f64_bound.ulp_of_max(w)) + 4 * float(gm["ref_fp32_err.prob"])
            assert got["time"] == want["time"] and list(got["target_bbox"]) == list(want["target_bbox"])
            for i in got["target_bbox"]:
                a, w = got["target_bbox"][i], want["target_bbox"][i]
                assert isinstance(a, list) and len(a) == 4 and all(isinstance(v, float) for v in a)
                assert np.abs(np.array(a) - np.array(w)).max() <= golden_tol(np.array(w))
