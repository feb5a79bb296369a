"""The TaMOs per-frame multi-object read-out on the MI355X (csrc_mot/mot_readout.hip through the C ABI of include/pt_mot.h and through
pytracking_amd.tamos_readout) against the float64 run of the numpy restatement (tests/tamos_readout_np.py) on the whole case table
(tests/tamos_readout_cases.py): no case and no object is excluded -- tests/test_tamos_readout_cpu.py asserts that every discrete decision
keeps a margin fp32 rounding cannot cross.

Bounds.  Discrete outputs (flag, chosen peak, both peaks' cells, whether the second peak was searched) equal the float64 restatement's.
Every float output -- the (T, H, W) map, both peak values, the raw and the clipped box, the ltrb targets, the label -- lies within
FACTOR x max(ref_err, 2^-23 max|want|) of float64: the bound of tests/f64_bound.py with its ulp_of_max floor, ref_err being the
restatement's own fp32 distance from float64 on that output of that case.  The four ltrb values read at the chosen cell are compared
exactly.  Figures are printed before they are asserted and, when TAMOS_READOUT_F64_OUT names a file, written there as a table
(profiles/tamos_readout_f64.txt is the table of such a run)."""
import ctypes

import numpy as np
import pytest
import torch

import f64_bound
import tamos_readout_cases as C
import tamos_readout_np as RN
from f64_bound import dev, needs_bundle
from pytracking_amd import _lib_mot as M
from pytracking_amd import tamos_readout as TR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# worst ratio of a device output to max(ref_err, ulp of max) measured on the MI355X (profiles/tamos_readout_f64.txt)
WORST_MEASURED = 1.00
FACTOR = f64_bound.raised_factor(WORST_MEASURED, C.F_MAX)
TABLE = f64_bound.Table("TAMOS_READOUT_F64_OUT",
                        "TaMOs per-frame multi-object read-out and training targets on the MI355X against float64 (tests/test_gpu_tamos_readout.py):\n"
                        "per output max |out - float64| and its ratio to max(ref_err, 2^-23 max|want|) -- the numpy restatement's own fp32 distance\n"
                        f"from float64 on that output, floored at one fp32 ulp of its range; bound = {FACTOR} x that.")
R = M


def anchor(name):
    return f64_bound.anchor(("tamos_readout", name), lambda dt: f64_bound.OrderedDict((k, C.run(C.CASES[name], dt)[k]) for k in RN.FLOAT_OUTPUTS))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(case, scores, ltrb, rec, map_out=None, seq=1.0):
    n = len(case["active"])
    act = (ctypes.c_int * n)(*case["active"])
    objs = (M.MotObject * n)(*[C.object_block(case["objects"][t]) for t in case["active"]])
    fr = C.frame_block(case["frame"])
    rc = M.lib().pt_mot_readout_f32(scores.data_ptr(), scores.shape[-2], scores.shape[-1], ltrb.data_ptr(), case["H"], case["W"], case["T"], act, n,
                                    objs, ctypes.byref(fr), None if map_out is None else map_out.data_ptr(), rec.data_ptr() if hasattr(rec, "data_ptr") else rec,
                                    seq, stream())
    assert rc == 0, M.lib().pt_mot_strerror(rc)
    return act


def record_fields(rec, active):
    r = rec[active].astype(np.float64)
    cell = lambda k: r[:, k:k + 2].astype(np.int64)
    return dict(flag=r[:, R.PT_MOT_R_FLAG].astype(np.int64), pick=r[:, R.PT_MOT_R_PICK].astype(np.int64), cell=cell(R.PT_MOT_R_ROW),
                peak1=cell(R.PT_MOT_R_ROW1), peak2=cell(R.PT_MOT_R_ROW2), second=r[:, R.PT_MOT_R_SECOND].astype(np.int64),
                max1=r[:, R.PT_MOT_R_MAX1], max2=r[:, R.PT_MOT_R_MAX2], presence=r[:, R.PT_MOT_R_PRESENCE],
                raw_box=r[:, R.PT_MOT_R_RAW_BOX:R.PT_MOT_R_RAW_BOX + 4], box=r[:, R.PT_MOT_R_BOX:R.PT_MOT_R_BOX + 4],
                ltrb=r[:, R.PT_MOT_R_LTRB:R.PT_MOT_R_LTRB + 4], obj=r[:, R.PT_MOT_R_OBJECT].astype(np.int64))


def hold(tag, got, want, ref_errs, table=TABLE):
    for q, w in want.items():
        f64_bound.held(tag, {q: float(np.abs(np.asarray(got[q], np.float64).reshape(w.shape) - w).max())}, None, ref_errs[q], factor=FACTOR,
                       floor=f64_bound.ulp_of_max(w), table=table)


@pytest.mark.parametrize("name", C.CASES)
def test_readout_through_the_c_abi(name):
    case, a, w = C.CASES[name], anchor(name), C.run(C.CASES[name])
    scores, ltrb = dev(case["scores"]), dev(case["ltrb"])
    T, H, Wd = case["T"], case["H"], case["W"]
    rec = torch.full((T, M.PT_MOT_REC_FLOATS), -7.0, device=DEV)
    maps = torch.full((T, H, Wd), -7.0, device=DEV)
    launch(case, scores, ltrb, rec, maps, seq=5.0)
    torch.cuda.synchronize()
    host = rec.cpu().numpy()
    got = record_fields(host, case["active"])
    got["map"] = maps.cpu().numpy()[case["active"]]
    for k in RN.DISCRETE_OUTPUTS:
        assert np.array_equal(got[k], w[k]), (name, k, got[k].tolist(), w[k].tolist())
    assert got["obj"].tolist() == case["active"] and np.array_equal(got["presence"], got["max1"])
    assert (host[case["active"], R.PT_MOT_R_SEQ] == 5.0).all()
    idle = [t for t in range(T) if t not in case["active"]]
    assert (host[idle] == -7.0).all() and (maps.cpu().numpy()[idle] == -7.0).all()          # inactive objects: nothing written
    assert np.array_equal(got["ltrb"], w["ltrb"])                                        # fp32 inputs read, not computed
    hold("readout_" + name, got, a.want, a.ref_errs)
    # the same call again, and with the record in pinned host memory behind the polled wait: the same bits
    rec2 = torch.zeros_like(rec)
    launch(case, scores, ltrb, rec2, None, seq=5.0)
    pinned = torch.zeros(T, M.PT_MOT_REC_FLOATS).pin_memory()
    act = launch(case, scores, ltrb, pinned, None, seq=5.0)
    assert M.lib().pt_mot_wait_f32(pinned.data_ptr(), act, len(case["active"]), 5.0, stream()) == 0
    landed = pinned.numpy()[case["active"]].copy()                                        # readable without a stream synchronisation
    torch.cuda.synchronize()
    assert np.array_equal(rec2.cpu().numpy()[case["active"]], host[case["active"]]) and np.array_equal(landed, host[case["active"]])


def test_targets_through_the_c_abi():
    lab = C.LABEL
    for nf in (1, 2):
        b = C.target_boxes(nf)
        want = RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE)
        ref = float(np.abs(RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE, np.float32) - want).max())
        got = TR.encode_boxes(dev(b), C.IMAGE_SAMPLE_SIZE, C.STRIDE)
        assert got.shape == want.shape
        hold(f"targets_nf{nf}", {"ltrb": got.cpu().numpy()}, {"ltrb": want}, {"ltrb": ref})
        assert (got[:, 1] == 0).all() and (got[-1, -1] == 0).all()
        assert torch.equal(TR.encode_boxes(dev(b), C.IMAGE_SAMPLE_SIZE, C.STRIDE), got)
    want = RN.label(C.LABEL_CENTRES, lab["feature_sz"], lab["sigma"], lab["end_pad"])
    ref = float(np.abs(RN.label(C.LABEL_CENTRES, lab["feature_sz"], lab["sigma"], lab["end_pad"], np.float32) - want).max())
    got = TR.gaussian_labels(C.LABEL_CENTRES.tolist(), lab["feature_sz"], lab["sigma"], lab["end_pad"], torch.device(DEV))
    assert got.shape == want.shape
    hold("targets", {"label": got.cpu().numpy()}, {"label": want}, {"label": ref})
    # both parts in one launch: the same bits
    b = dev(C.target_boxes(2).reshape(-1, 4))
    ltrb = torch.empty(b.shape[0], 4, 12, 18, device=DEV)
    both = torch.empty_like(got)
    lb = TR.label_block(lab["feature_sz"], lab["sigma"], lab["end_pad"])
    cen = (ctypes.c_float * 8)(*C.LABEL_CENTRES.reshape(-1).tolist())
    assert M.lib().pt_mot_targets_f32(b.data_ptr(), b.shape[0], 96, 144, C.STRIDE, ltrb.data_ptr(), ctypes.byref(lb), cen, 4, both.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(both, got) and torch.equal(ltrb.reshape(2, -1, 4, 12, 18), TR.encode_boxes(dev(C.target_boxes(2)), C.IMAGE_SAMPLE_SIZE, C.STRIDE))


def test_graph_replay_equals_the_eager_call():
    case = C.CASES["up6x9_wide"]
    scores, ltrb = dev(case["scores"]), dev(case["ltrb"])
    boxes = dev(C.target_boxes(2))
    eager_rec = torch.zeros(case["T"], M.PT_MOT_REC_FLOATS, device=DEV)
    eager_map = torch.zeros(case["T"], case["H"], case["W"], device=DEV)
    launch(case, scores, ltrb, eager_rec, eager_map, seq=3.0)
    eager_ltrb = TR.encode_boxes(boxes, C.IMAGE_SAMPLE_SIZE, C.STRIDE)
    torch.cuda.synchronize()
    rec, mp = torch.zeros_like(eager_rec), torch.zeros_like(eager_map)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(case, scores, ltrb, rec, mp, seq=3.0)                               # warm-up: kernels loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    rec.zero_(), mp.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(case, scores, ltrb, rec, mp, seq=3.0)
        g_ltrb = TR.encode_boxes(boxes, C.IMAGE_SAMPLE_SIZE, C.STRIDE)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rec, eager_rec) and torch.equal(mp, eager_map) and torch.equal(g_ltrb, eager_ltrb)


# ---- through the host mirror, on the unmodified class -------------------------------------------------------------------------------------------
def _tracker(case, device=DEV):
    import tamos_tracker as TT
    return TT.bare_tracker(case["frame"], {t + 1: s for t, s in case["objects"].items()}, (case["H"] * C.STRIDE, case["W"] * C.STRIDE), device=device)


@needs_bundle
@pytest.mark.parametrize("name", ("up6x9_wide", "asis12x18_clip"))
def test_mot_readout_run_reads_the_tracker_as_the_reference_does(name):
    case, g = C.CASES[name], C.golden(name)
    trk = _tracker(case)
    coords = torch.Tensor([list(case["frame"]["sample_coords"])])
    res = TR.MotReadout(trk).run(dev(case["scores"])[None, None], dev(case["ltrb"])[None, None], coords, (case["frame"]["image_h"], case["frame"]["image_w"]))
    assert list(res) == [t + 1 for t in case["active"]]
    for i, r in enumerate(res.values()):
        assert r.flag == RN.FLAGS[int(g["flag"][i])] and r.score_loc.int().tolist() == g["cell"][i].tolist()
        assert not r.score_loc.is_cuda and r.score_loc.dtype == torch.float32 and r.bbox.shape == (4,)
        tol = 2 * FACTOR * f64_bound.ULP * max(1.0, float(np.abs(g["raw_box"][i]).max()))
        assert np.abs(r.bbox_raw.numpy() - g["raw_box"][i]).max() <= tol and np.abs(r.bbox.numpy() - g["box"][i]).max() <= tol


@pytest.fixture()
def amd():
    from oracle import ref_harness
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(tamos=True, tamos_readout=True)
    amd.stats.clear()
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
def test_drop_ins_keep_the_reference_contract(amd):
    import tamos_tracker as TT
    from pytracking import TensorList
    from pytracking.tracker.tamos.tamos import TaMOs
    name = "up6x9_wide"
    case, g = C.CASES[name], C.golden(name)
    trk = _tracker(case)
    trk.net = TT.CaseNet(torch.from_numpy(case["scores"]), torch.from_numpy(case["ltrb"]), DEV)
    mem = torch.from_numpy(C.target_boxes(2, T=16))
    TT.give_memory(trk, mem, (6, 9), DEV)
    trk.params.feature_stride = 16
    fast = lambda k: amd.stats["TaMOs." + k + ".fast"]
    fell = lambda k: amd.stats["TaMOs." + k + ".reference"]
    scores_raw, bbox_preds = trk.classify_target({"layer3": torch.zeros(1, 4, 6, 9, device=DEV)})
    assert fast("classify_target") == 1 and fast("encode_bbox") == 2 and fell("encode_bbox") == 0       # one launch per memory frame (tamos.py:299)
    want_ltrb = RN.encode_bbox(mem.numpy(), (96, 144), 16)
    assert trk.net.calls[0]["train_ltrb"].shape == want_ltrb.shape
    assert np.abs(trk.net.calls[0]["train_ltrb"].cpu().numpy() - want_ltrb).max() <= FACTOR * f64_bound.ULP * float(np.abs(want_ltrb).max())
    assert scores_raw.shape == (1, 1, 16, 12, 18) and bbox_preds.shape == (1, 1, 16, 4, 12, 18)          # the reference's own upsample
    scores_raw = torch.sigmoid(scores_raw)                                                  # tamos.py:173-174
    coords = torch.Tensor([list(case["frame"]["sample_coords"])])
    for i, oid in enumerate(trk.object_ids):
        scale_ind, s, flag, loc = trk.localize_target(scores_raw[:, :, oid - 1], trk.scale_factor, oid)
        box = trk.direct_bbox_regression(bbox_preds[:, :, oid - 1], coords, loc, scores_raw[:, :, oid - 1], stride=8)
        assert int(scale_ind) == 0 and s.shape == (1, 12, 18) and s.is_cuda and torch.equal(s, scores_raw[:, :, oid - 1].squeeze(1))
        assert flag == RN.FLAGS[int(g["flag"][i])] and loc.int().tolist() == g["cell"][i].tolist() and not loc.is_cuda and loc.dtype == torch.float32
        assert isinstance(box, torch.Tensor) and not box.is_cuda and box.dtype == torch.float32 and box.shape == (4,)
        assert np.abs(box.numpy() - g["raw_box"][i]).max() <= 2 * FACTOR * f64_bound.ULP * max(1.0, float(np.abs(g["raw_box"][i]).max()))
        assert s[0, int(loc[0]), int(loc[1])].item() == pytest.approx(float(g["map"][i][tuple(g["cell"][i])]), abs=1e-5)
    n = len(trk.object_ids)
    assert fast("localize_target") == n and fast("direct_bbox_regression") == n and fell("localize_target") == 0 and fell("direct_bbox_regression") == 0
    # what the stash does not cover is the reference's call: another frame, a tensor that is not the queued one
    trk.frame_num += 1
    oid = trk.object_ids[3]
    _, _, flag, loc = trk.localize_target(scores_raw[:, :, oid - 1], trk.scale_factor, oid)
    assert fell("localize_target") == 1 and flag == RN.FLAGS[int(g["flag"][3])] and loc.int().tolist() == g["cell"][3].tolist()
    trk.frame_num -= 1
    trk.localize_target(scores_raw[:, :, oid - 1], trk.scale_factor, oid)
    box = trk.direct_bbox_regression(bbox_preds[:, :, oid - 1].clone(), coords, loc, scores_raw[:, :, oid - 1], stride=8)   # not the queued tensor
    assert fell("direct_bbox_regression") == 1 and fast("localize_target") == n + 1
    assert np.abs(box.numpy() - g["raw_box"][3]).max() <= 2 * FACTOR * f64_bound.ULP * max(1.0, float(np.abs(g["raw_box"][3]).max()))
    # the label: a TensorList of one (1, 1, H3, W3) device tensor
    trk.feature_sz, trk.sigma = torch.Tensor(list(C.LABEL["feature_sz"])), torch.Tensor(list(C.LABEL["sigma"]))
    gt = C.golden("targets")
    y = trk.get_label_function(torch.from_numpy(gt["pos"].copy()), trk.scale_factor)
    assert isinstance(y, TensorList) and len(y) == 1 and y[0].is_cuda and y[0].shape == (1, 1, 12, 18) and fast("get_label_function") == 1
    assert np.abs(y[0].cpu().numpy()[0, 0] - gt["label_from_pos"]).max() <= 2 * FACTOR * f64_bound.ULP
    # uninstall restores the reference's own functions
    ref = amd.original(TaMOs, "localize_target")
    amd.uninstall()
    assert vars(TaMOs)["localize_target"] is ref
