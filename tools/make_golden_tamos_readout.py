"""TEST INFRASTRUCTURE ONLY -- goldens of the TaMOs per-frame multi-object read-out from the UNMODIFIED reference on the CPU (needs the
reference tree):
    python -B tools/make_golden_tamos_readout.py            tests/golden/tamos_readout_<case>.npz, tamos_readout_targets.npz
    python -B tools/make_golden_tamos_readout.py tracker    tests/golden/tracker_tamos.npz
  tamos_readout_<case>   For every case of tests/tamos_readout_cases.CASES a bare `TaMOs` object (tests/tamos_tracker.bare_tracker: TaMOs.__new__,
                         attributes set by hand) and the reference's own methods on it, per active object as track() calls them
                         (pytracking/tracker/tamos/tamos.py:181-185): localize_target, direct_bbox_regression, clip_bbox_to_image_area.  The two
                         lines of classify_target / track that form the map (tamos.py:319-320, 173-174) are torch calls, made here as written
                         there: F.interpolate(scores[0], size, mode='bicubic').unsqueeze(0) when both sizes differ, torch.sigmoid.
  tamos_readout_targets  encode_bbox on every memory frame of tamos_readout_cases.target_boxes(nf), nf = 1 and 2, and get_label_function /
                         dcf.label_function_spatial for the label centres of the table.
  tracker_tamos          the closed loop of tests/tamos_tracker.run on the CPU without install().
Inputs are regenerated from the seeds of the case table by the tests; nothing of the numpy restatement is read here."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import tamos_readout_cases as C  # noqa: E402
import tamos_tracker as TT  # noqa: E402

OUT = os.environ.get("TAMOS_READOUT_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))


def case_golden(case):
    fr = case["frame"]
    trk = TT.bare_tracker(fr, {t + 1: s for t, s in case["objects"].items()}, (case["H"] * C.STRIDE, case["W"] * C.STRIDE))
    target_scores = torch.from_numpy(case["scores"].copy())[None, None]                     # (1, 1, T, Hs, Ws)
    bbox_preds = torch.from_numpy(case["ltrb"].copy())[None, None]                           # (1, 1, T, 4, H, W)
    if target_scores.shape[-1] != bbox_preds.shape[-1] and target_scores.shape[-2] != bbox_preds.shape[-2]:
        target_scores = F.interpolate(target_scores[0], bbox_preds.shape[-2:], mode='bicubic').unsqueeze(0)
    scores_raw = torch.sigmoid(target_scores) if trk.params.get('normalize_scores', False) else target_scores
    sample_coords = torch.Tensor([list(fr["sample_coords"])])
    image = np.zeros((fr["image_h"], fr["image_w"], 3), np.uint8)
    rows = dict(map=[], flag=[], cell=[], raw_box=[], box=[], max1=[])
    for oid in trk.object_ids:
        scale_ind, s, flag, score_loc = trk.localize_target(scores_raw[:, :, oid - 1], trk.scale_factor, oid)
        bbox_raw = trk.direct_bbox_regression(bbox_preds[:, :, oid - 1], sample_coords, score_loc, scores_raw[:, :, oid - 1], stride=fr["stride"])
        bbox = trk.clip_bbox_to_image_area(bbox_raw, image)
        assert int(scale_ind) == 0
        rows["map"].append(s[0].numpy())
        rows["flag"].append(C.RN.FLAGS.index(flag))
        rows["cell"].append(score_loc.int().numpy())
        rows["raw_box"].append(bbox_raw.numpy())
        rows["box"].append(bbox.numpy())
        rows["max1"].append(float(s[0].max()))
    return {k: np.stack([np.asarray(v) for v in vs]) for k, vs in rows.items()}


def targets_golden():
    out = {}
    fr = C.CASES["up6x9_wide"]["frame"]
    trk = TT.bare_tracker(fr, {1: C.CASES["up6x9_wide"]["objects"][0]}, C.IMAGE_SAMPLE_SIZE, feature_stride=C.STRIDE, label=C.LABEL)
    for nf in (1, 2):
        boxes = torch.from_numpy(C.target_boxes(nf))
        out[f"ltrb_nf{nf}"] = torch.cat([trk.encode_bbox(b).unsqueeze(0) for b in boxes], dim=0).numpy()         # tamos.py:299
    from pytracking import dcf
    ksz_even = torch.Tensor([(trk.kernel_size[0] + 1) % 2, (trk.kernel_size[1] + 1) % 2])
    out["label"] = np.concatenate([dcf.label_function_spatial(trk.feature_sz, trk.sigma, torch.from_numpy(c.copy()), end_pad=ksz_even).numpy()[0]
                                   for c in C.LABEL_CENTRES])
    # get_label_function itself, from a position: the centre it forms and its label
    pos = torch.Tensor([130.0, 77.0])
    out["pos"] = pos.numpy()
    out["label_from_pos"] = trk.get_label_function(pos, trk.scale_factor)[0].numpy()[0, 0]
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:] == ["tracker"]:
        rec, _ = TT.run(device="cpu", **TT.RUN)
        np.savez_compressed(os.path.join(OUT, "tracker_tamos.npz"), **rec.to_npz_dict())
        print("tracker_tamos:", [e["kind"] for e in rec.events].count("object"), "object events,",
              [str(e["flag"]) for e in rec.events if e["kind"] == "object"])
        return
    for name, case in C.CASES.items():
        g = case_golden(case)
        np.savez_compressed(os.path.join(OUT, f"tamos_readout_{name}.npz"), **g)
        print(name, "flags", g["flag"].tolist(), "cells", g["cell"].tolist())
    np.savez_compressed(os.path.join(OUT, "tamos_readout_targets.npz"), **targets_golden())


if __name__ == "__main__":
    main()
