"""TEST INFRASTRUCTURE ONLY -- tests/golden/seg_readout_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_seg_readout.py
  seg_readout_readout_<case>  LWL.convert_scores_crop_to_image (pytracking/tracker/lwl/lwl.py:330-359) on tests/seg_readout_cases.blob_scores,
                              torch.sigmoid, both get_target_state bodies (lwl.py:276-300, rts.py:405-430) and masks_to_bboxes
                              (ltr/data/bounding_box_utils.py:33-67) on the result, and what RTS.convert_seg_scores_crop_to_image
                              (rts.py:460-493) returns for sample coordinates of the same window.  The 720 x 1280 case keeps every 4th row
                              and column of the score image.
  seg_readout_merge_<case>    LWL.merge_results and RTS.merge_results (lwl.py:210-274, rts.py:340-403) on seg_readout_cases.merge_input.
  seg_readout_patch_<case>    sample_patch(is_mask=True) (pytracking/features/preprocessing.py:54-148).
The methods run on a stub `self` carrying params, pos, target_sz and img_sample_sz.  Inputs are regenerated from the stored seeds by the
tests.  `ref_fp32_err.<output>` is the largest distance of the reference's fp32 run from the same operations in float64: the reference's
own code on float64 tensors where it keeps them float64 (the paste, sigmoid), and `state64` / `merge64` below -- the reference's lines
written out on float64 torch tensors -- where it rounds to fp32 itself (get_target_state ends in torch.Tensor([...]), merge_results
starts with .float()).  Neither reads tests/seg_readout_cases' numpy restatements, which the CPU tests hold against these figures."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import seg_readout_cases as SC  # noqa: E402

OUT = os.environ.get("SEG_READOUT_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def get(self, name, default=None):
        return self.__dict__.get(name, default)


def stub(cls, img_sample_sz=(480.0, 832.0)):
    """What the methods read from the tracker: params, pos, target_sz, img_sample_sz, and their own siblings."""
    members = {k: v for k, v in vars(cls).items() if k in ("get_target_state", "get_sample_location")}
    self = type("Stub", (), members)()
    self.params = Params(seg_to_bb_mode="var", seg_to_bb_sz_factor=SC.SZ_FACTOR, min_mask_area=-10)
    self.pos, self.target_sz = torch.Tensor([3.0, 4.0]), torch.Tensor([5.0, 6.0])
    self.img_sample_sz = torch.Tensor(list(img_sample_sz))
    return self


def save(tag, g):
    path = os.path.join(OUT, f"seg_readout_{tag}.npz")
    np.savez_compressed(path, **g)
    assert os.path.getsize(path) < 560 * 1024, (path, os.path.getsize(path))
    return os.path.getsize(path)


def dist(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def state64(prob, clamp):
    """get_target_state (lwl.py:285-298; rts.py:408-428 with the clamp) on a float64 image, without the final fp32 packing:
    (pos [e_y, e_x], size [sqrt(e_h), sqrt(e_w)] * factor) as float64 tensors."""
    p = prob.double().clamp(min=0) if clamp else prob.double()
    ay, ax = torch.arange(p.shape[-2], dtype=torch.float64), torch.arange(p.shape[-1], dtype=torch.float64)
    prob_sum = p.sum()
    e_y = torch.sum(p.sum(dim=-1) * ay) / prob_sum
    e_x = torch.sum(p.sum(dim=-2) * ax) / prob_sum
    e_h = torch.sum(p.sum(dim=-1) * (ay - e_y) ** 2) / prob_sum
    e_w = torch.sum(p.sum(dim=-2) * (ax - e_x) ** 2) / prob_sum
    return torch.stack([e_y, e_x]), torch.stack([e_h.sqrt() * SC.SZ_FACTOR, e_w.sqrt() * SC.SZ_FACTOR])


def merge64(scores):
    """lwl.py:229-243 on float64 tensors: the N + 1 aggregated probabilities, background first."""
    s = torch.from_numpy(scores).double()
    prob = torch.sigmoid(s)
    eps = 1e-7
    bg_p = torch.prod(1 - prob, dim=0).clamp(eps, 1.0 - eps)
    bg_score = (bg_p / (1.0 - bg_p)).log()
    allS = torch.cat((bg_score.unsqueeze(0), s), dim=0)
    return torch.stack([1.0 / (allS - a.unsqueeze(0)).exp().sum(dim=0) for a in allS], dim=0)


def readouts():
    from pytracking.tracker.lwl.lwl import LWL
    from pytracking.tracker.rts.rts import RTS
    from ltr.data.bounding_box_utils import masks_to_bboxes
    for name, ((Hc, Wc), (Hi, Wi), scale, pos, seed) in SC.READOUT_CASES.items():
        scores = torch.from_numpy(SC.readout_input(name))[None, None]
        im = torch.empty(1, 1, Hi, Wi)
        s_t, p_t = torch.tensor(scale, dtype=torch.float32), torch.tensor(pos, dtype=torch.float64)
        lwl, rts = stub(LWL), stub(RTS, (Hc, Wc))
        run = {}
        for tag, x in (("f32", scores), ("f64", scores.double())):
            sim = LWL.convert_scores_crop_to_image(lwl, x, im, s_t, p_t)
            prob = torch.sigmoid(sim)
            lp, ls = LWL.get_target_state(lwl, prob)
            rp, rs = RTS.get_target_state(rts, prob)
            if tag == "f64":                                             # the reference packs its result into fp32: evaluate its lines in float64
                (lp, ls), (rp, rs) = state64(prob, False), state64(prob, True)
            run[tag] = dict(scores_im=sim, prob_sum=prob.sum(), lwl_pos=lp, lwl_sz=ls, rts_pos=rp, rts_sz=rs)
        f32 = run["f32"]
        mask = (f32["scores_im"] > 0).float()
        bbox = masks_to_bboxes(mask[None], fmt="v").view(-1)
        # RTS: sample coordinates whose centre and scale are this window's (get_sample_location, rts.py:432-437)
        sz = torch.tensor([Hc, Wc], dtype=torch.float64) * scale
        c0 = torch.tensor(pos, dtype=torch.float64) - sz / 2 + 0.5
        coords = torch.cat([c0, c0 + sz]).float()
        rsim, rr1, rc1, rrows, rcols = RTS.convert_seg_scores_crop_to_image(rts, scores, im, coords)
        sub = SC.SUBSAMPLE.get(name, 1)
        g = dict(seed=seed, crop=np.array([Hc, Wc]), image=np.array([Hi, Wi]), scale=scale, pos=np.array(pos), subsample=sub,
                 scores_im=f32["scores_im"].numpy()[::sub, ::sub], prob_sum=float(f32["prob_sum"]), mask_count=float(mask.sum()),
                 bbox=bbox.numpy(), rts_coords=coords.numpy(), rts_window=np.array([rr1, rc1, rrows, rcols]),
                 rts_max_diff=dist(rsim, f32["scores_im"]))
        for k in ("lwl_pos", "lwl_sz", "rts_pos", "rts_sz"):
            g[k] = f32[k].numpy()
        for k in f32:
            g["ref_fp32_err." + k] = dist(f32[k], run["f64"][k])
        # the excluded share of the mask comparison: pixels whose float64 score is within 1e-5 of zero
        g["near_zero"] = int((run["f64"]["scores_im"].abs() < 1e-5).sum())
        size = save("readout_" + name, g)
        print(f"readout_{name}: image {Hi}x{Wi}  window {rr1},{rc1} {rrows}x{rcols}  mask {int(g['mask_count'])} px  near zero {g['near_zero']}  "
              + "  ".join(f"{k} {g['ref_fp32_err.' + k]:.2e}" for k in f32) + f"  rts diff {g['rts_max_diff']:.1e}  {size} B")
        assert g["near_zero"] == 0, name


def merges():
    from pytracking.tracker.lwl.lwl import LWL
    from pytracking.tracker.rts.rts import RTS
    for name, (N, (H, W), seed) in SC.MERGE_CASES.items():
        scores, entries = SC.merge_input(name)
        ids = SC.merge_ids(N)
        out_all = OrderedDict((i, dict(e, target_bbox=[0.0, 0.0, 1.0, 1.0], time=0.0)) for i, e in zip(ids, entries))
        lw = LWL.merge_results(stub(LWL), out_all)
        rt = RTS.merge_results(stub(RTS), out_all)
        prob = np.stack([lw["segmentation_raw"][i] for i in ids])
        assert prob.dtype == np.float32 and lw["segmentation"].dtype == np.uint8
        assert np.array_equal(prob, np.stack([rt["segmentation_raw"][i] for i in ids])) and np.array_equal(lw["segmentation"], rt["segmentation"])
        want = merge64(scores)
        lwl_boxes = np.array([lw["target_bbox"][i] for i in ids], dtype=np.float64)
        box64 = []
        for k in range(N):
            p, sz = state64(want[k + 1], False)
            box64.append(torch.cat((p[[1, 0]] - (sz[[1, 0]] - 1) / 2, sz[[1, 0]])).tolist())
        srt = torch.sort(want, dim=0).values
        gap = (srt[-1] - srt[-2]).numpy()
        g = dict(seed=seed, N=N, H=H, W=W, ids=np.array(ids), prob=prob, segmentation=lw["segmentation"], lwl_boxes=lwl_boxes,
                 rts_boxes=np.array([rt["target_bbox"][i] for i in ids], dtype=np.float64), keys=np.array(list(lw.keys())),
                 near_tie=int((gap < 1e-5).sum()))
        g["ref_fp32_err.prob"] = float(np.abs(prob - want[1:].numpy()).max())
        g["ref_fp32_err.lwl_boxes"] = float(np.abs(lwl_boxes - np.array(box64)).max())
        size = save("merge_" + name, g)
        print(f"merge_{name}: N {N} {H}x{W}  ref_fp32_err prob {g['ref_fp32_err.prob']:.2e} boxes {g['ref_fp32_err.lwl_boxes']:.2e}  near ties "
              f"{g['near_tie']}  nan {int(np.isnan(prob).sum())}  zeros {float((prob == 0).mean()):.2f}  ones {float((prob == 1).mean()):.2f}  {size} B")
        assert g["near_tie"] == 0 and not np.isnan(prob).any(), name


def patches():
    from pytracking.features.preprocessing import sample_patch
    for name, ((H, W), pos, ssz, osz, mode, seed) in SC.PATCH_CASES.items():
        im = torch.from_numpy(SC.patch_input(name))[None, None]
        patch, coord = sample_patch(im, torch.Tensor(list(pos)), torch.Tensor(list(ssz)), None if osz is None else torch.Tensor(list(osz)),
                                    mode=mode, is_mask=True)
        g = dict(seed=seed, image=np.array([H, W]), pos=np.array(pos), sample_sz=np.array(ssz), output_sz=np.array(osz if osz else [0, 0]),
                 mode=mode, patch=patch[0, 0].numpy(), coord=coord.numpy())
        size = save("patch_" + name, g)
        print(f"patch_{name}: {H}x{W} -> {tuple(patch.shape[-2:])}  zeros {float((patch == 0).float().mean()):.2f}  {size} B")


if __name__ == "__main__":
    readouts()
    merges()
    patches()
