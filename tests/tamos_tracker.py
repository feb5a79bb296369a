"""The unmodified reference TaMOs tracker (pytracking/tracker/tamos/tamos.py) for the tests of the per-frame multi-object read-out.

Two uses.  `bare_tracker(...)`: a `TaMOs` object made with `TaMOs.__new__` and the attributes the read-out methods read set by hand, for
calling the reference's own `localize_target` / `direct_bbox_regression` / `clip_bbox_to_image_area` / `encode_bbox` /
`get_label_function` on the case table (tools/make_golden_tamos_readout.py on the CPU, tests/test_gpu_tamos_readout.py on the device).

`run(...)`: the whole tracker closed loop -- `initialize()` and `track()` as the reference ships them -- on a stub `net` whose head methods
return seeded synthetic score / ltrb maps: three objects whose blobs move, two of them cross, one vanishes for a frame.  Every object's
score channel also carries the other objects' blobs, lower, so that the distractor and hard-negative branches are reached.  The calls across
the read-out boundary are recorded event by event; the CPU run without install() is tests/golden/tracker_tamos.npz
(tools/make_golden_tamos_readout.py tracker)."""
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import tracker_harness as TH  # noqa: E402
import tracker_replay as TR  # noqa: E402

# every method install(tamos_readout=True) rebinds, as install.stats names them
EXPECT_FAST = ("TaMOs.classify_target", "TaMOs.localize_target", "TaMOs.direct_bbox_regression", "TaMOs.encode_bbox", "TaMOs.get_label_function")


def make_params(frame=None, device="cpu", **over):
    """The parameters the read-out methods read (pytracking/parameter/tamos/*.py names); `frame`: a frame dict of tamos_readout_cases"""
    TH.ref_harness.install()
    from pytracking.utils import TrackerParams
    p = TrackerParams()
    fr = frame or {}
    for k in ("target_not_found_threshold", "distractor_threshold", "hard_negative_threshold", "target_neighborhood_scale", "dispalcement_scale"):
        setattr(p, k, fr.get(k, dict(target_not_found_threshold=0.25, distractor_threshold=0.8, hard_negative_threshold=0.5,
                                     target_neighborhood_scale=2.2, dispalcement_scale=0.8)[k]))
    for k in ("uncertain_threshold", "hard_sample_threshold"):
        if math.isfinite(fr.get(k, -math.inf)):
            setattr(p, k, fr[k])
    p.advanced_localization = True
    p.normalize_scores = bool(fr.get("normalize_scores", 1))
    p.score_preprocess = "none"
    p.window_output = False
    for k, v in over.items():
        setattr(p, k, v)
    return TH.use_device(p, device)


def bare_tracker(frame, objects, image_sample_size, feature_stride=16, device="cpu", label=None):
    """objects: {object id (1-based): state dict of fp32 pos / pos_prev / target_sz}"""
    TH.ref_harness.install()
    from pytracking.tracker.tamos.tamos import TaMOs
    t = TaMOs.__new__(TaMOs)
    t.params = make_params(frame, device, image_sample_size=tuple(int(v) for v in image_sample_size), feature_stride=feature_stride)
    t.object_ids = list(objects)
    f32 = lambda v: torch.from_numpy(np.asarray(v, np.float32).copy())
    t.pos = OrderedDict((o, f32(s["pos"])) for o, s in objects.items())
    t.pos_prev = OrderedDict((o, f32(s["pos_prev"])) for o, s in objects.items())
    t.target_sz = OrderedDict((o, f32(s["target_sz"])) for o, s in objects.items())
    t.img_sample_sz = torch.Tensor(list(frame["img_sample_sz"]))
    t.img_support_sz = t.img_sample_sz
    t.train_img_sample_sz = torch.Tensor(list(frame["train_img_sample_sz"]))
    t.kernel_size = torch.Tensor(list(frame["kernel_size"]))
    t.scale_factor = frame["scale_factor"]
    t.image_sz = torch.Tensor([frame["image_h"], frame["image_w"]])
    t.frame_num = 1
    if label is not None:
        t.feature_sz = torch.Tensor(list(label["feature_sz"]))
        t.sigma = torch.Tensor(list(label["sigma"]))
    return t


class CaseNet:
    """A `net` for classify_target (tamos.py:289-322) on a bare tracker: the head returns one case's maps.  give_memory() sets the memory
    attributes the method reads."""

    def __init__(self, scores, ltrb, device):
        self.scores, self.ltrb = scores.to(device)[None, None], ltrb.to(device)[None, None]
        self.head = self
        self.calls = []

    def extract_head_feat(self, x):
        return x

    def get_filter_and_features_in_parallel(self, train_feat, test_feat, num_gth_frames, train_label, train_ltrb_target, train_bb):
        self.calls.append(dict(train_label=train_label, train_ltrb=train_ltrb_target, train_bb=train_bb))
        return None, None, None, None

    def fpn(self, enc, x):
        return {"feat2": None}

    def classifier(self, feat, weights):
        return self.scores.clone()

    def bb_regressor(self, feat, weights):
        return self.ltrb.clone()


def give_memory(tracker, boxes, feature_hw, device):
    """boxes (nf, T, 4): the stored target boxes of nf memory frames"""
    from pytracking import TensorList
    nf, T = boxes.shape[:2]
    tracker.num_stored_samples = [nf]
    tracker.training_samples = TensorList([torch.zeros(nf, 4, *feature_hw, device=device)])
    tracker.target_labels = TensorList([torch.zeros(nf, T, *feature_hw, device=device)])
    tracker.target_boxes = boxes.to(device)


# ---- closed loop ---------------------------------------------------------------------------------------------------------------------------
RUN = dict(seed=7300, n_frames=8)
HS, WS, H, W, TOKENS = 6, 9, 12, 18, 4                  # raw 6 x 9 (feature stride 16), decision map 12 x 18 (stride 8), 4 object tokens
SAMPLE = (96, 144)
IMAGE_HW = (240, 360)                                   # scale_factor 0.4: 20 image pixels per decision cell
INIT = OrderedDict([("1", (3.0, 2.0)), ("2", (3.0, 15.0)), ("3", (9.0, 9.0))])     # decision cells [row, col] of the three objects in frame 1
BOX = 48.0                                              # side of every object's box in image pixels


def _centre(oid, k):
    """where object `oid` is in frame k (k = 0: the first frame): 1 and 2 run towards each other along one row and cross, 3 stands"""
    r, c = INIT[str(oid)]
    return (r, c + 1.5 * k) if oid == 1 else (r, c - 1.5 * k) if oid == 2 else (r, c)


def frame_maps(seed, k):
    """(scores (1, 1, TOKENS, HS, WS), ltrb (1, 1, TOKENS, 4, H, W)) of frame k.  Object 3 vanishes in frame 5."""
    rng = np.random.default_rng(seed + 31 * k)
    scores = -3.0 + rng.uniform(0, 0.02, (TOKENS, HS, WS))
    rr, cc = np.mgrid[0:HS, 0:WS]
    for t in range(3):
        for other in range(3):
            gone = k == 5 and 2 in (t, other)                                    # object 3 is gone: not in the other channels, and its own channel
            if gone and other != t:                                              # keeps a faint blob (below target_not_found_threshold) so that the
                continue                                                         # peak is a blob and not a cell of the noise
            r, c = _centre(other + 1, k)
            r, c = (r + 0.5) * HS / H - 0.5, (c + 0.5) * WS / W - 0.5
            # object 1's channel barely sees the others (normal), object 2's sees them almost as high as itself (distractor tests), object 3's
            # in between (hard negative)
            height = (1.2 if gone else 5.0) if other == t else (2.0, 4.6, 3.6)[t]
            scores[t] += height * np.exp(-((rr - r) ** 2 + (cc - c) ** 2) / (2 * 0.7 ** 2))
    ltrb = np.empty((TOKENS, 4, H, W))
    half = BOX * 0.4 / 2                                                         # half a box in sample pixels
    ltrb[:, 0::2] = half / SAMPLE[1] + rng.uniform(0, 0.01, (TOKENS, 2, H, W))
    ltrb[:, 1::2] = half / SAMPLE[0] + rng.uniform(0, 0.01, (TOKENS, 2, H, W))
    return torch.from_numpy(scores.astype(np.float32))[None, None], torch.from_numpy(ltrb.astype(np.float32))[None, None]


class _Head:
    """The five calls classify_target makes on `net.head` (tamos.py:296-317); the maps of the frame come from frame_maps"""

    def __init__(self, owner):
        self.owner = owner
        self.filter_predictor = type("FilterPredictor", (), {"num_tokens": TOKENS})()

    def extract_head_feat(self, x):
        return x

    def get_filter_and_features_in_parallel(self, train_feat, test_feat, num_gth_frames, train_label, train_ltrb_target, train_bb):
        self.owner.rec.add("targets", train_label=train_label, train_ltrb=train_ltrb_target, n_bb=np.array([len(d) for d in train_bb]))
        return None, None, None, None

    def fpn(self, enc, x):
        return {"feat2": None}

    def classifier(self, feat, weights):
        s, self._ltrb = frame_maps(self.owner.seed, self.owner.k)
        self.owner.k += 1
        return s.to(self.owner.device)

    def bb_regressor(self, feat, weights):
        return self._ltrb.to(self.owner.device)


class StubNet:
    def __init__(self, seed, device, rec):
        self.seed, self.device, self.rec, self.k = seed, torch.device(device), rec, 1
        self.net = self
        self.head = _Head(self)

    def initialize(self):
        pass

    def extract_backbone(self, im):
        g = torch.Generator().manual_seed(self.seed + self.k)
        return {"layer3": torch.randn(1, 8, HS, WS, generator=g).to(self.device)}

    def get_backbone_head_feat(self, feat):
        return feat


def run(seed, n_frames, device="cpu", tamos_params=None):
    """initialize() + n_frames x track(); returns (Recorder, tracker)."""
    TH.ref_harness.install()
    from pytracking.tracker.tamos.tamos import TaMOs
    rec = TH.Recorder()
    net = StubNet(seed, device, rec)
    prm = make_params(None, device, image_sample_size=SAMPLE, feature_stride=16, train_feature_size=(HS, WS), search_area_scale=4.0,
                      sample_memory_size=4, learning_rate=0.1, hard_negative_learning_rate=0.2, update_classifier=True, net=net,
                      conf_ths=0.5, **(tamos_params or {}))
    tracker = TaMOs(prm)
    tracker.visdom = None
    rec.add("config", seed=seed, n_frames=n_frames)

    orig_loc, orig_box, orig_mem = tracker.localize_target, tracker.direct_bbox_regression, tracker.update_memory
    last = {}

    def localize(scores, scale_factor, obj_id):
        scale_ind, s, flag, loc = orig_loc(scores, scale_factor, obj_id)
        last.update(oid=obj_id, flag=flag, loc=loc)
        assert s.shape == scores.squeeze(1).shape and int(scale_ind) == 0
        return scale_ind, s, flag, loc

    def regress(bbox_preds, sample_coords, score_loc, scores_raw, stride=16):
        b = orig_box(bbox_preds, sample_coords, score_loc, scores_raw, stride=stride)
        rec.add("object", oid=last["oid"], flag=last["flag"], score_loc=last["loc"].int(), bbox=b)
        return b

    def update_memory(sample_x, ys, boxes, learning_rate=None):
        orig_mem(sample_x, ys, boxes, learning_rate)
        slot = int(tracker.previous_replace_ind[0])
        rec.add("memory", slot=slot, stored=int(tracker.num_stored_samples[0]), label=tracker.target_labels[0][slot], target_boxes=tracker.target_boxes[slot],
                sample_weights=tracker.sample_weights[0])
    tracker.localize_target, tracker.direct_bbox_regression, tracker.update_memory = localize, regress, update_memory

    rng = np.random.default_rng(seed + 77)
    half = (BOX - 1) / 2
    boxes = OrderedDict((oid, [c * 20.0 - half, r * 20.0 - half, BOX, BOX]) for oid, (r, c) in INIT.items())
    tracker.initialize(TH.synthetic_frame(rng, IMAGE_HW), {"init_object_ids": list(INIT), "object_ids": list(INIT), "init_bbox": boxes})
    for _ in range(n_frames):
        rec.add("frame", frame=tracker.frame_num + 1)
        out = tracker.track(TH.synthetic_frame(rng, IMAGE_HW))
        rec.add("state", target_bbox=np.array([out["target_bbox"][o] for o in INIT], dtype=np.float64),
                presence=np.array([out["object_presence_score"][o] for o in INIT], dtype=np.float64))
    return rec, tracker


def events(rec):
    return TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()})


def run_installed(device="cuda"):
    """The same run on the device through install(tamos=True, tamos_readout=True); returns (events, install.stats)."""
    TH.ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(tamos=True, tamos_readout=True)
    amd.stats.clear()
    try:
        rec, _ = run(device=device, **RUN)
        stats = dict(amd.stats)
    finally:
        amd.uninstall()
    return events(rec), stats
