"""The case table of the TaMOs per-frame multi-object read-out (tests/test_tamos_readout_cpu.py, tests/test_gpu_tamos_readout.py,
tools/make_golden_tamos_readout.py): seeded synthetic score / ltrb maps and tracker states at the smallest shapes at which each step can go
wrong.  A case is built from a specification in score cells -- where each object's blobs sit and how high, where the object was, how
large its neighbourhood is -- so that the intended statement of `localize_advanced` (tamos.py:386-429) is reached with a margin; the CPU
test asserts statement and margin, nothing here is tuned on device output.

    maps      5x7 as it is; 6x9 -> 12x18 bicubic with either aspect branch of extract_backbone_features (tamos.py:438-447); 12x18 as it is;
              one 24x36 -> 48x72 (the deployed sizes)
    objects   T = 1, 2, 4, 16 (nine active with gaps in the ids)
    peaks     in a corner, on each border, a tie between two cells, a neighbourhood bound that lands exactly on .5
    flags     every one of the nine return statements
    clipping  each of the four sides and the minimum width / height
    targets   empty boxes, nf = 1 and 2 memory frames; a label centre off the map

numpy only at import (frame_block / object_block load the ctypes bindings when called); reads tests/golden/ and nothing outside the
repository."""
import math
import os
from collections import OrderedDict

import numpy as np

import tamos_readout_np as RN

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDE = 8
DEFAULT_THRESHOLDS = dict(target_not_found_threshold=0.25, uncertain_threshold=-math.inf, hard_sample_threshold=-math.inf,
                          distractor_threshold=0.8, hard_negative_threshold=0.5, target_neighborhood_scale=2.2, dispalcement_scale=0.8)


def _frame(H, W, image_hw, normalize, train_feature=None, **over):
    """The host values of one frame as TaMOs.initialize / extract_backbone_features form them (tamos.py:81-86, 432-454)."""
    sample = (float(H * STRIDE), float(W * STRIDE))                              # params.image_sample_size
    h, w = float(image_hw[0]), float(image_hw[1])
    if h / w <= sample[0] / sample[1]:
        sf = sample[1] / w                                                       # scale such that the width matches
    else:
        sf = sample[0] / h
    tf = train_feature or (H // 2 + 1, W // 2 - 1)                               # train_feature_size x feature_stride 16: not the sample size, not square
    fr = dict(DEFAULT_THRESHOLDS, scale_factor=sf, img_support_sz=sample, img_sample_sz=sample,
              train_img_sample_sz=(float(tf[0] * 16), float(tf[1] * 16)), kernel_size=(1.0, 1.0),
              sample_coords=(0.0, 0.0, float(F32(sample[0]) / F32(sf)), float(F32(sample[1]) / F32(sf))),
              image_h=int(image_hw[0]), image_w=int(image_hw[1]), stride=STRIDE, min_width=10, min_height=10,
              normalize_scores=int(normalize), score_preprocess=0, score_filter_ksz=1, window_output=0, advanced_localization=1)
    fr.update(over)
    return fr


def _ratio(fr, H, W):
    out_sz = np.array([H, W], F32)
    return (np.asarray(fr["img_support_sz"], F32) / out_sz) / F32(fr["scale_factor"])


def _state(fr, H, W, center, prev_vec=(0.0, 0.0), neigh=(3.3, 3.3)):
    """pos / pos_prev / target_sz (image pixels, fp32) of an object that sits at `center` (score cells), moved by prev_vec since the last
    frame and has the neighbourhood `neigh` (score cells)"""
    r = _ratio(fr, H, W)
    pos = np.asarray(center, F32) * r
    return dict(pos=pos, pos_prev=pos - np.asarray(prev_vec, F32) * r, target_sz=np.asarray(neigh, F32) * r / F32(fr["target_neighborhood_scale"]))


def _scores(seed, Hs, Ws, H, W, blobs, base, noise=0.02, width=0.7):
    """base + seeded noise + one Gaussian blob per (row, col, height above base); (row, col) in cells of the (H, W) decision map: the blob
    sits at the raw position that F.interpolate samples for that cell, so the upsampled map peaks in exactly one cell"""
    rng = np.random.default_rng(seed)
    m = base + rng.uniform(0, noise, (Hs, Ws))
    rr, cc = np.mgrid[0:Hs, 0:Ws]
    for r, c, a in blobs:
        r, c = (r + 0.5) * Hs / H - 0.5, (c + 0.5) * Ws / W - 0.5
        m = m + a * np.exp(-((rr - r) ** 2 + (cc - c) ** 2) / (2 * width ** 2))
    return m.astype(F32)


def _ltrb(seed, T, H, W):
    return np.random.default_rng(seed).uniform(0.05, 0.3, (T, 4, H, W)).astype(F32)


def _case(name, Hs, Ws, H, W, T, image_hw, normalize, objects, ltrb_at=(), seed=0, **over):
    """objects: {object index: dict(blobs=[(r, c, a)], base, center, prev_vec, neigh, [spikes=[(r, c, value)]])} in cells of the (H, W) decision map (spikes: raw cells,
    maps used as they are only); ltrb_at: [(index, (l, t, r, b))] written at EVERY cell of that object's ltrb map."""
    fr = _frame(H, W, image_hw, normalize, **over)
    scores = np.zeros((T, Hs, Ws), F32)
    states = OrderedDict()
    for t, ob in objects.items():
        scores[t] = _scores(seed + 17 * t, Hs, Ws, H, W, ob.get("blobs", ()), ob.get("base", -3.0 if normalize else 0.0))
        for r, c, v in ob.get("spikes", ()):
            scores[t, r, c] = v
        states[t] = _state(fr, H, W, ob["center"], ob.get("prev_vec", (0.0, 0.0)), ob.get("neigh", (3.3, 3.3)))
    ltrb = _ltrb(seed + 1000, T, H, W)
    for t, v in ltrb_at:
        ltrb[t] = np.asarray(v, F32)[:, None, None]
    return dict(name=name, scores=scores, ltrb=ltrb, frame=fr, objects=states, active=list(objects), T=T, H=H, W=W)


def _build():
    cases = OrderedDict()
    # 5 x 7 as it is, raw scores, T = 2.  object 0: the peak in the corner (0, 0), nothing else -> normal.
    # object 1: an exact tie between (2, 5) and (4, 1): max2d takes the smaller column, (4, 1); the other one is a distractor that is far from
    # where the object was while the winner is near -> hard_negative at peak 1 (statement 4).
    cases["asis5x7"] = _case("asis5x7", 5, 7, 5, 7, 2, (60, 112), False, OrderedDict([
        (0, dict(spikes=[(0, 0, 1.0), (3, 4, 0.2)], center=(0.0, 0.0), neigh=(2.0, 2.0))),
        (1, dict(spikes=[(2, 5, 0.9), (4, 1, 0.9)], center=(4.0, 1.0), neigh=(2.0, 2.0))),
    ]), seed=11)
    # 6 x 9 -> 12 x 18 bicubic, sigmoid, wide image (the width decides the scale), T = 16 with nine active objects and gaps in the ids: one
    # per return statement.  Every object has a second, lower blob, so that the second peak is a blob too and not a cell of the noise.
    hi, mid, sub, far = 5.0, 4.4, 3.2, 1.2            # heights above base -3: about sigmoid(2), sigmoid(1.4), sigmoid(.2), sigmoid(-1.8) at the peak
    nine = OrderedDict([
        (0, dict(blobs=[(5, 7, far), (9, 14, 0.6)], center=(5.0, 7.0))),                                    # 1 not_found: peak < .25
        (1, dict(blobs=[(5, 7, 2.6), (9, 14, far)], center=(5.0, 7.0))),                                    # 2 uncertain: .25 < peak < .5
        (2, dict(blobs=[(5, 7, 3.5), (9, 14, far)], center=(5.0, 7.0))),                                    # 3 hard sample: .5 < peak < .7
        (4, dict(blobs=[(3, 5, hi), (8, 14, mid)], center=(3.0, 5.0))),                                     # 4 far 2, near 1
        (5, dict(blobs=[(3, 5, hi), (8, 14, mid)], center=(8.0, 14.0))),                                    # 5 near 2, far 1 -> peak 2
        (6, dict(blobs=[(1, 1, hi), (10, 16, mid)], center=(5.0, 8.0), neigh=(2.0, 2.0))),                  # 6 both far
        (7, dict(blobs=[(5, 6, hi), (5, 11, mid)], center=(5.0, 9.0))),                                     # 7 both near
        (8, dict(blobs=[(3, 5, hi), (8, 14, sub)], center=(3.0, 5.0))),                                     # 8 hard negative: .5 < peak 2 / peak 1 < .8
        (15, dict(blobs=[(7, 11, hi), (2, 3, far)], center=(7.0, 11.0), prev_vec=(0.5, -0.5))),             # 9 normal
    ])
    cases["up6x9_wide"] = _case("up6x9_wide", 6, 9, 12, 18, 16, (120, 400), True, nine, seed=23,
                                uncertain_threshold=0.5, hard_sample_threshold=0.7, dispalcement_scale=0.5)
    # the same sizes, raw scores, tall image (the height decides the scale), T = 1, the peak on the bottom border; a power-of-two ratio and
    # target_neighborhood_scale 2 make target_neigh_sz exactly 3: both bounds r -+ 1.5 land on .5
    cases["up6x9_tall"] = _case("up6x9_tall", 6, 9, 12, 18, 1, (192, 200), False, OrderedDict([
        (0, dict(blobs=[(11, 9, 1.0), (3, 3, 0.3)], center=(11.0, 9.0), neigh=(3.0, 3.0))),
    ]), seed=31, target_neighborhood_scale=2.0, hard_negative_threshold=0.45)
    # 12 x 18 as it is (sigmoid), T = 4: peaks on the top / left / right border, each object's ltrb constant so that one side of the box leaves
    # the image; object 3: a box that sits beyond the far corner -> minimum width and height.  Object 2 also carries the rounding trap: peak in
    # row 4 with target_neigh_sz 3 -> top = round(2.5) = 2 (half to even), and a second blob in row 2 that only half-up rounding leaves unmasked.
    cases["asis12x18_clip"] = _case("asis12x18_clip", 12, 18, 12, 18, 4, (96, 144), True, OrderedDict([
        (0, dict(blobs=[(0, 8, 5.0), (8, 2, 1.2)], center=(0.0, 8.0))),                                        # top border; box leaves at the top and left
        (1, dict(blobs=[(6, 0, 5.0), (2, 12, 1.2)], center=(6.0, 0.0))),                                       # left border; box leaves at the bottom and right
        (2, dict(blobs=[(4, 17, 5.0), (9, 4, 1.2)], spikes=[(2, 17, 1.0)], center=(4.0, 17.0), neigh=(3.0, 3.0))),   # right border
        (3, dict(blobs=[(11, 17, 5.0), (3, 6, 1.2)], center=(11.0, 17.0))),                                    # bottom-right corner
    ]), ltrb_at=[(0, (0.9, 0.9, 0.1, 0.1)), (1, (0.0, 0.1, 2.5, 2.5)), (3, (-0.3, -0.3, 0.31, 0.31))], seed=41, target_neighborhood_scale=2.0)
    # the deployed sizes: 24 x 36 -> 48 x 72, sigmoid, two objects
    cases["deployed"] = _case("deployed", 24, 36, 48, 72, 2, (480, 854), True, OrderedDict([
        (0, dict(blobs=[(21, 25, 5.0), (37, 61, 3.4)], center=(21.0, 25.0), neigh=(6.0, 9.0))),
        (1, dict(blobs=[(47, 71, 5.0), (12, 20, 1.2)], center=(47.0, 71.0), neigh=(5.0, 5.0))),
    ]), seed=53)
    return cases


CASES = _build()
# the statement of localize_advanced (tamos.py:386-429, 1..9 in source order) each object is built to reach
STATEMENTS = {"asis5x7": [9, 4], "up6x9_wide": [1, 2, 3, 4, 5, 6, 7, 8, 9], "up6x9_tall": [9], "asis12x18_clip": [9, 9, 9, 9], "deployed": [8, 9]}

# ---- what the library refuses before anything is queued: (name, frame overrides, T, (Hs, Ws, H, W)) -> PT_MOT_ERR_UNSUPPORTED -------------------
REFUSALS = [
    ("T = 0", {}, 0, (6, 9, 12, 18)), ("T = 17", {}, 17, (6, 9, 12, 18)), ("map beyond the LDS plan", {}, 1, (64, 100, 128, 200)),
    ("score_preprocess", dict(score_preprocess=1), 1, (6, 9, 12, 18)), ("score_filter_ksz", dict(score_filter_ksz=3), 1, (6, 9, 12, 18)),
    ("window_output", dict(window_output=1), 1, (6, 9, 12, 18)), ("advanced_localization off", dict(advanced_localization=0), 1, (6, 9, 12, 18)),
    ("even kernel_size", dict(kernel_size=(2.0, 2.0)), 1, (6, 9, 12, 18)),
]

# ---- training targets ------------------------------------------------------------------------------------------------------------------------------
IMAGE_SAMPLE_SIZE = (96, 144)                           # 12 x 18 cells of stride 8


def target_boxes(nf, T=3):
    """(nf, T, 4) xywh in sample pixels; object 1 of every frame is empty (w = 0), the last object of the last frame has h < 0"""
    rng = np.random.default_rng(70 + nf)
    b = np.concatenate([rng.uniform(-10, 100, (nf, T, 2)), rng.uniform(4, 60, (nf, T, 2))], -1).astype(F32)
    b[:, 1, 2] = 0
    b[-1, -1, 3] = -3
    return b


LABEL = dict(feature_sz=(12.0, 18.0), sigma=(0.9185586, 0.9185586), end_pad=(0.0, 0.0))       # 1/4 / 4 * sqrt(12 * 18), as an fp32 value
# centres [row, col] in label cells relative to the middle: inside, on a half cell, far off the map (every value underflows towards 0)
LABEL_CENTRES = np.array([[0.0, 0.0], [-3.25, 6.5], [5.5, -8.5], [40.0, -60.0]], F32)


# The factor of the device bound may never reach the miss of the weakest seeded defect (tests/test_tamos_readout_cpu.py asserts that every
# defect of tamos_readout_np.DEFECTS misses by more than this): the cap f64_bound.raised_factor() takes in tests/test_gpu_tamos_readout.py.
F_MAX = 1000


def frame_block(fr):
    """`pt_mot_frame` of a frame dict of this table"""
    from pytracking_amd import _lib_mot
    f = _lib_mot.MotFrame()
    for k in ("target_not_found_threshold", "uncertain_threshold", "hard_sample_threshold", "distractor_threshold", "hard_negative_threshold",
              "target_neighborhood_scale", "dispalcement_scale", "scale_factor", "image_h", "image_w", "stride", "min_width", "min_height",
              "normalize_scores", "score_preprocess", "score_filter_ksz", "window_output", "advanced_localization"):
        setattr(f, k, fr[k])
    for k in ("img_support_sz", "img_sample_sz", "train_img_sample_sz", "kernel_size", "sample_coords"):
        getattr(f, k)[:] = list(fr[k])
    return f


def object_block(st):
    """`pt_mot_object` of an object state of this table"""
    from pytracking_amd import _lib_mot
    o = _lib_mot.MotObject()
    for k in ("pos", "pos_prev", "target_sz"):
        getattr(o, k)[:] = [float(v) for v in st[k]]
    return o


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"tamos_readout_{name}.npz")))


def run(case, dtype=np.float64, defect=None):
    return RN.readout(case["scores"], case["ltrb"], case["frame"], case["objects"], case["active"], dtype, defect)
