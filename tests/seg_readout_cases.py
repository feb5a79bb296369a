"""Shared by tests/test_seg_readout_cpu.py, tests/test_gpu_seg_readout.py, tools/make_golden_seg_readout.py and tools/bench_seg_readout.py:
the case tables of the segmentation read-out (seg_readout.hip), the synthesis of their inputs from seeds, and float64 numpy restatements of
what the four entry points compute (include/pt_hot.h): the crop-to-image paste with its statistics, the statistics of a probability image,
the soft aggregation of N objects, and the zero-padded nearest mask patch (whose index rule is fp32 BY DEFINITION: ATen's).  Reads nothing
outside the repository.  Test infrastructure only."""
import math
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SZ_FACTOR = 4
FILL = -100.0

# name: crop (Hc, Wc), image (Hi, Wi), scale factor, window centre (row, column), seed
READOUT_CASES = OrderedDict((
    ("topleft", ((5, 7), (9, 11), 1.37, (1.2, 2.3), 4100)),            # hangs off the top-left; int() and floor differ on both axes
    ("inside", ((12, 20), (16, 16), 0.61, (8.0, 8.5), 4101)),
    ("larger", ((12, 20), (10, 14), 1.9, (5.0, 7.0), 4102)),           # the window exceeds the image on all four sides
    ("bottomright", ((30, 52), (40, 70), 1.13, (30.5, 50.25), 4103)),
    ("one", ((1, 1), (3, 3), 2.0, (1.5, 1.5), 4104)),
    ("ragged_a", ((64, 64), (131, 197), 2.3, (70.0, 100.0), 4105)),    # 9 x 4 tiles of 16 x 64, ragged on both sides, W % 4 != 0
    ("ragged_b", ((64, 64), (257, 70), 1.7, (140.0, 30.0), 4106)),     # 17 x 2 tiles
    ("deployed", ((480, 832), (720, 1280), 1.31, (350.4, 600.7), 4107)),
))
# the trackers hold the scale factor in a float32 tensor: the cases' factors are float32 values
READOUT_CASES = OrderedDict((k, (c, i, float(np.float32(s)), p, seed)) for k, (c, i, s, p, seed) in READOUT_CASES.items())
MISS = ((12, 20), (16, 16), float(np.float32(0.61)), (-40.0, 8.0), 4108)                  # the window misses the image: no golden (the reference raises)
SUBSAMPLE = {"deployed": 4}                                            # the golden keeps every 4th row and column of the big image

# name: N, (H, W), seed
MERGE_CASES = OrderedDict((
    ("n1", (1, (9, 11), 4200)), ("n3", (3, (17, 23), 4201)), ("n6", (6, (33, 40), 4202)), ("n16", (16, (8, 8), 4203)),
    ("n3_tiles", (3, (131, 197), 4204)),
))

# name: image (H, W), centre, sample_sz, output_sz (None: the crop), mode, seed.  The nearest resize runs from the padded crop to the
# output: the size pairs on which the float64 index rule goes wrong (26 -> 22, 30 -> 22, 30 -> 26) sit on those axes.  (A crop has an
# even size only where its corner is negative: the reference's half-pixel corners truncate towards zero.)
PATCH_CASES = OrderedDict((
    ("ordinary", ((37, 53), (18.0, 26.0), (30.0, 50.0), (24, 40), "replicate", 4300)),
    ("df2", ((90, 120), (9.0, 11.0), (52.0, 60.0), (22, 26), "replicate", 4301)),            # stride 2, crop 26 x 30 -> 22 x 26
    ("df2_odd", ((91, 121), (8.0, 11.0), (52.0, 60.0), (22, 26), "replicate", 4302)),        # stride 2 with offsets (0, 1)
    ("df2_in", ((90, 120), (41.0, 57.0), (52.0, 60.0), (22, 26), "replicate", 4310)),        # stride 2, crop 27 x 31 inside the image
    ("p30_22", ((48, 44), (4.0, 3.0), (30.0, 26.0), (22, 22), "replicate", 4303)),           # 30 -> 22 and 26 -> 22
    ("topleft", ((37, 53), (2.0, 3.0), (30.0, 50.0), (24, 40), "replicate", 4304)),
    ("bottomright", ((37, 53), (35.0, 50.0), (30.0, 50.0), (24, 40), "replicate", 4305)),
    ("allsides", ((20, 24), (10.0, 12.0), (30.0, 50.0), (24, 40), "replicate", 4306)),      # the crop exceeds the image on all sides
    ("same", ((37, 53), (5.0, 2.0), (24.0, 40.0), (24, 40), "replicate", 4307)),           # no resize: the padded crop itself
    ("nosize", ((37, 53), (30.0, 9.0), (17.0, 21.0), None, "replicate", 4308)),
    ("inside", ((37, 53), (2.0, 50.0), (30.0, 50.0), (24, 40), "inside", 4309)),
))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def blob_scores(seed, H, W, amp=6.0, offset=-3.0, noise=0.3):
    """A smooth blob plus noise, fp32: positive inside, negative outside, no pixel on the zero crossing by construction of the noise."""
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
    sy, sx = max(0.22 * H, 0.8), max(0.22 * W, 0.8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    s = amp * np.exp(-((y - cy) ** 2 / (2 * sy * sy) + (x - cx) ** 2 / (2 * sx * sx))) + offset + noise * rng.standard_normal((H, W))
    return s.astype(np.float32)


def readout_input(name):
    (Hc, Wc), _, _, _, seed = READOUT_CASES[name] if name != "miss" else MISS
    return blob_scores(seed, Hc, Wc)


def merge_ids(N):
    return [2 * k + 1 for k in range(N)]                                 # not the positions: the label map is mapped through the ids


def merge_input(name):
    """(scores (N, H, W) fp32 as merge_results stacks them, out_all-style entries): one object enters as a 0/1 mask (-> +-100), the rows
    of the top third of another sit at -100 (what the crop-to-image paste leaves outside the search window)."""
    N, (H, W), seed = MERGE_CASES[name]
    maps, entries = [], []
    for k in range(N):
        raw = blob_scores(seed + 10 * (k + 1), H, W)
        if k == 0 and N > 1:
            seg = (raw > 0).astype(np.float32)
            entries.append({"segmentation": seg})
            maps.append((seg - 0.5) * 200.0)
            continue
        if k == (1 if N > 1 else 0):
            raw[:max(H // 3, 1)] = FILL
        entries.append({"segmentation_raw": raw})
        maps.append(raw)
    return np.stack(maps).astype(np.float32), entries


def patch_input(name):
    (H, W), _, _, _, _, seed = PATCH_CASES[name]
    return (1.0 / (1.0 + np.exp(-blob_scores(seed, H, W).astype(np.float64)))).astype(np.float32)


def golden(kind, name):
    with np.load(os.path.join(GOLDEN, f"seg_readout_{kind}_{name}.npz")) as g:
        return {k: g[k] for k in g.files}


# ---- float64 restatements --------------------------------------------------------------------------------------------------------
def placement(crop_hw, image_hw, scale, pos):
    """(Hr, Wr, r1, c1): F.interpolate's output size for scale_factor and lwl.py:342-343 -- int() truncates towards zero."""
    Hr, Wr = int(math.floor(crop_hw[0] * float(scale))), int(math.floor(crop_hw[1] * float(scale)))
    return Hr, Wr, int(float(pos[0]) - 0.5 * Hr), int(float(pos[1]) - 0.5 * Wr)


def _axis(n_in, n_out, scale):
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) / scale - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), np.clip(src - i0, 0.0, 1.0)


def resize_f64(scores, scale):
    """F.interpolate(scale_factor=scale, mode='bilinear', align_corners=False), no recomputed scale factor, in float64."""
    s = np.asarray(scores, dtype=np.float64)
    Hr, Wr = int(math.floor(s.shape[0] * float(scale))), int(math.floor(s.shape[1] * float(scale)))
    y0, y1, wy = _axis(s.shape[0], Hr, float(scale))
    x0, x1, wx = _axis(s.shape[1], Wr, float(scale))
    top = s[y0][:, x0] * (1 - wx) + s[y0][:, x1] * wx
    bot = s[y1][:, x0] * (1 - wx) + s[y1][:, x1] * wx
    return top * (1 - wy)[:, None] + bot * wy[:, None]


def state_f64(prob, mask):
    """The statistics block (include/pt_hot.h) of a probability image and a boolean mask, as a dict, in float64."""
    p = np.asarray(prob, dtype=np.float64)
    H, W = p.shape
    out = OrderedDict()
    for tag, q in (("", p), ("_c", np.maximum(p, 0.0))):
        rows, cols, tot = q.sum(1), q.sum(0), q.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            e_y, e_x = (rows * np.arange(H)).sum() / tot, (cols * np.arange(W)).sum() / tot
            out["prob_sum" + tag], out["e_y" + tag], out["e_x" + tag] = tot, e_y, e_x
            out["var_y" + tag] = (rows * (np.arange(H) - e_y) ** 2).sum() / tot
            out["var_x" + tag] = (cols * (np.arange(W) - e_x) ** 2).sum() / tot
    m = np.asarray(mask, dtype=bool)
    out["mask_count"] = float(m.sum())
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    out["bbox"] = np.array([xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) and len(ys) else [0, 0, 0, 0], dtype=np.float64)
    return out


STAT_KEYS = ("prob_sum", "e_y", "e_x", "var_y", "var_x", "prob_sum_c", "e_y_c", "e_x_c", "var_y_c", "var_x_c", "mask_count")


def stats_dict(block):
    """A device / host statistics block (16 floats) as the dict state_f64 returns."""
    b = np.asarray(block, dtype=np.float64).reshape(-1)
    out = OrderedDict(zip(STAT_KEYS, b[:11]))
    out["bbox"] = b[11:15].copy()
    return out


def readout_f64(scores, image_hw, scale, pos):
    """dict(scores_im, prob_im, mask_im, stats, window=(r1, c1, Hr, Wr)) of the crop-to-image read-out in float64."""
    Hi, Wi = image_hw
    Hr, Wr, r1, c1 = placement(np.shape(scores), image_hw, scale, pos)
    re = resize_f64(scores, scale)
    im = np.full((Hi, Wi), FILL, dtype=np.float64)
    ya, yb, xa, xb = max(r1, 0), min(r1 + Hr, Hi), max(c1, 0), min(c1 + Wr, Wi)
    if ya < yb and xa < xb:
        im[ya:yb, xa:xb] = re[ya - r1:yb - r1, xa - c1:xb - c1]
    prob = 1.0 / (1.0 + np.exp(-im))
    return dict(scores_im=im, prob_im=prob, mask_im=(im > 0).astype(np.float64), stats=state_f64(prob, im > 0), window=(r1, c1, Hr, Wr))


def target_state_f64(stats, kind):
    """(pos, size) of get_target_state from a statistics dict: LWL the plain moments, RTS those of max(p, 0)."""
    t = "" if kind == "lwl" else "_c"
    return (np.array([stats["e_y" + t], stats["e_x" + t]]),
            np.array([math.sqrt(stats["var_y" + t]), math.sqrt(stats["var_x" + t])]) * SZ_FACTOR)


def merge_f64(scores):
    """dict(prob (N + 1, H, W) background first, labels (H, W) uint8 positions, gap = largest minus second largest probability,
    stats = per object the statistics dict of its probability with its label region) of lwl.py:228-248 in float64."""
    s = np.asarray(scores, dtype=np.float64)
    eps = 1e-7
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-s))
        bg = np.clip(np.prod(1 - p, axis=0), eps, 1.0 - eps)
        allS = np.concatenate([np.log(bg / (1 - bg))[None], s], 0)
        prob = np.stack([1.0 / np.exp(allS - si[None]).sum(0) for si in allS])
    labels = prob.argmax(0).astype(np.uint8)
    srt = np.sort(prob, axis=0)
    gap = srt[-1] - srt[-2]
    return dict(prob=prob, labels=labels, gap=gap, stats=[state_f64(prob[i + 1], labels == i + 1) for i in range(s.shape[0])])


def nearest_index(n_in, n_out):
    """ATen's legacy 'nearest' source index, computed in fp32 as ATen does: min((int)floorf(dst * ((float)in / (float)out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def nearest_index_f64(n_in, n_out):
    """The same formula in float64: wrong for 626 of the size pairs up to 159 (26 -> 22 is the smallest)."""
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float64) * (n_in / n_out)).astype(np.int64), n_in - 1)


def mask_patch(im, geom, out_hw, index=nearest_index):
    """sample_patch(is_mask=True) for the integer geometry `geom` (pytracking_amd.preprocessing.patch_geometry): the strided view, the crop
    with zero padding, the nearest resize to `out_hw` (None: the crop).  im (H, W)."""
    view = np.asarray(im)[geom.os0::geom.df, geom.os1::geom.df]
    crop = np.zeros((geom.crop_h, geom.crop_w), dtype=view.dtype)
    ya, yb = max(geom.tl0, 0), min(geom.tl0 + geom.crop_h, view.shape[0])
    xa, xb = max(geom.tl1, 0), min(geom.tl1 + geom.crop_w, view.shape[1])
    if ya < yb and xa < xb:
        crop[ya - geom.tl0:yb - geom.tl0, xa - geom.tl1:xb - geom.tl1] = view[ya:yb, xa:xb]
    if out_hw is None or tuple(out_hw) == crop.shape:
        return crop
    return crop[index(geom.crop_h, out_hw[0])][:, index(geom.crop_w, out_hw[1])]


def patch_geometry(name):
    from pytracking_amd.preprocessing import patch_geometry as pg
    hw, pos, ssz, osz, mode, _ = PATCH_CASES[name]
    return pg(hw, pos, ssz, osz, mode)
