"""numpy restatement of the TaMOs per-frame multi-object read-out and of its training targets, in float64 or fp32 (`dtype`), written
from the reference's lines (pytracking/tracker/tamos/tamos.py, pytracking/libs/dcf.py) and torch's documented interpolation:

    bicubic(...)            tamos.py:319-320   F.interpolate(target_scores[0], bbox_preds.shape[-2:], mode='bicubic')
    sigmoid                 tamos.py:173-174
    constants(...)          tamos.py:369-372, 394, 408, 414   (always fp32: host state of the tracker, fp32 CPU tensors)
    max2d(...)              dcf.py:156-164
    localize(...)           tamos.py:366-429   (no output window)
    box(...)                tamos.py:248-280
    clip(...)               tamos.py:106-112
    encode_bbox(...)        tamos.py:114-153
    label(...)              tamos.py:582-592, dcf.py:48-59

What is a float64 / fp32 choice and what is not: the maps (bicubic, sigmoid), the box arithmetic, the targets and the label follow `dtype`.
The tracker's host state is fp32 by construction (torch.Tensor on the CPU) and Python scalars that meet an fp32 tensor are rounded to fp32
by torch's binary operators; both runs therefore use the SAME fp32 constants, exactly as the reference forms them.  `tensor.item() <
python float` compares doubles; Python's round() is round-half-to-even.

`defect` names one seeded defect (DEFECTS): the CPU tests show that each of them misses the bound the device is held to.
Test infrastructure only; reads nothing outside the repository."""
import math
from collections import OrderedDict

import numpy as np

F32 = np.float32
FLAGS = ("normal", "hard_negative", "uncertain", "not_found")                 # the codes of PT_MOT_* / PT_LOC_*
DEFECTS = ("align_corners", "cubic_a", "round_half_up", "train_sz_order", "no_half_stride", "clip_min_size")


# ---- maps ------------------------------------------------------------------------------------------------------------------------
def _cubic_weights(t, A, dtype):
    """torch's cubic convolution coefficients for the taps at floor(x) - 1 .. floor(x) + 2 (aten UpSample.h: get_cubic_upsample_coefficients)"""
    t = t.astype(dtype)
    A = dtype(A)

    def c1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def c2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], -1)


def _axis(n_in, n_out, dtype, align_corners):
    dst = np.arange(n_out, dtype=dtype)
    if align_corners:
        src = dst * (dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0))
    else:
        src = dtype(n_in) / dtype(n_out) * (dst + dtype(0.5)) - dtype(0.5)         # area_pixel_compute_source_index(cubic=True): no clamp
    fl = np.floor(src)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None], 0, n_in - 1)   # taps clamped to the map
    return idx, (src - fl)


def bicubic(x, H, W, dtype=np.float64, defect=None):
    """x (T, Hs, Ws) -> (T, H, W): rows first inside a tap row, then the four rows (upsample_bicubic2d)"""
    x = np.asarray(x, dtype=dtype)
    A = -0.5 if defect == "cubic_a" else -0.75
    iy, ty = _axis(x.shape[1], H, dtype, defect == "align_corners")
    ix, tx = _axis(x.shape[2], W, dtype, defect == "align_corners")
    wy, wx = _cubic_weights(ty, A, dtype), _cubic_weights(tx, A, dtype)
    out = np.zeros((x.shape[0], H, W), dtype=dtype)
    for u in range(4):
        rows = x[:, iy[:, u], :]                                                  # (T, H, Ws)
        r = np.zeros((x.shape[0], H, W), dtype=dtype)
        for k in range(4):
            r = r + wx[None, None, :, k] * rows[:, :, ix[:, k]]
        out = out + wy[None, :, u, None] * r
    return out


def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return (dtype(1) / (dtype(1) + np.exp(-x))).astype(dtype)


def decision_map(scores, H, W, normalize, dtype=np.float64, defect=None):
    """The map `track()` localises on (tamos.py:319-320, 173-174): as it is when a size agrees, else bicubic; then the sigmoid."""
    scores = np.asarray(scores, dtype=dtype)
    if scores.shape[-1] != W and scores.shape[-2] != H:
        scores = bicubic(scores, H, W, dtype, defect)
    return sigmoid(scores, dtype) if normalize else scores


# ---- localize_advanced ---------------------------------------------------------------------------------------------------------------
def constants(frame, obj, H, W):
    """score_center, target_neigh_sz, prev_target_vec, disp_threshold of tamos.py:369-372,394,408,414 in the reference's fp32 operation order"""
    out_sz = np.array([H, W], F32) - np.mod(np.asarray(frame["kernel_size"], F32) + F32(1), F32(2))
    ratio = (np.asarray(frame["img_support_sz"], F32) / out_sz) / F32(frame["scale_factor"])
    pos, prev, tsz = (np.asarray(obj[k], F32) for k in ("pos", "pos_prev", "target_sz"))
    return dict(center=pos / ratio, neigh=(tsz / ratio) * F32(frame["target_neighborhood_scale"]), prev=(pos - prev) / ratio,
                disp_threshold=F32(frame["dispalcement_scale"] * math.sqrt(H * W) / 2))


def max2d(m):
    """dcf.max2d: torch.max over rows, then over columns, each returning the first index -> ties go to the smallest column, then row"""
    col_max, col_arg = m.max(0), m.argmax(0)
    c = int(col_max.argmax())
    return m.dtype.type(col_max[c]), int(col_arg[c]), c


def _py_round(x, defect):
    return int(math.floor(x + 0.5)) if defect == "round_half_up" else round(x)


def _peak_margin(m, cell, tied):
    """distance of the winner from the best cell that is not an exact tie of it (`tied`: boolean map of the cells whose value equals the
    winner's in every precision)"""
    rest = np.where(tied, -np.inf, m)
    rest[cell] = -np.inf
    return float(m[cell] - rest.max()) if np.isfinite(rest.max()) else math.inf


def localize(m, raw_exact, frame, cst, defect=None):
    """m (H, W): one object's map.  raw_exact: (H, W) array whose equal entries mark cells that are equal in every precision (the raw map
    when it is used as it is), or None.  -> dict: flag code, statement (1..9: which return of tamos.py:386-429), pick, cell, both peaks,
    second (second peak searched), mask bounds, margins {test: |lhs - rhs|} of every discrete decision."""
    T = m.dtype.type
    H, W = m.shape
    margins = OrderedDict()
    v1, r1, c1 = max2d(m)
    tied = np.zeros((H, W), bool) if raw_exact is None else raw_exact == raw_exact[r1, c1]
    margins["peak1"] = _peak_margin(m, (r1, c1), tied)
    out = dict(max1=v1, peak1=(r1, c1), max2=T(0), peak2=(0, 0), pick=1, second=False, mask=(0, 0, 0, 0))
    m1 = float(v1)                                                                # .item(): a double
    for stmt, flag, key in ((1, 3, "target_not_found_threshold"), (2, 2, "uncertain_threshold"), (3, 1, "hard_sample_threshold")):
        thr = frame.get(key, -math.inf)
        if math.isfinite(thr):
            margins[key] = abs(m1 - thr)
        if m1 < thr:
            out.update(flag=flag, statement=stmt, cell=(r1, c1), margins=margins)
            return out
    nr, nc = float(cst["neigh"][0]), float(cst["neigh"][1])
    top = max(_py_round(r1 - nr / 2, defect), 0)
    bottom = min(_py_round(r1 + nr / 2 + 1, defect), H)
    left = max(_py_round(c1 - nc / 2, defect), 0)
    right = min(_py_round(c1 + nc / 2 + 1, defect), W)
    masked = m.copy()
    masked[top:bottom, left:right] = 0
    v2, r2, c2 = max2d(masked)
    inmask = np.zeros((H, W), bool)
    inmask[top:bottom, left:right] = True
    if inmask[r2, c2]:
        tied2 = inmask
    else:
        tied2 = np.zeros((H, W), bool) if raw_exact is None else (raw_exact == raw_exact[r2, c2]) & ~inmask
    margins["peak2"] = _peak_margin(masked, (r2, c2), tied2)
    out.update(max2=v2, peak2=(r2, c2), second=True, mask=(top, bottom, left, right))
    d1 = (np.array([r1, c1], F32) - cst["center"]) - cst["prev"]                   # target_disp - prev_target_vec, fp32 tensors
    d2 = (np.array([r2, c2], F32) - cst["center"]) - cst["prev"]
    n1, n2 = np.sqrt((d1 * d1).sum(dtype=F32)), np.sqrt((d2 * d2).sum(dtype=F32))
    th = cst["disp_threshold"]
    dist, hn, nf = (T(F32(frame[k])) for k in ("distractor_threshold", "hard_negative_threshold", "target_not_found_threshold"))
    margins["distractor"] = abs(float(v2) - float(dist * v1))
    if v2 > dist * v1:
        margins["disp1"], margins["disp2"] = abs(float(n1) - float(th)), abs(float(n2) - float(th))
        if n2 > th and n1 < th:
            out.update(flag=1, statement=4)
        elif n2 < th and n1 > th:
            out.update(flag=1, statement=5, pick=2)
        elif n2 > th and n1 > th:
            out.update(flag=2, statement=6)
        else:
            out.update(flag=2, statement=7)
    else:
        margins["hard_negative"] = abs(float(v2) - float(hn * v1))
        if v2 > hn * v1:
            margins["hard_negative_nf"] = abs(float(v2) - float(nf))
        if v2 > hn * v1 and v2 > nf:
            out.update(flag=1, statement=8)
        else:
            out.update(flag=0, statement=9)
    out.update(cell=(r1, c1) if out["pick"] == 1 else (r2, c2), margins=margins)
    return out


# ---- direct_bbox_regression and clip_bbox_to_image_area --------------------------------------------------------------------------------------
def box(ltrb4, cell, frame, dtype=np.float64, defect=None):
    """tamos.py:248-280 at `cell`: [x1, y1, w, h]"""
    T = dtype
    stride = int(frame["stride"])
    half = 0 if defect == "no_half_stride" else stride // 2
    xs, ys = T(cell[1] * stride + half), T(cell[0] * stride + half)                # locations = shifts + stride // 2
    th, tw = (T(v) for v in frame["train_img_sample_sz"])
    order = (th, tw, th, tw) if defect == "train_sz_order" else (tw, th, tw, th)    # train_img_sample_sz[[1, 0, 1, 0]]
    l, t, r, b = (T(v) * s for v, s in zip(ltrb4, order))
    xs1, xs2, ys1, ys2 = xs - l, xs + r, ys - t, ys + b
    sh, sw = (T(v) for v in frame["img_sample_sz"])
    y0, x0, y1, x1 = (T(v) for v in frame["sample_coords"])
    bx1 = xs1 / sw * (x1 - x0) + x0
    by1 = ys1 / sh * (y1 - y0) + y0
    bx2 = xs2 / sw * (x1 - x0) + x0
    by2 = ys2 / sh * (y1 - y0) + y0
    return np.array([bx1, by1, bx2 - bx1, by2 - by1], dtype=dtype)


def clip(b, frame, dtype=np.float64, defect=None):
    """tamos.py:106-112"""
    T = dtype
    Hi, Wi = T(frame["image_h"]), T(frame["image_w"])
    mw, mh = (T(0), T(0)) if defect == "clip_min_size" else (T(frame["min_width"]), T(frame["min_height"]))
    b = [T(v) for v in b]
    x1 = max(T(0), min(b[0], Wi - mw))
    y1 = max(T(0), min(b[1], Hi - mh))
    x2 = max(x1 + mw, min(b[0] + b[2], Wi))
    y2 = max(y1 + mh, min(b[1] + b[3], Hi))
    return np.array([x1, y1, x2 - x1, y2 - y1], dtype=dtype)


def readout(scores, ltrb, frame, objects, active, dtype=np.float64, defect=None):
    """One frame.  scores (T, Hs, Ws), ltrb (T, 4, H, W), objects: {index: state} of the active object indices `active`.
    -> OrderedDict of arrays over the active objects, in the order of `active`: floats map, max1, max2, raw_box, box in `dtype`; ints
    flag, statement, pick, cell, peak1, peak2, second, mask; `margins`: one dict per object."""
    H, W = ltrb.shape[-2:]
    maps = decision_map(scores, H, W, frame["normalize_scores"], dtype, defect)
    exact = scores.shape[-2:] == (H, W)
    rows = []
    for t in active:
        cst = constants(frame, objects[t], H, W)
        loc = localize(maps[t], np.asarray(scores[t]) if exact else None, frame, cst, defect)
        l4 = np.asarray(ltrb[t][:, loc["cell"][0], loc["cell"][1]], dtype=dtype)
        raw = box(l4, loc["cell"], frame, dtype, defect)
        rows.append(dict(loc, raw_box=raw, box=clip(raw, frame, dtype, defect), map=maps[t], ltrb=l4))
    out = OrderedDict()
    for k in ("map", "max1", "max2", "raw_box", "box", "ltrb"):
        out[k] = np.stack([np.asarray(r[k], dtype=dtype) for r in rows])
    for k in ("flag", "statement", "pick", "cell", "peak1", "peak2", "second", "mask"):
        out[k] = np.array([r[k] for r in rows], dtype=np.int64)
    out["margins"] = [r["margins"] for r in rows]
    return out


FLOAT_OUTPUTS = ("map", "max1", "max2", "raw_box", "box")
DISCRETE_OUTPUTS = ("flag", "pick", "cell", "peak1", "peak2", "second")


# ---- training targets -------------------------------------------------------------------------------------------------------------------
def encode_bbox(boxes, image_sample_size, stride, dtype=np.float64, defect=None):
    """tamos.py:114-153 for boxes (..., 4) xywh -> (..., 4, H3, W3); zeros where w <= 0 or h <= 0"""
    b = np.asarray(boxes, dtype=dtype).reshape(-1, 4)
    oh, ow = int(image_sample_size[0]), int(image_sample_size[1])
    half = 0 if defect == "no_half_stride" else stride // 2
    xs = (np.arange(0, ow, stride).astype(dtype) + dtype(half))[None, None, :]
    ys = (np.arange(0, oh, stride).astype(dtype) + dtype(half))[None, :, None]
    x0, y0, w, h = (b[:, k][:, None, None] for k in range(4))
    full = np.broadcast_to
    shape = (b.shape[0], ys.shape[1], xs.shape[2])
    out = np.stack([full((xs - x0) / dtype(ow), shape), full((ys - y0) / dtype(oh), shape),
                    full(((x0 + w) - xs) / dtype(ow), shape), full(((y0 + h) - ys) / dtype(oh), shape)], 1).astype(dtype)
    out[~((b[:, 2] > 0) & (b[:, 3] > 0))] = 0
    return out.reshape(np.asarray(boxes).shape[:-1] + out.shape[1:])


def label_centre(pos, frame, feature_sz):
    """`center` of tamos.py:585-589 in the reference's fp32 operation order; pos [row, col] fp32"""
    sup = np.asarray(frame["img_support_sz"], F32)
    norm = (np.asarray(pos, F32) * F32(frame["scale_factor"]) - sup / F32(2)) / sup
    even = np.mod(np.asarray(frame["kernel_size"], F32) + F32(1), F32(2))
    return np.asarray(feature_sz, F32) * norm + F32(0.5) * even


def label(centres, feature_sz, sigma, end_pad, dtype=np.float64):
    """dcf.label_function_spatial (dcf.py:48-59) for centres (n, 2) fp32 -> (n, sz0 + end_pad0, sz1 + end_pad1)"""
    g = []
    for d in range(2):
        sz, sg, ep = float(feature_sz[d]), float(sigma[d]), float(end_pad[d])
        k = np.arange(-(sz - 1) / 2, (sz + 1) / 2 + ep).astype(dtype)             # torch.arange: fp32 samples, exact halves
        coef = dtype(F32(-1.0 / (2 * sg ** 2)))                                   # a Python float meeting an fp32 tensor
        c = np.asarray(centres, F32)[:, d].astype(dtype)
        g.append(np.exp(coef * (k[None] - c[:, None]) ** 2))
    return (g[0][:, :, None] * g[1][:, None, :]).astype(dtype)
