"""float64 numpy restatement of `ATOM.localize_target` / `localize_advanced` (pytracking/tracker/atom/atom.py:304-406) "by definition, not by
padding": the chain cfft2 / (N_h N_w) -> shift_fs -> sample_fs(output_sz) is linear and separable in the real input,

    out = A_y . (weight * s) . A_x^T,        A[y, m] = (1 + 2 sum_{k=1..N//2} cos(pi k r / (N G))) / N,
    r = (N G - p G + 2 y N - 2 m G) mod 2 N G,   p = kernel side % 2

(one real G x N matrix per axis; N: series side, G: grid side).  What the reference's quirks contribute is all in that formula:
  - for an even N `rfftshift2` (fourier.py:8-10) puts the Nyquist row at BOTH ends of the series, and the zero-padded one-sided `irfft`
    (fourier.py:59) counts the Nyquist column with its conjugate: the k = N/2 term has the weight 2 of every other term, on both axes (a
    one-hot 18 x 18 map with a 4 x 4 kernel peaks at (19/18)^2, not 1, at grid cell 16 (n + 9) mod 288);
  - `shift_fs` by pi (1 - p / N) (atom.py:310): the phase numerator N G - p G;
  - `rescale` multiplies by G_h G_w, which the inverse transform divides by: no factor is left.
The phases are reduced in integers, so the float64 run carries no argument-reduction error.

localize(case) returns every output of the reference and the MARGIN of every discrete decision it took (the gap between the two largest
values of each arg-max's map, the distance of each threshold comparison from equality, the distance of each `round` argument from a
half-integer).  `defect` seeds one of DEFECTS.  Host scalars are formed in the reference's float32 operation order (constants()).
numpy only; reads nothing outside the repository.  Test infrastructure only."""
from collections import OrderedDict

import numpy as np

FLAGS = ("normal", "hard_negative", "uncertain", "not_found")              # the codes of PT_LOC_* (include/pt_hot.h, include/pt_loc.h)
RETURN_FLAG = (None, "hard_negative", "uncertain", "not_found")            # what the reference method returns for each code
DEFECTS = ("nyquist_single", "no_inv_sz", "half_away", "roll_floor", "window_after_argmax", "mask_neg_inf")
FLOAT_OUTPUTS = ("map", "max1", "max2", "tv")
DISCRETE_OUTPUTS = ("flag", "scale_ind", "peak1", "peak2", "which")
f32 = np.float32


def interp_matrix(N, G, p, defect=None):
    """A (G, N) float64: sample y of the shifted, zero-padded series of one-hot m."""
    y = np.arange(G, dtype=np.int64)[:, None]
    m = np.arange(N, dtype=np.int64)[None, :]
    NG = N * G
    num = NG - (0 if defect == "no_inv_sz" else p * G) + 2 * y * N - 2 * m * G
    A = np.ones((G, N), np.float64)
    for k in range(1, N // 2 + 1):
        r = (k * num) % (2 * NG)
        w = 1.0 if (defect == "nyquist_single" and 2 * k == N) else 2.0
        A += w * np.cos(np.pi * (r.astype(np.float64) / NG))
    return A / N


def constants(case):
    """The host scalars of atom.py:327-331, 363-364, 373, 391 in the reference's float32 operation order."""
    G = np.asarray(case["G"], np.int64)
    out_sz = G.astype(f32)
    ratio = (np.asarray(case["img_support_sz"], f32) / out_sz).astype(f32)                 # img_support_sz / output_sz
    ts = f32(case["target_scale"])
    neigh = ((f32(case["target_neighborhood_scale"]) * np.asarray(case["target_sz"], f32)).astype(f32) / ts).astype(f32)
    return dict(ratio=ratio, target_scale=ts, neigh=neigh, center=np.floor(out_sz / f32(2)).astype(f32), half=(out_sz / f32(2)).astype(f32),
                out_sz=out_sz, disp_threshold=f32(case["dispalcement_scale"] * np.sqrt(float(G[0] * G[1])) / 2),
                scale_factors=np.asarray(case["scale_factors"], f32))


def upsample(case, defect=None):
    """(S, G_h, G_w) float64: atom.py:306-313, un-rolled, un-windowed."""
    s = np.asarray(case["scores"], f32)[:, 0]
    s = (f32(case.get("translation_weight", 1.0)) * s).astype(f32).astype(np.float64)      # atom.py:307, a float32 product
    Nh, Nw = s.shape[-2:]
    Ay = interp_matrix(Nh, case["G"][0], case["kernel"][0] % 2, defect)
    Ax = interp_matrix(Nw, case["G"][1], case["kernel"][1] % 2, defect)
    return np.einsum("ym,smn,xn->syx", Ay, s, Ax)


def roll(a, defect=None):
    """atom.py:355-356 (and :349-350): rolled[i] = a[(i + (sz + 1) // 2) % sz]"""
    for ax in (-2, -1):
        sz = a.shape[ax]
        a = np.roll(a, -((sz // 2) if defect == "roll_floor" else (sz + 1) // 2), axis=ax)
    return a


def max2d(a):
    """dcf.max2d (dcf.py:156-164) of one map: the first row of each column's maximum, then the first column.  -> value, (r, c), top-two gap"""
    col_max, col_arg = a.max(axis=0), a.argmax(axis=0)
    c = int(col_max.argmax())
    flat = np.sort(a.reshape(-1))
    return float(col_max[c]), (int(col_arg[c]), c), float(flat[-1] - flat[-2]) if flat.size > 1 else np.inf


def _round(x, defect):
    return int(np.floor(x + 0.5)) if defect == "half_away" and x >= 0 else int(-np.floor(-x + 0.5)) if defect == "half_away" else int(round(x))


def _half_distance(x):
    return abs(x - np.floor(x) - 0.5)


def localize(case, defect=None):
    c = constants(case)
    S = len(case["scores"])
    Gh, Gw = case["G"]
    win = None if case.get("window") is None else np.asarray(case["window"], f32).astype(np.float64)
    hn = bool(case.get("hn_without_windowing", False)) and win is not None
    raw = upsample(case, defect)
    margins = OrderedDict()

    def windowed(a):
        # the reference multiplies float32 maps: the float64 run multiplies the float64 map by the float32 window's values
        return a * win

    if not case["advanced"]:
        m = windowed(raw) if (win is not None and not case.get("hn_without_windowing", False)) else raw
        search = raw if (defect == "window_after_argmax" and m is not raw) else m
        peaks = [max2d(search[s]) for s in range(S)]
        vals = np.array([p[0] for p in peaks])
        si = int(vals.argmax())
        margins["gap1"] = min(peaks[si][2], *(vals[si] - vals[s] for s in range(S) if s != si)) if S > 1 else peaks[si][2]
        r, cc = peaks[si][1]
        d = np.array([r, cc], f32)
        disp = (np.fmod((d + c["half"]).astype(f32), c["out_sz"]).astype(f32) - c["half"]).astype(f32)        # atom.py:327
        tv = ((disp * c["ratio"]).astype(f32) * c["target_scale"]).astype(f32)
        tv = (tv * c["scale_factors"][si]).astype(f32)                                                         # atom.py:331
        return dict(flag=0, scale_ind=si, peak1=np.array([r, cc]), peak2=np.array([0, 0]), which=0, max1=float(m[si][r, cc]), max2=0.0,
                    tv=tv.astype(np.float64), map=m, map_first=m, margins=margins, branch="plain")

    # ---- localize_advanced (atom.py:341-406) ----
    if win is not None:
        first = roll(windowed(raw), defect)                    # windowed before (atom.py:316) or inside (:352) the method: the same map
        orig = roll(raw, defect)
    else:
        first, orig = roll(raw, defect), None
    search = roll(raw, defect) if (defect == "window_after_argmax" and win is not None) else first
    peaks = [max2d(search[s]) for s in range(S)]
    vals = np.array([p[0] for p in peaks])
    si = int(vals.argmax())
    margins["gap1"] = min([peaks[si][2]] + [vals[si] - vals[s] for s in range(S) if s != si])
    p1 = peaks[si][1]
    max1 = float(first[si][p1])
    centre = c["center"]

    def tvec(p):
        d = (np.array(p, f32) - centre).astype(f32)
        return ((d * c["ratio"]).astype(f32) * c["target_scale"]).astype(f32), d

    tv1, d1 = tvec(p1)
    out = dict(scale_ind=si, peak1=np.array(p1), peak2=np.array([0, 0]), max1=max1, max2=0.0, which=0, map=first, map_first=first, margins=margins)
    margins["not_found"] = abs(max1 - case["target_not_found_threshold"])
    if max1 < case["target_not_found_threshold"]:
        return dict(out, flag=3, tv=tv1.astype(np.float64), branch="not_found")
    second = orig if hn else first                              # atom.py:369-370
    nr, nc = float(c["neigh"][0]), float(c["neigh"][1])
    args = (p1[0] - nr / 2, p1[0] + nr / 2 + 1, p1[1] - nc / 2, p1[1] + nc / 2 + 1)
    for name, x in zip(("top", "bottom", "left", "right"), args):
        if name not in case.get("on_half", ()):
            margins["round_" + name] = _half_distance(x)
    top, bottom = max(_round(args[0], defect), 0), min(_round(args[1], defect), Gh)
    left, right = max(_round(args[2], defect), 0), min(_round(args[3], defect), Gw)
    masked = second[si].copy()
    masked[top:bottom, left:right] = -np.inf if defect == "mask_neg_inf" else 0.0
    max2, p2, gap2 = max2d(masked)
    outside = second[si].copy()
    outside[top:bottom, left:right] = -np.inf
    if defect != "mask_neg_inf" and bottom > top and right > left and outside.max() < 0:
        # every cell outside the neighbourhood is negative: the winner is the first of the mask's exact zeros (ties that rounding cannot
        # move); what a rounding error would have to cross is the distance of the largest outside value from 0
        gap2 = float(-outside.max())
    margins["gap2"] = gap2
    tv2, d2 = tvec(p2)
    out.update(peak2=np.array(p2), max2=max2, which=1 if hn else 0, map=second, mask=(top, bottom, left, right))
    th_d, th_h = float(f32(case["distractor_threshold"])), float(f32(case["hard_negative_threshold"]))
    margins["distractor"] = abs(max2 - th_d * max1)
    if max2 > th_d * max1:
        n1 = float(np.sqrt((d1 * d1).astype(f32).sum(dtype=f32)))
        n2 = float(np.sqrt((d2 * d2).astype(f32).sum(dtype=f32)))
        th = float(c["disp_threshold"])
        margins["disp1"], margins["disp2"] = abs(n1 - th), abs(n2 - th)
        if n2 > th and n1 < th:
            return dict(out, flag=1, tv=tv1.astype(np.float64), branch="hn_first")
        if n2 < th and n1 > th:
            return dict(out, flag=1, tv=tv2.astype(np.float64), branch="hn_second")
        return dict(out, flag=2, tv=tv1.astype(np.float64), branch="uncertain_far" if (n2 > th and n1 > th) else "uncertain_near")
    margins["hard_negative"] = abs(max2 - th_h * max1)
    margins["hard_negative_floor"] = abs(max2 - float(f32(case["target_not_found_threshold"])))
    if max2 > th_h * max1 and max2 > float(f32(case["target_not_found_threshold"])):
        return dict(out, flag=1, tv=tv1.astype(np.float64), branch="hn_weak")
    return dict(out, flag=0, tv=tv1.astype(np.float64), branch="normal")


def floats(out):
    """the float outputs as arrays, for tests/f64_bound.py"""
    return OrderedDict((k, np.atleast_1d(np.asarray(out[k], np.float64))) for k in FLOAT_OUTPUTS)
