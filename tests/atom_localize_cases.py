"""Case table of ATOM's per-frame score localisation (pytracking/tracker/atom/atom.py:304-406; csrc_loc/atom_localize.hip): the smallest
shapes at which the kernel can still go wrong, plus the deployed one.

  series -> grid            kernel   what it is there for
  4 x 4   -> 9 x 9          (4, 4)   smallest series, odd grid: the roll by (sz + 1) // 2 against the displacement's sz // 2
  6 x 7   -> 24 x 28        (4, 4)   even and odd series side in one map, window on
  5 x 6   -> 40 x 24        (3, 3)   odd kernel (the 1 / sz phase term), `perform_hn_without_windowing`
  8 x 8   -> 32 x 48        (4, 3)   kernel parity mixed per axis; one case per outcome of atom.py:366-406, the neighbourhood clipped at each
                                     border, a neighbourhood bound on a half-integer
  18 x 18 -> 288 x 288      (4, 4)   the deployed size
  18 x 18 -> 576 x 576      (4, 4)   the largest grid
S = 1, 2, 3, 8 scales; the window off, on, and on with `perform_hn_without_windowing`; advanced localisation on and off.

Inputs are periodic Gaussian blobs plus seeded noise, generated here; the goldens (tests/golden/atom_localize_<case>.npz, written by
tools/make_golden_atom_localize.py from the unmodified reference) hold the reference's outputs and its own fp32 distance from its float64
run, `ref_fp32_err`.  Every discrete decision of every case keeps the margin tests/test_atom_localize_cpu.py asserts; a case that does not
is replaced here, never skipped.  bare_tracker() builds the object the reference method reads.  Test infrastructure only."""
import os
from collections import OrderedDict

import numpy as np

import atom_localize_np as RN

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F_MAX = 64            # the weakest seeded defect misses max(ref_err, ulp of max) by more than this (tests/test_atom_localize_cpu.py)
STORE_MAP64_CELLS = 48 * 48           # goldens keep the returned map of both runs for the small grids, and the fp32 map of `deployed`


def hann_window(G):
    """dcf.hann2d(sz, centered=False) (dcf.py:8-18) in float32"""
    def h1(sz):
        i = np.arange(sz)
        d = np.minimum(i, sz - i)
        return (0.5 * (1 + np.cos((2 * np.pi / (sz + 2)) * d.astype(np.float32)))).astype(np.float32)
    return (h1(G[0])[:, None] * h1(G[1])[None, :]).astype(np.float32)


def blob_scores(S, N, blobs, seed, noise=0.01, base=0.05):
    """(S, 1, N_h, N_w) float32: per scale `base` + noise, plus periodic Gaussians (scale, row, col, amplitude, sigma)"""
    rng = np.random.default_rng(seed)
    s = base + noise * rng.standard_normal((S, 1, N[0], N[1]))
    r, c = np.arange(N[0])[:, None], np.arange(N[1])[None, :]
    for sc, r0, c0, amp, sig in blobs:
        dr = np.minimum(np.abs(r - r0), N[0] - np.abs(r - r0))
        dc = np.minimum(np.abs(c - c0), N[1] - np.abs(c - c0))
        s[sc, 0] += amp * np.exp(-(dr ** 2 + dc ** 2) / (2 * sig ** 2))
    return s.astype(np.float32)


def _case(N, G, kernel, S, blobs, seed, window=None, hn=False, advanced=True, target_sz=(3.0, 3.0), target_scale=1.0, scale_factors=None,
          on_half=(), noise=0.01, base=0.05, **params):
    G = tuple(G)
    c = dict(scores=blob_scores(S, N, blobs, seed, noise, base), N=tuple(N), G=G, kernel=tuple(kernel), advanced=advanced,
             window=hann_window(G) if window else None, hn_without_windowing=hn, target_sz=target_sz, target_scale=target_scale,
             img_support_sz=(float(16 * N[0]), float(16 * N[1])),
             scale_factors=tuple(scale_factors) if scale_factors is not None else tuple(1.02 ** (k - S // 2) for k in range(S)),
             translation_weight=1.0, on_half=tuple(on_half),
             target_not_found_threshold=0.25, distractor_threshold=0.8, hard_negative_threshold=0.5, target_neighborhood_scale=2.2,
             dispalcement_scale=0.8)
    c.update(params)
    return c


# the 8 x 8 -> 32 x 48 family: the map centre is sample (4, 3.5); th = 0.8 sqrt(32 * 48) / 2 = 15.7 cells
_B = dict(N=(8, 8), G=(32, 48), kernel=(4, 3))
CASES = OrderedDict([
    ("n4_g9", _case((4, 4), (9, 9), (4, 4), 1, [(0, 1, 2, 1.0, 0.7)], 11, target_sz=(1.0, 1.0))),
    ("n4_g9_plain", _case((4, 4), (9, 9), (4, 4), 2, [(1, 3, 0, 1.0, 0.7), (0, 1, 1, 0.6, 0.7)], 12, advanced=False, window=True)),
    ("n6x7_g24x28_win", _case((6, 7), (24, 28), (4, 4), 2, [(0, 2, 4, 1.0, 0.8), (1, 3, 3, 0.7, 0.8)], 13, window=True, target_sz=(5.2, 6.1))),
    ("n6x7_g24x28_plain", _case((6, 7), (24, 28), (4, 4), 3, [(2, 5, 1, 0.9, 0.8), (0, 2, 2, 0.5, 0.8)], 14, advanced=False)),
    ("n5x6_k3_g40x24_hn", _case((5, 6), (40, 24), (3, 3), 3, [(1, 2, 3, 1.0, 0.8), (1, 4, 0, 0.9, 0.8), (2, 2, 2, 0.6, 0.8)], 15, window=True, hn=True,
                                target_sz=(4.0, 2.0))),
    ("b_not_found", _case(S=1, blobs=[(0, 4, 4, 0.12, 0.8)], seed=21, **_B)),
    ("b_normal", _case(S=2, blobs=[(1, 4, 4, 1.0, 0.8)], seed=22, target_sz=(8.0, 10.0), **_B)),
    ("b_hn_weak", _case(S=3, blobs=[(0, 4, 4, 1.0, 0.8), (0, 1, 1, 0.65, 0.8)], seed=23, target_sz=(8.0, 10.0), **_B)),
    ("b_hn_first", _case(S=8, blobs=[(5, 4, 4, 1.0, 0.8), (5, 0, 0, 0.92, 0.8)], seed=24, **_B)),
    ("b_hn_second_clip_br", _case(S=2, blobs=[(0, 7, 7, 1.0, 0.8), (0, 4, 3, 0.92, 0.8)], seed=25, target_sz=(4.0, 4.0), **_B)),
    ("b_uncertain_far_clip_tl", _case(S=3, blobs=[(2, 0, 0, 1.0, 0.8), (2, 7, 6, 0.92, 0.8)], seed=26, target_sz=(4.0, 4.0), **_B)),
    ("b_uncertain_near", _case(S=1, blobs=[(0, 4, 3, 1.0, 0.6), (0, 4, 5, 0.92, 0.6)], seed=27, target_sz=(2.0, 2.0), **_B)),
    # neighbourhood rows p - 3.5 and p + 4.5 with p even: half-to-even and half-away rounding mask different rows
    ("b_half_even", _case(S=1, blobs=[(0, 5, 4, 1.0, 1.2)], seed=28, target_sz=(3.5, 12.0), target_neighborhood_scale=2.0, on_half=("top", "bottom"),
                          noise=0.002, **_B)),
    # every cell outside the neighbourhood is negative: the second peak is one of the mask's zeros (ATOM zeroes, it does not use -inf)
    ("b_mask_zero", _case(S=1, blobs=[(0, 4, 4, 1.4, 0.8)], seed=29, target_sz=(8.0, 10.0), base=-0.3, **_B)),
    ("deployed", _case((18, 18), (288, 288), (4, 4), 1, [(0, 10, 8, 1.0, 1.2), (0, 4, 13, 0.55, 1.2)], 31, target_sz=(40.0, 33.0), target_scale=1.25)),
    ("deployed_s8_hn", _case((18, 18), (288, 288), (4, 4), 8, [(3, 9, 9, 1.0, 1.2), (3, 14, 3, 0.9, 1.2), (4, 9, 9, 0.95, 1.2)], 32, window=True, hn=True,
                             target_sz=(40.0, 33.0), target_scale=1.25)),
    ("n18_g576_plain", _case((18, 18), (576, 576), (4, 4), 2, [(1, 12, 5, 1.0, 1.2), (0, 12, 5, 0.9, 1.2)], 33, advanced=False, window=True,
                             img_support_sz=(288.0, 288.0))),
    ("n18_g576", _case((18, 18), (576, 576), (4, 4), 1, [(0, 7, 11, 1.0, 1.2)], 34, img_support_sz=(288.0, 288.0), target_sz=(80.0, 80.0))),
])
for _c in CASES.values():
    _c["scores"].setflags(write=False)

# what each case is in the table for (asserted by tests/test_atom_localize_cpu.py)
BRANCHES = {"n4_g9": "hn_weak", "n4_g9_plain": "plain", "n6x7_g24x28_win": "normal", "n6x7_g24x28_plain": "plain", "n5x6_k3_g40x24_hn": "hn_first",
            "b_not_found": "not_found", "b_normal": "normal", "b_hn_weak": "hn_weak", "b_hn_first": "hn_first", "b_hn_second_clip_br": "hn_second",
            "b_uncertain_far_clip_tl": "uncertain_far", "b_uncertain_near": "uncertain_near", "b_half_even": "hn_weak", "b_mask_zero": "normal", "deployed": "hn_weak",
            "deployed_s8_hn": "hn_first", "n18_g576_plain": "plain", "n18_g576": "normal"}

# (what, N_h, N_w, G_h, G_w, S): refused with "unsupported", nothing queued
REFUSALS = (("grid equal to the series", 18, 18, 19, 19, 1), ("grid smaller than the series", 18, 18, 16, 16, 1), ("one side equal", 8, 8, 32, 9, 1),
            ("series above 32", 33, 18, 288, 288, 1), ("series below 4", 3, 8, 32, 32, 1), ("grid above 576", 18, 18, 577, 288, 1),
            ("more than 8 scales", 18, 18, 288, 288, 9), ("no scale", 18, 18, 288, 288, 0))

_RUNS = {}


def run(name, defect=None):
    """the float64 restatement on a case of the table (cached without a defect)"""
    if defect is not None:
        return RN.localize(CASES[name], defect)
    if name not in _RUNS:
        _RUNS[name] = RN.localize(CASES[name])
    return _RUNS[name]


def golden(name):
    with np.load(os.path.join(GOLDEN_DIR, f"atom_localize_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def ref_errs(name):
    """{output: the unmodified reference's fp32 distance from its own float64 run} of the golden"""
    g = golden(name)
    return OrderedDict((k, float(g["ref_fp32_err"][i])) for i, k in enumerate(RN.FLOAT_OUTPUTS))


def bare_tracker(case, device="cpu", dtype=None):
    """An `ATOM` object (ATOM.__new__, attributes set by hand) holding exactly what `localize_target` / `localize_advanced` read.  dtype:
    torch.float64 for the reference's float64 run (the caller also sets torch's default dtype, which `torch.Tensor(...)` follows)."""
    import torch
    from pytracking import TensorList
    from pytracking.tracker.atom.atom import ATOM
    from pytracking.utils import TrackerParams
    dtype = dtype or torch.float32
    t = ATOM.__new__(ATOM)
    p = TrackerParams()
    p.debug, p.device = 0, device
    p.advanced_localization = bool(case["advanced"])
    p.perform_hn_without_windowing = bool(case["hn_without_windowing"])
    for k in ("target_not_found_threshold", "distractor_threshold", "hard_negative_threshold", "target_neighborhood_scale", "dispalcement_scale"):
        setattr(p, k, case[k])
    p.scale_factors = torch.tensor(case["scale_factors"], dtype=dtype)
    t.params = p

    class _FParams:
        def attribute(self, name, *default):
            return TensorList([case.get(name, *default)])
    t.fparams = _FParams()
    t.feature_sz = TensorList([torch.tensor([float(v) for v in case["N"]], dtype=dtype)])
    t.kernel_size = TensorList([tuple(case["kernel"])])
    t.output_sz = torch.tensor([float(v) for v in case["G"]], dtype=dtype)
    t.img_support_sz = torch.tensor(case["img_support_sz"], dtype=dtype)
    t.target_sz = torch.tensor(case["target_sz"], dtype=dtype)
    t.target_scale = case["target_scale"]
    t.output_window = None if case["window"] is None else torch.from_numpy(case["window"].copy()).to(dtype)[None, None].to(device)
    return t


def state_block(case):
    """`pt_loc_atom_state` of a case, through the product's own builder"""
    from pytracking_amd import atom_localize as AL
    return AL.state_block(kernel_size=case["kernel"], output_sz=case["G"], img_support_sz=case["img_support_sz"], target_sz=case["target_sz"],
                          target_scale=case["target_scale"], translation_weight=case["translation_weight"], scale_factors=case["scale_factors"],
                          advanced_localization=case["advanced"], windowed=case["window"] is not None, hn_without_windowing=case["hn_without_windowing"],
                          **{k: case[k] for k in ("target_not_found_threshold", "distractor_threshold", "hard_negative_threshold",
                                                  "target_neighborhood_scale", "dispalcement_scale")})
