"""Cases of KeepTrack's target-candidate matching (tcm.hip behind pytracking_amd.candidate_matching) off the shapes of the two deployed
configurations, shared by tests/test_keep_track_cpu.py and tests/test_gpu_keep_track_f64.py: peak maps that need several compaction passes
of k_tcm_peaks, more than 1024 hits, non-square maps, other window sizes, ties and non-finite values; descriptor gathers with B > 1, H != W,
point counts around the 16-point pass and both coordinate forms; matcher runs with unequal image sizes, other layer lists, zero and one
Sinkhorn iteration and token counts around the 16-token tile of k_tcm_linear.

The anchor of every case is the float64 restatement tests/tcm_np.py (`want`).  ref_err is that of tests/f64_bound.py: the same
operation in fp32 on the CPU (torch.nn.functional.conv2d read at the points; the reference's own SuperGlue), pinned to f64_bound.THREADS
threads, ref_err = max |fp32 - float64| over the descriptor tensor / over log_assignment; a device output is held to f64_bound.bound(ref_err).
Reads nothing outside the repository (the matcher's ref_err needs the reference through oracle.ref_harness).  Test infrastructure only."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

import f64_bound
import tcm_np
from pytracking_amd import synth

# ---------------------------------------------------------------------------------------------------------------------------
# peaks: name -> (H, W, ks, th, how the map is made, seed).  k_tcm_peaks compacts the hits 1024 raster positions per pass.
PEAK_CASES = OrderedDict([
    ("33x33", (33, 33, 5, 0.1, "uniform", 2101)),              # two passes, 65 positions in the second: `base` is carried once
    ("64x64", (64, 64, 5, 0.1, "uniform", 2102)),              # four passes
    ("64x64_ks1", (64, 64, 1, 0.1, "uniform", 2103)),          # every score above th is a hit: n > 1024 in the rank loop
    ("64x64_ks127", (64, 64, 127, 0.1, "two_maxima", 2104)),   # the window is the map: the global maximum, planted twice
    ("9x64", (9, 64, 3, 0.1, "uniform", 2105)),
    ("64x9", (64, 9, 3, 0.1, "uniform", 2106)),
    ("1x1", (1, 1, 5, 0.1, "uniform_high", 2107)),
    ("1x64", (1, 64, 5, 0.1, "uniform", 2108)),
    ("40x50_eighths", (40, 50, 3, 0.1, "eighths", 2109)),      # multiples of 1/8: exact ties and plateaus
    ("23x23_nonfinite", (23, 23, 5, 0.1, "nonfinite", 2110)),  # one NaN, one +inf, one -inf
    ("40x50_batch3", (40, 50, 5, 0.1, "batch3", 2111)),        # (3, 1, 40, 50): the 4-D form
])
TWO_MAXIMA = ((10, 40), (50, 3))                               # ascending raster order
NONFINITE = {"nan": (4, 4), "+inf": (11, 17), "-inf": (18, 6)}


def _bumps(rng, H, W):
    """A score-map-like field: a few Gaussian bumps over small noise."""
    y, x = np.mgrid[0:H, 0:W]
    m = rng.uniform(0, 0.05, (H, W))
    for _ in range(6):
        cy, cx, a, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.15, 1.0), rng.uniform(1.0, 3.0)
        m += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return m.astype(np.float32)


def peak_map(name):
    """The float32 score map of a peak case: (H, W), or (3, 1, H, W) for the batch."""
    H, W, _, _, how, seed = PEAK_CASES[name]
    rng = np.random.default_rng(seed)
    if how == "uniform":
        return rng.uniform(0, 1, (H, W)).astype(np.float32)
    if how == "uniform_high":
        return rng.uniform(0.5, 1, (H, W)).astype(np.float32)
    if how == "two_maxima":
        m = rng.uniform(0, 1, (H, W)).astype(np.float32)
        for y, x in TWO_MAXIMA:
            m[y, x] = np.float32(2.0)
        return m
    if how == "eighths":
        return (np.round(rng.uniform(0, 1, (H, W)) * 8) / 8).astype(np.float32)
    if how == "nonfinite":
        m = _bumps(rng, H, W)
        m[NONFINITE["nan"]], m[NONFINITE["+inf"]], m[NONFINITE["-inf"]] = np.nan, np.inf, -np.inf
        return m
    assert how == "batch3"
    return np.stack([_bumps(rng, H, W) for _ in range(3)])[:, None]


def peak_want(name):
    """[(coords (P, 2) int64, values (P,) float32)] per map of the case, from the float64 anchor."""
    _, _, ks, th, _, _ = PEAK_CASES[name]
    m = peak_map(name)
    maps = [m] if m.ndim == 2 else [m[b, 0] for b in range(m.shape[0])]
    out = []
    for s in maps:
        c, v = tcm_np.find_local_maxima(s, th, ks)
        out.append((c, v.astype(np.float32)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# descriptors: name -> (B, C, H, W, D, P, coordinate form, seed).  k_tcm_desc takes 16 points per pass and 16 channels per K slice.
# "shared": one (P, 2) int64 tensor for every image; "per_image": (B, P, 2) int64, different per image; "int32": (P, 2) int32.
DESC_CASES = OrderedDict([
    ("p16", (1, 48, 22, 22, 64, 16, "shared", 2201)),          # exactly one pass
    ("p17", (1, 64, 22, 22, 128, 17, "shared", 2202)),         # one point past a pass
    ("p32", (1, 48, 22, 22, 128, 32, "shared", 2203)),         # exactly two passes
    ("p33", (1, 64, 22, 22, 64, 33, "shared", 2204)),
    ("h9_w30", (1, 48, 9, 30, 64, 17, "shared", 2205)),
    ("h30_w9", (1, 48, 30, 9, 64, 17, "shared", 2206)),
    ("b2_per_image", (2, 48, 13, 17, 64, 17, "per_image", 2207)),   # the second image's points start inside the second pass
    ("b3_shared", (3, 64, 12, 10, 128, 20, "shared", 2208)),
    ("int32", (1, 48, 22, 22, 64, 7, "int32", 2209)),
    ("c16", (1, 16, 22, 22, 64, 33, "shared", 2210)),          # a single K slice
])
DescInputs = namedtuple("DescInputs", "x weight bias coords coords3")   # coords as the caller passes them; coords3 (B, P, 2) int64
_CACHE = {}


def desc_inputs(name):
    B, C, H, W, D, P, form, seed = DESC_CASES[name]
    x = synth.tcm_layer3(seed, B, C, H, W)
    w, b = synth.tcm_desc_conv(seed + 1, D, C)
    rng = np.random.default_rng(seed + 2)
    corners = np.array([[0, 0], [0, W], [H, 0], [H, W]], np.int64)     # of the (H + 1) x (W + 1) output map

    def points(order):
        inner = np.stack([rng.integers(0, H + 1, P), rng.integers(0, W + 1, P)], 1).astype(np.int64)
        return np.concatenate([corners[order], inner])[:P] if P > 4 else inner
    if form == "per_image":
        coords = np.stack([points(np.roll(np.arange(4), k)) for k in range(B)])
        assert all(not np.array_equal(coords[0], coords[k]) for k in range(1, B))
        return DescInputs(x, w, b, coords, coords)
    coords = points(np.arange(4))
    coords3 = np.broadcast_to(coords[None], (B, P, 2)).copy()
    return DescInputs(x, w, b, coords.astype(np.int32) if form == "int32" else coords, coords3)


def conv2d_at_points(x, weight, bias, coords3, dtype):
    """torch.nn.functional.conv2d(padding=2) in `dtype` on the CPU, read at the points -> (B, D, P) numpy."""
    with torch.no_grad():
        full = torch.nn.functional.conv2d(torch.from_numpy(x).to(dtype), torch.from_numpy(weight).to(dtype),
                                          torch.from_numpy(bias).to(dtype), padding=2)
    c = torch.from_numpy(coords3)
    return torch.stack([full[b][:, c[b, :, 0], c[b, :, 1]] for b in range(full.shape[0])]).numpy()


def desc_anchor(name):
    """Anchor (tests/f64_bound.py) with want (B, D, P) float64 read-only, once per session."""
    def run(dtype):
        i = desc_inputs(name)
        if dtype == np.float32:
            return OrderedDict(desc=conv2d_at_points(i.x, i.weight, i.bias, i.coords3, torch.float32))
        return OrderedDict(desc=tcm_np.get_descriptors(i.x, i.weight, i.bias, i.coords3))
    a = f64_bound.anchor(("tcm_desc", name), run, threads=f64_bound.THREADS)
    return a._replace(want=a.want["desc"])


# ---------------------------------------------------------------------------------------------------------------------------
# matcher: (name, M, N, layers, iters, image_size0, image_size1, seed).  Weights synth.tcm_superglue_state(seed, len(layers)); data
# synth.tcm_match_inputs(seed, M, N, image_size0) with img_coords1 of synth.tcm_match_inputs(seed + 1000, M, N, image_size1).  Every
# seed was chosen so that the smallest margin of tcm_np.margins exceeds 1e-3 in float64 (tests/test_keep_track_cpu.py asserts it): the
# discrete outputs are compared exactly.
SC2 = ("self", "cross") * 2
VGA = (480, 640)
MATCH_CASES = [
    ("1x1", 1, 1, SC2, 10, VGA, VGA, 950),
    ("64x1", 64, 1, SC2, 10, VGA, VGA, 961),                   # tcm_wave_lse: rows of two operands, a column that uses lane + 64
    ("1x64", 1, 64, SC2, 10, VGA, VGA, 972),
    ("16x1", 16, 1, SC2, 10, VGA, VGA, 981),                   # T = 17: one token in the second tile, the side split at the tile's edge
    ("15x2", 15, 2, SC2, 10, VGA, VGA, 991),                   # T = 17: the side split inside the first tile
    ("16x16", 16, 16, SC2, 10, VGA, VGA, 1002),
    ("33x16", 33, 16, SC2, 10, VGA, VGA, 1013),                # T = 49
    ("5x64", 5, 64, SC2, 10, VGA, VGA, 1022),
    ("sizes", 9, 12, SC2, 10, (352, 640), (720, 400), 1031),   # per-side centre and scale in k_tcm_kenc
    ("it0", 7, 10, SC2, 0, VGA, VGA, 1041),
    ("it1", 7, 10, SC2, 1, VGA, VGA, 1051),
    ("cross1", 6, 11, ("cross",), 10, VGA, VGA, 1060),         # layer mask 0b1
    ("ssc", 6, 11, ("self", "self", "cross"), 10, VGA, VGA, 1071),                       # 0b100
    ("css5", 6, 11, ("cross", "self", "self", "cross", "cross"), 10, VGA, VGA, 1081),    # 0b11001
]
MATCH = OrderedDict((c[0], c) for c in MATCH_CASES)
MATCH_OUTPUTS = ("log_assignment", "matches0", "matches1", "match_scores0", "match_scores1")


def match_inputs(name):
    """(state (numpy), layers, iters, data (numpy, with image_size0 / image_size1)) of a matcher case."""
    _, M, N, layers, iters, size0, size1, seed = MATCH[name]
    data = synth.tcm_match_inputs(seed, M, N, size0)
    data["img_coords1"] = synth.tcm_match_inputs(seed + 1000, M, N, size1)["img_coords1"]
    data["image_size0"], data["image_size1"] = tuple(size0), tuple(size1)
    return synth.tcm_superglue_state(seed, len(layers)), list(layers), iters, data


def match_want(name):
    """The float64 anchor's outputs {name: numpy, read-only}, once per session.  Needs no reference."""
    if ("match", name) not in _CACHE:
        sd, layers, iters, data = match_inputs(name)
        want = OrderedDict(zip(MATCH_OUTPUTS, tcm_np.match(sd, layers, iters, data)))
        for v in want.values():
            v.setflags(write=False)
        _CACHE[("match", name)] = want
    return _CACHE[("match", name)]


def superglue(name, dtype=torch.float32, device="cpu"):
    """The reference's SuperGlue with the case's conf and state (oracle.ref_harness must be available)."""
    from oracle import ref_harness
    ref_harness.install()
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    sd, layers, iters, _ = match_inputs(name)
    sg = SuperGlue({'skip_gnn': False, 'GNN_layers': layers, 'num_sinkhorn_iterations': iters, 'output_normalization': 'sinkhorn'})
    sg.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return sg.to(device=device, dtype=dtype).eval()


def match_data(name, dtype=torch.float32, device="cpu"):
    """The data dict as KeepTrack passes it: tensors on `device`, the image sizes as tuples."""
    data = match_inputs(name)[3]
    return {k: v if isinstance(v, tuple) else torch.from_numpy(v.copy()).to(device=device, dtype=dtype) for k, v in data.items()}


def reference_match(name, dtype):
    """The reference's own SuperGlue on the CPU in `dtype` -> {output: numpy} without the batch dimension."""
    with torch.no_grad():
        pred = superglue(name, dtype)(match_data(name, dtype))
    return OrderedDict((k, pred[k][0].numpy()) for k in MATCH_OUTPUTS)


def match_anchor(name):
    """Anchor (tests/f64_bound.py) with want = match_want(name) and ref_err = max |reference fp32 log_assignment - float64|, once per
    session.  Needs the reference."""
    def run(dtype):
        out = match_want(name) if dtype == np.float64 else reference_match(name, torch.float32)
        return OrderedDict(log_assignment=out["log_assignment"])
    return f64_bound.anchor(("tcm_match", name), run, threads=f64_bound.THREADS)._replace(want=match_want(name))
