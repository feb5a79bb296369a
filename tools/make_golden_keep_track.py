"""TEST INFRASTRUCTURE ONLY -- tests/golden/tcm_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_keep_track.py
KeepTrack's target-candidate matching (pytracking/tracker/keep_track/keep_track.py:437-475):
  tcm_peaks_*   ltr.data.processing_utils.find_local_maxima (ks=5 as KeepTrack calls it; 2-D maps and one 4-D batch)
  tcm_desc_*    DescriptorExtractor(1024, 256, 4).get_descriptors at the default_fast (22x22) and default (30x30) sizes; the layer3
                map and the conv come from pytracking_amd.synth (seed + shape stored, not the 4-16 MB arrays)
  tcm_match_*   SuperGlue with KeepTrack's conf (target_candidate_matching_net_resnet50), state from synth.tcm_superglue_state
                (BatchNorm statistics away from their defaults), eval mode, fed the data dict of KeepTrack.extract_matches
  tracker_keep_track  the unmodified KeepTrack, closed loop on the stub backbone (tests/keep_track_tracker.py), CPU, without install()
Every discrete matcher output is stored with its margins (row / column runner-up gap, distance to filter_threshold).
    python -B tools/make_golden_keep_track.py [peaks] [descriptors] [matches] [tracker]      (default: all)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

from pytracking_amd import synth  # noqa: E402
import tcm_np  # noqa: E402

OUT = os.environ.get("TCM_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
T = torch.from_numpy
TH = 0.1          # parameter/keep_track/default_fast.py: local_max_candidate_score_th
IMAGE_SHAPE = (480, 640)

MATCH_CASES = {   # name: (seed, M, N, skip_gnn, sinkhorn iterations)
    "tcm_match_1x2": (901, 1, 2, False, 10),
    "tcm_match_2x1": (902, 2, 1, False, 10),
    "tcm_match_3x5": (903, 3, 5, False, 10),
    "tcm_match_8x8": (904, 8, 8, False, 10),
    "tcm_match_17x31": (905, 17, 31, False, 10),
    "tcm_match_64x64": (906, 64, 64, False, 10),
    "tcm_match_skip_gnn": (907, 6, 9, True, 10),
    "tcm_match_it50": (908, 8, 8, False, 50),
}
DESC_CASES = {    # name: (seed, H, W, P)
    "tcm_desc_fast_p1": (801, 22, 22, 1),
    "tcm_desc_fast_p7": (802, 22, 22, 7),
    "tcm_desc_fast_p40": (803, 22, 22, 40),
    "tcm_desc_default_p1": (806, 30, 30, 1),
    "tcm_desc_default_p7": (804, 30, 30, 7),
    "tcm_desc_default_p40": (805, 30, 30, 40),
}


def conf(skip_gnn, iters):
    return {'skip_gnn': skip_gnn, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': iters,
            'output_normalization': 'sinkhorn'}


def superglue(seed, skip_gnn, iters):
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    torch.manual_seed(seed)
    sg = SuperGlue(conf(skip_gnn, iters))
    sd = synth.tcm_superglue_state(seed, 4, skip_gnn)
    sg.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    return sg.eval(), sd


def smooth_map(rng, H, W):
    """A score-map-like field: a few Gaussian bumps plus small noise, all values distinct."""
    y, x = np.mgrid[0:H, 0:W]
    m = rng.uniform(0, 0.05, (H, W))
    for _ in range(6):
        cy, cx, a, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.05, 1.0), rng.uniform(1.0, 3.0)
        m += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return m.astype(np.float32)


def peaks():
    import ltr.data.processing_utils as prutils
    rng = np.random.default_rng(1001)
    cases = {"tcm_peaks_23": smooth_map(rng, 23, 23), "tcm_peaks_31": smooth_map(rng, 31, 31),
             "tcm_peaks_noise": rng.uniform(0, 1, (23, 23)).astype(np.float32)}
    # threshold boundary: isolated peaks at exactly float32(TH) (not > th) and at the next float above it
    b = np.zeros((23, 23), np.float32)
    b[3, 3] = np.float32(TH)
    b[10, 10] = np.nextafter(np.float32(TH), np.float32(1))
    b[18, 5] = np.float32(0.5)
    b[5, 18] = np.float32(TH) - np.float32(1e-3)
    cases["tcm_peaks_boundary"] = b
    # plateau: a 2x2 block of equal maxima (every element is a peak; the order of ties is not compared)
    p = smooth_map(rng, 23, 23) * np.float32(0.5)
    p[11:13, 7:9] = np.float32(0.9)
    cases["tcm_peaks_plateau"] = p
    for name, m in cases.items():
        c, v = prutils.find_local_maxima(T(m), th=TH, ks=5)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), scores=m, th=np.float64(TH), ks=np.int64(5), coords=c.numpy(),
                            values=v.numpy())
    maps = np.stack([smooth_map(rng, 23, 23) for _ in range(3)])[:, None]
    cs, vs = prutils.find_local_maxima(T(maps), th=TH, ks=5)
    np.savez_compressed(os.path.join(OUT, "tcm_peaks_batch.npz"), scores=maps, th=np.float64(TH), ks=np.int64(5),
                        counts=np.array([len(c) for c in cs], np.int64), coords=np.concatenate([c.numpy() for c in cs]),
                        values=np.concatenate([v.numpy() for v in vs]))


def descriptors():
    from ltr.models.target_candidate_matching.target_candidate_matching import DescriptorExtractor
    for name, (seed, H, W, P) in DESC_CASES.items():
        rng = np.random.default_rng(seed)
        x = synth.tcm_layer3(seed, 1, 1024, H, W)
        w, b = synth.tcm_desc_conv(seed + 1)
        edge = np.array([[0, 0], [H, W], [0, W], [H, 0], [0, W // 2], [H // 2, 0]], np.int64)
        inner = np.stack([rng.integers(0, H + 1, P), rng.integers(0, W + 1, P)], 1)
        coords = np.concatenate([edge, inner])[:P] if P > 1 else inner[:1]
        ext = DescriptorExtractor(1024, 256, 4)
        ext.conv.weight.data.copy_(T(w))
        ext.conv.bias.data.copy_(T(b))
        with torch.no_grad():
            out = ext.get_descriptors(T(x), T(coords)).numpy()
        np.savez_compressed(os.path.join(OUT, name + ".npz"), seed=np.int64(seed), H=np.int64(H), W=np.int64(W), coords=coords,
                            desc=out)


def matches():
    for name, (seed, M, N, skip, iters) in MATCH_CASES.items():
        sg, sd = superglue(seed, skip, iters)
        inp = synth.tcm_match_inputs(seed + 1, M, N, IMAGE_SHAPE)
        data = {k: T(v.copy()) for k, v in inp.items()}
        data["image_size0"] = data["image_size1"] = torch.Size(IMAGE_SHAPE)
        with torch.no_grad():
            pred = sg(data)
        la = pred["log_assignment"][0].numpy()
        nd = dict(inp, image_size0=IMAGE_SHAPE, image_size1=IMAGE_SHAPE)
        Z, _, _, ms0, _ = tcm_np.match(sd, [] if skip else ['self', 'cross'] * 2, iters, nd)
        rows, cols, thr = tcm_np.margins(la.astype(np.float64), pred["match_scores0"][0].numpy().astype(np.float64))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), seed=np.int64(seed), M=np.int64(M), N=np.int64(N),
                            skip_gnn=np.int64(skip), iters=np.int64(iters), image_shape=np.array(IMAGE_SHAPE, np.int64),
                            **inp, log_assignment=la, matches0=pred["matches0"][0].numpy(), matches1=pred["matches1"][0].numpy(),
                            match_scores0=pred["match_scores0"][0].numpy(), match_scores1=pred["match_scores1"][0].numpy(),
                            margin_rows=np.float64(rows), margin_cols=np.float64(cols), margin_thr=np.float64(thr))
        print(name, "margins", rows, cols, thr, "max |Z - np|", float(np.abs(la - Z).max()))


def tracker():
    import keep_track_tracker as KT
    _, rec, _ = KT.run(device="cpu", **KT.RUN)
    multi = [e for e in rec.events if e["kind"] == "match" and max(e["m"], e["n"]) >= 2]
    assert len(multi) >= 3, f"the run must call the matcher on several frames with >= 2 candidates on a side: {len(multi)}"
    assert any(e["kind"] == "refine" for e in rec.events) and any(e["kind"] == "localize" for e in rec.events)
    path = os.path.join(OUT, "tracker_keep_track.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB), matcher on {len(multi)} frames")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    steps = dict(peaks=peaks, descriptors=descriptors, matches=matches, tracker=tracker)
    for name in sys.argv[1:] or list(steps):
        steps[name]()
