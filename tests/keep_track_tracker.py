"""The unmodified reference KeepTrack tracker (pytracking/tracker/keep_track/keep_track.py) on a stubbed backbone, for the closed-loop
comparison of tests/test_gpu_keep_track_tracker.py.  The DiMP-simple network is the one of tests/dimp_simple_tracker.py (random-init
`dimpnet50_simple`, backbone_pretrained=False, hot-path weights seeded); the target-candidate matching network is the reference's
`TargetCandidateMatchingNetwork` around a `DescriptorExtractor(1024, 256, 4)` and a `SuperGlue` with KeepTrack's conf
(target_candidate_matching_net_resnet50), both seeded from pytracking_amd.synth; its backbone is the same stub (KeepTrack hands the
tracker's own backbone features to it, keep_track.py:440).  Boundary calls are recorded event by event, the candidate extraction and
the matcher included.  The CPU run without install() is tests/golden/tracker_keep_track.npz (tools/make_golden_keep_track.py)."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import tracker_harness as TH  # noqa: E402
import dimp_simple_tracker as DST  # noqa: E402
import tracker_replay as TR  # noqa: E402
from pytracking_amd import synth  # noqa: E402

DIMS = dict(DST.DIMS, base_seed=61)
FRAME_HW = DST.FRAME_HW
RUN = dict(seed=6100, n_frames=8, dims=DIMS, thresholds=dict(target_not_found_threshold=0.05, hard_negative_threshold=0.75,
                                                              local_max_candidate_score_th=0.02))
# every rebound symbol a whole keep_track frame goes through (sample_patch* are reached with host images: their binding is asserted)
EXPECT_FAST = DST.EXPECT_FAST[:4] + ("KeepTrack.localize_advanced", "KeepTrack.optimize_boxes_relative", "find_local_maxima",
                                     "DescriptorExtractor.get_descriptors", "SuperGlue._forward")


def build_tcm_net(seed):
    """The reference TargetCandidateMatchingNetwork with KeepTrack's matcher conf, descriptor conv and matcher seeded."""
    TH.ref_harness.install()
    from ltr.models.target_candidate_matching.target_candidate_matching import (DescriptorExtractor,
                                                                               TargetCandidateMatchingNetwork)
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    torch.manual_seed(seed)
    ext = DescriptorExtractor(backbone_feat_dim=1024, descriptor_dim=256, kernel_size=4)
    w, b = synth.tcm_desc_conv(seed)
    ext.conv.weight.data.copy_(torch.from_numpy(w))
    ext.conv.bias.data.copy_(torch.from_numpy(b))
    matcher = SuperGlue({'skip_gnn': False, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': 10,
                         'output_normalization': 'sinkhorn'})
    matcher.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.tcm_superglue_state(seed + 1).items()})
    net = TargetCandidateMatchingNetwork(feature_extractor=torch.nn.Identity(), classification_layer=['layer3'],
                                         descriptor_extractor=ext, matcher=matcher)
    return net.eval()


def params(net_stub, tcm_stub):
    """pytracking/parameter/keep_track/default_fast.py's KeepTrack settings on the DiMP-simple set of tests/dimp_simple_tracker.py."""
    p = DST.params(net_stub)
    p.use_certainty_for_weight_computation = True
    p.certainty_for_weight_computation_ths = 0.5
    p.local_max_candidate_score_th = 0.1
    p.target_candidate_matching_net = tcm_stub
    p.visualize_candidate_matching = False
    p.visualize_candidate_assignment_matrix = False
    return p


def run(seed, n_frames, dims, thresholds=None, device="cpu", rec_events=True, times=None):
    """initialize() + n_frames x track(); returns (boxes, Recorder, tracker).  `times`: a list that receives the wall time of every
    track() call in seconds (device synchronised before and after; tools/bench_keep_track.py)."""
    TH.ref_harness.install()
    from pytracking.tracker.keep_track.keep_track import KeepTrack
    net = DST.build_dimp_simple(seed, dims).to(device)
    stub = TH.StubBackbone(seed, dims, device)
    tcm = TH.NetStub(build_tcm_net(seed + 11).to(device), stub)
    prm = TH.use_device(params(TH.NetStub(net, stub), tcm), device)
    for k, v in (thresholds or {}).items():
        setattr(prm, k, v)
    tracker = KeepTrack(prm)
    tracker.visdom = None
    rec = TH.Recorder()
    net.bb_regressor.get_iou_feat = lambda feats: stub.iou_feat(feats[0].shape[0])
    rec.add("config", seed=seed, n_frames=n_frames, **{f"dim_{k}": v for k, v in dims.items()})
    if rec_events:
        _instrument(tracker, net, rec)
    rng = np.random.default_rng(seed + 77)
    torch.manual_seed(seed)
    outs = []
    tracker.initialize(TH.synthetic_frame(rng, FRAME_HW), {"init_bbox": [445.0, 315.0, 70.0, 90.0]})
    frames = [TH.synthetic_frame(rng, FRAME_HW) for _ in range(n_frames)]
    for im in frames:
        rec.add("frame", frame=tracker.frame_num + 1)
        if times is not None:
            if torch.device(device).type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
        out = tracker.track(im)
        if times is not None:
            if torch.device(device).type == "cuda":
                torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        outs.append(np.array(out["target_bbox"], dtype=np.float64))
        rec.add("state", target_bbox=outs[-1], flag=str(tracker.debug_info.get("flag", "")))
    return np.stack(outs), rec, tracker


def _instrument(tracker, net, rec):
    orig_cls = tracker.classify_target

    def classify(x):
        s = orig_cls(x)
        rec.add("classify", scores=s)
        return s
    tracker.classify_target = classify
    opt = net.classifier.filter_optimizer
    orig_fwd = opt.forward

    def opt_forward(weights, *a, **kw):
        out = orig_fwd(weights, *a, **kw)
        if kw.get("sample_weight") is not None:
            rec.add("optimize", num_iter=kw["num_iter"], n=kw["feat"].shape[0], filter=out[0][0])
        return out
    opt.forward = opt_forward
    orig_loc = tracker.localize_advanced

    def localize(scores, sample_pos, sample_scales):
        tv, scale_ind, s, flag = orig_loc(scores, sample_pos, sample_scales)
        rec.add("localize", tv=tv, scale_ind=int(scale_ind), flag=flag)
        return tv, scale_ind, s, flag
    tracker.localize_advanced = localize
    orig_ref = tracker.optimize_boxes_relative

    def refine(iou_features, init_boxes):
        b, iou = orig_ref(iou_features, init_boxes)
        rec.add("refine", init_boxes=init_boxes, boxes=b, iou=iou)
        return b, iou
    tracker.optimize_boxes_relative = refine
    orig_cand = tracker.extract_descriptors_and_keypoints

    def candidates(backbone_feat, score_map, search_area_box):
        c = orig_cand(backbone_feat, score_map, search_area_box)
        rec.add("candidates", tsm_coords=c["tsm_coords"], scores=c["scores"], descriptors=c["descriptors"],
                img_coords=c["img_coords"])
        return c
    tracker.extract_descriptors_and_keypoints = candidates
    orig_match = tracker.extract_matches

    def matches(**kw):
        p = orig_match(**kw)
        rec.add("match", m=int(kw["scores0"].shape[0]), n=int(kw["scores1"].shape[0]), log_assignment=p["log_assignment"],
                matches0=p["matches0"], matches1=p["matches1"], match_scores0=p["match_scores0"], match_scores1=p["match_scores1"])
        return p
    tracker.extract_matches = matches


def run_installed(device="cuda"):
    """The same run on the device through pytracking_amd.install(); returns (events, install.stats)."""
    TH.ref_harness.install()
    from pytracking_amd import install as amd
    amd.install()
    amd.stats.clear()
    try:
        _, rec, _ = run(device=device, **RUN)
        stats = dict(amd.stats)
    finally:
        amd.uninstall()
    return TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()}), stats
