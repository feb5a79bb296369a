"""The unmodified reference KYS tracker (pytracking/tracker/kys/kys.py) on a stubbed backbone, for the closed-loop comparison of
tests/test_gpu_kys_tracker.py: a random-init `kysnet_res50` built by the reference's constructor with the arguments of the train setting
(ltr/train_settings/kys/kys.py:110-114: optim_iter=3, cv_kernel_size=3, cv_max_displacement=9, cv_stride=1,
init_gauss_sigma=output_sigma * feature_sz = 1/4 / 5 * 18 (:41-44, :111), train_feature_extractor=False, train_iounet=False, detach_length=0,
state_dim=8, representation_predictor_dims=(16,), conf_measure='entropy', dimp_thresh=0.05; the bundle on the GPU box does not carry
ltr/train_settings, so they are restated here; backbone_pretrained=False, nothing is downloaded), its DiMP classifier and IoU head seeded
like the DiMP run of oracle/tracker_harness.py, its response predictor from synth.kys_predictor_state, boundary calls recorded event by event.
Motion features are the stub's `layer3` (PredictorWrapper.extract_motion_feat is a reshape).  The CPU run without install(), with the
plain-torch stand-in sampler of tests/kys_standin.py, is tests/golden/tracker_kys.npz (tools/make_golden_kys.py tracker)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import tracker_harness as TH  # noqa: E402
from pytracking_amd import synth  # noqa: E402
import tracker_replay as TR  # noqa: E402

DIMS = dict(TH.DIMP50_TEST, base_seed=61)            # 18 x 18 maps from 288 x 288 samples; layer3 (1024 channels) is the motion feature
RUN = dict(seed=6100, n_frames=6, dims=DIMS)
PREDICTOR_SEED = 6150
# every rebound symbol a whole KYS frame goes through, as install.stats names them
EXPECT_FAST = ("PredictorWrapper.predict_response", "apply_filter", "DiMPSteepestDescentGN", "residual_bottleneck", "PrRoIPool2D")


def build_kysnet(seed, dims=DIMS):
    TH.ref_harness.install()
    from ltr.models.tracking.kysnet import kysnet_res50
    torch.manual_seed(seed)
    net = kysnet_res50(backbone_pretrained=False, optim_iter=3, cv_kernel_size=3, cv_max_displacement=9, cv_stride=1, init_gauss_sigma=0.9,
                       state_dim=8, representation_predictor_dims=(16,), conf_measure='entropy', dimp_thresh=0.05,
                       train_feature_extractor=False, train_iounet=False, detach_length=0)
    net.eval()
    TH.seed_dimp_net(types.SimpleNamespace(classifier=net.dimp_classifier, bb_regressor=net.bb_regressor), seed, dims)
    sd = synth.kys_predictor_state(PREDICTOR_SEED, "entropy", rep_dims=(16,))
    net.predictor.predictor.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return net


def params(net_stub):
    """pytracking/parameter/kys/default.py on the shortened-cadence set of the harness (train_skipping 20 -> 2; the `rotate` and `dropout`
    augmentations dropped as there: OpenCV / torch's global RNG)."""
    p = TH.dimp50_params(net_stub)
    for k in ("net_opt_hn_iter", "advanced_localization", "target_not_found_threshold", "distractor_threshold", "hard_negative_threshold",
              "target_neighborhood_scale", "dispalcement_scale", "hard_negative_learning_rate"):       # DiMP's, not in kys/default.py
        delattr(p, k)
    p.output_sigma_factor = 1 / 4
    p.window_output = True
    p.use_clipped_window = True
    p.effective_search_area = 10.0
    p.apply_window_to_dimp_score = True
    p.dimp_threshold = 0.05
    p.target_not_found_threshold_fused = 0.05
    p.reset_state_during_occlusion = False
    p.prev_feat_remove_subpixel_shift = True
    p.move_feat_to_center = True
    p.use_iou_net = True
    p.remove_offset_in_fused_score = True
    p.score_downsample_factor = 1
    return p


def run(seed, n_frames, dims, thresholds=None, device="cpu"):
    """initialize() + n_frames x track(); returns (boxes, Recorder, (tracker, net))."""
    TH.ref_harness.install()
    from pytracking.tracker.kys.kys import KYS
    net = build_kysnet(seed, dims).to(device)
    stub = TH.StubBackbone(seed, dims, device)
    ns = TH.NetStub(net, stub)
    prm = TH.use_device(params(ns), device)
    for k, v in (thresholds or {}).items():
        setattr(prm, k, v)
    tracker = KYS(prm)
    tracker.visdom = None
    rec = TH.Recorder()
    net.bb_regressor.get_iou_feat = lambda feats: stub.iou_feat(feats[0].shape[0])      # stock convs: stubbed like the backbone
    rec.add("config", seed=seed, n_frames=n_frames, predictor_seed=PREDICTOR_SEED, **{f"dim_{k}": v for k, v in dims.items()})

    orig_head = tracker.get_classification_features

    def head(backbone_feat):
        out = orig_head(backbone_feat)
        rec.add("head", n=out.shape[0], checksum=float(out.double().abs().sum()))
        return out
    tracker.get_classification_features = head
    clf = net.dimp_classifier
    orig_get_filter = clf.get_filter

    def get_filter(feat, bb, *a, **kw):
        w, its, losses = orig_get_filter(feat, bb, *a, **kw)
        rec.add("get_filter", bb=bb, num_iter=kw.get("num_iter"), filter=w, n=feat.shape[0])
        return w, its, losses
    clf.get_filter = get_filter
    opt = clf.filter_optimizer
    orig_fwd = opt.forward

    def opt_forward(weights, *a, **kw):
        out = orig_fwd(weights, *a, **kw)
        if kw.get("sample_weight") is not None:                                  # update call (kys.py:738-742)
            rec.add("optimize", bb=kw["bb"], sw=kw["sample_weight"], num_iter=kw["num_iter"], n=kw["feat"].shape[0], filter=out[0])
        return out
    opt.forward = opt_forward
    orig_cls = tracker.classify_target

    def classify(x):
        s = orig_cls(x)
        rec.add("classify", scores=s)
        return s
    tracker.classify_target = classify
    wrapper = net.predictor
    orig_pr = wrapper.predict_response                                           # looked up on the class: install()'s dispatcher, if bound

    def predict_response(data, dimp_thresh=None, output_window=None):
        out = orig_pr(data, dimp_thresh=dimp_thresh, output_window=output_window)
        rec.add("predict_response", response=out["response"], state=out["state_cur"], with_state=int(data["state_prev"] is not None),
                conf=out["auxiliary_outputs"]["propagation_conf"])
        return out
    wrapper.predict_response = predict_response
    orig_loc = tracker.localize_target

    def localize(score_fused, score_dimp, sample_scales):
        tv, scale_ind, s, flag = orig_loc(score_fused, score_dimp, sample_scales)
        rec.add("localize", tv=tv, scale_ind=int(scale_ind), flag=flag)
        return tv, scale_ind, s, flag
    tracker.localize_target = localize
    orig_ref = tracker.optimize_boxes_default

    def refine(iou_features, init_boxes):
        b, iou = orig_ref(iou_features, init_boxes)
        rec.add("refine", init_boxes=init_boxes, boxes=b, iou=iou)
        return b, iou
    tracker.optimize_boxes_default = refine
    orig_mem = tracker.update_memory

    def update_memory(sample_x, target_box, learning_rate=None):
        orig_mem(sample_x, target_box, learning_rate)
        rec.add("memory", slot=int(tracker.previous_replace_ind[0]), stored=int(tracker.num_stored_samples[0]))
    tracker.update_memory = update_memory

    rng = np.random.default_rng(seed + 77)
    torch.manual_seed(seed)                                                      # the tracker draws proposal jitter from torch's RNG
    outs = []
    tracker.initialize(TH.synthetic_frame(rng), {"init_bbox": [200.0, 140.0, 70.0, 90.0]})
    for _ in range(n_frames):
        rec.add("frame", frame=tracker.frame_num + 1)
        out = tracker.track(TH.synthetic_frame(rng))
        outs.append(np.array(out["target_bbox"], dtype=np.float64))
        rec.add("state", target_bbox=outs[-1], flag=str(tracker.debug_info.get("flag", "")))
    return np.stack(outs), rec, (tracker, net)


def run_cpu_reference():
    """The golden: CPU, no install(), the stand-in sampler under the CUDA extension's name."""
    TH.ref_harness.install()
    import kys_standin
    kys_standin.register()
    return run(**RUN)


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
