"""Seeded synthetic workloads for the hot path.

There are no checkpoints and no datasets (no network), so every test, golden vector and benchmark
draws its inputs from the generators below.  They use numpy's PCG64 `default_rng(seed)` so the same
seed reproduces the same arrays in the build container (where the goldens are generated from the
reference) and on the GPU box (where the HIP path is checked against them) without shipping the
33 MB feature tensors.

Hyper-parameters are the deployed values the reference trains/tracks with (no learned values
exist here):
  DiMP-50   ltr/train_settings/dimp/dimp50.py:91-95, pytracking/parameter/dimp/dimp50.py
  PrDiMP-50 ltr/train_settings/dimp/prdimp50.py:95-98, pytracking/parameter/dimp/prdimp50.py
  ATOM      pytracking/parameter/atom/default.py
"""
import math

import numpy as np


def clf_features(rng, n, C, H, W, K):
    """N(0,1) features, instance-L2-normalised like `InstanceL2Norm(scale=sqrt(1/(C*K*K)))`
    (ltr/models/layers/normalization.py:15-20, dimpnet.py:159): x * sqrt(C*H*W / sum x^2) * scale."""
    x = rng.standard_normal((n, C, H, W), dtype=np.float32)
    ss = (x.astype(np.float64) ** 2).sum(axis=(1, 2, 3), keepdims=True)
    scale = math.sqrt(1.0 / (C * K * K))
    return (x * np.sqrt(C * H * W / ss) * scale).astype(np.float32)


def target_boxes(rng, n, crop=288.0):
    """xywh boxes around the crop centre: w,h ~ U(40,80), centre jitter U(-8,8) px (section 8d)."""
    wh = rng.uniform(40.0, 80.0, size=(n, 2))
    ctr = crop / 2.0 + rng.uniform(-8.0, 8.0, size=(n, 2))
    return np.concatenate((ctr - wh / 2.0, wh), axis=1).astype(np.float32)


def decay_weights(n, lr=0.01):
    """Steady-state DiMP memory weights (pytracking/tracker/dimp/dimp.py:445-484): the sample
    inserted j updates ago carries lr*(1-lr)^j, normalised to sum 1."""
    w = lr * (1.0 - lr) ** np.arange(n - 1, -1, -1, dtype=np.float64)
    return (w / w.sum()).astype(np.float32)


def gauss_lut(num_bins, bin_displacement, sigma):
    """`label_map_predictor` initial weights (optimizer.py:45-54)."""
    d = np.arange(num_bins, dtype=np.float32) * np.float32(bin_displacement)
    if sigma == 0:
        g = np.zeros_like(d)
        g[0] = 1
    else:
        g = np.exp(-0.5 * (d / np.float32(sigma)) ** 2)
    return (g - g.min()).astype(np.float32)


def mask_lut(num_bins, bin_displacement, mask_init_factor, mask_act="sigmoid"):
    """`target_mask_predictor[0]` initial weights (optimizer.py:57-66)."""
    d = np.arange(num_bins, dtype=np.float32) * np.float32(bin_displacement)
    bias = 0.0 if mask_act == "sigmoid" else 0.5
    return (mask_init_factor * np.tanh(2.0 - d) + bias).astype(np.float32)


DIMP50 = dict(  # dimpnet50(...) as instantiated by train_settings/dimp/dimp50.py:91-95
    C=512, H=18, W=18, K=4, feat_stride=16, num_iter=5, memory=50,
    init_step_length=0.9, init_filter_reg=0.1, min_filter_reg=1e-3, init_gauss_sigma=0.9,
    num_dist_bins=100, bin_displacement=0.1, mask_init_factor=3.0, mask_act="sigmoid",
    score_act="relu", alpha_eps=0.0,
)

PRDIMP50 = dict(  # klcedimpnet50(...) per train_settings/dimp/prdimp50.py:95-98; 22x22 per parameter/dimp/prdimp50.py:12
    C=512, H=22, W=22, K=4, feat_stride=16, num_iter=5, memory=50,
    init_step_length=1.0, init_filter_reg=0.05, min_filter_reg=0.05, gauss_sigma=0.9,
    alpha_eps=0.05, normalize_label=True, init_uni_weight=None, label_shrink=0.0,
    softmax_reg=None, label_threshold=0.0,
)

ATOM18 = dict(  # pytracking/parameter/atom/default.py:20-21,26-28,40,44-45,58-62,74
    C=64, H=18, W=18, K=4, memory=250, cg_iter=5, filter_reg=0.1, act_min_val=0.05,
    output_sigma_factor=0.25, search_area_scale=5.0,
)


def dimp_problem(seed, n, cfg=DIMP50, with_weights=True, small=None):
    """Inputs of one `filter_optimizer` call: (w0, feat, bb, sw).  `small` overrides C/H/W for the
    oracle-sized parity cases."""
    c = dict(cfg)
    if small:
        c.update(small)
    rng = np.random.default_rng(seed)
    feat = clf_features(rng, n, c["C"], c["H"], c["W"], c["K"])
    crop = c["feat_stride"] * c["H"]
    bb = target_boxes(rng, n, crop=float(crop))
    if crop < 200:      # tiny maps: shrink the boxes with the crop
        bb = (bb * (crop / 288.0)).astype(np.float32)
    sw = decay_weights(n) if with_weights else None
    w0 = (rng.standard_normal((c["C"], c["K"], c["K"]), dtype=np.float32) *
          np.float32(0.5 * math.sqrt(1.0 / (c["C"] * c["K"] ** 2))))
    return w0, feat, bb, sw


def atom_problem(seed, n, cfg=ATOM18, small=None):
    """Inputs of one ATOM `ConjugateGradient.run` call (section 8d cfg1)."""
    c = dict(cfg)
    if small:
        c.update(small)
    rng = np.random.default_rng(seed)
    C, H, W, K = c["C"], c["H"], c["W"], c["K"]
    samples = (rng.standard_normal((n, C, H, W), dtype=np.float32) * np.float32(0.1))
    # label_function_spatial Gaussians (pytracking/libs/dcf.py:56-72 semantics): centred labels with jitter
    sigma = c["output_sigma_factor"] * H / c["search_area_scale"] * 2.0
    ctr = np.stack((H / 2.0 + rng.uniform(-2, 2, n), W / 2.0 + rng.uniform(-2, 2, n)), axis=1)
    yy = np.arange(H, dtype=np.float64).reshape(1, -1, 1)
    xx = np.arange(W, dtype=np.float64).reshape(1, 1, -1)
    y = np.exp(-0.5 * ((yy - ctr[:, 0].reshape(-1, 1, 1)) ** 2 + (xx - ctr[:, 1].reshape(-1, 1, 1)) ** 2) / sigma ** 2)
    sw = decay_weights(n)
    x0 = rng.standard_normal((C, K, K), dtype=np.float32) * np.float32(0.05)
    return x0, samples, y.astype(np.float32), sw


# ------------------------------------------------------------------------------------------------------
# ToMP transformer model predictor (BASELINE configs[3])
# ------------------------------------------------------------------------------------------------------
TOMP = dict(  # tompnet50/101 as instantiated by ltr/train_settings/tomp/tomp50.py, tomp101.py (out_feature_dim=256)
    D=256, nhead=8, ff=2048, n_enc=6, n_dec=6, H=18, W=18, feature_sz=18, n_train=2, num_gth_frames=1)
TOMP_SMALL = dict(D=128, nhead=4, ff=256, n_enc=2, n_dec=2, H=6, W=6, feature_sz=6, n_train=2, num_gth_frames=1)


def _xavier(rng, shape, fan_in, fan_out):
    a = np.float32(math.sqrt(6.0 / (fan_in + fan_out)))
    return (rng.random(shape, dtype=np.float32) * 2 - 1) * a


def tomp_params(seed, cfg=TOMP):
    """Seeded parameters of FilterPredictor ('fp.'), LinearFilterClassifier ('cls.') and DenseBoxRegressor ('reg.'),
    keyed by the reference's state_dict names (filter_predictor.py:19-39, transformer.py:152-190,
    heads.py:83-117).  Xavier-uniform matrices as `Transformer._reset_parameters` (transformer.py:85-88) draws them;
    biases, LayerNorm / GroupNorm / BatchNorm affine terms and running statistics are perturbed away from their
    initial 0/1 so that a dropped term cannot go unnoticed."""
    rng = np.random.default_rng(seed)
    D, ff = cfg["D"], cfg["ff"]
    p = {}

    def vec(n, centre=0.0, spread=0.1):
        return (np.float32(centre) + np.float32(spread) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)

    def mha(prefix):
        p[prefix + "in_proj_weight"] = _xavier(rng, (3 * D, D), D, 3 * D)
        p[prefix + "in_proj_bias"] = vec(3 * D)
        p[prefix + "out_proj.weight"] = _xavier(rng, (D, D), D, D)
        p[prefix + "out_proj.bias"] = vec(D)

    def ffn_norms(prefix, norms):
        p[prefix + "linear1.weight"] = _xavier(rng, (ff, D), D, ff)
        p[prefix + "linear1.bias"] = vec(ff)
        p[prefix + "linear2.weight"] = _xavier(rng, (D, ff), ff, D)
        p[prefix + "linear2.bias"] = vec(D)
        for nm in norms:
            p[prefix + nm + ".weight"] = vec(D, 1.0)
            p[prefix + nm + ".bias"] = vec(D)

    for i in range(cfg["n_enc"]):
        pre = f"fp.transformer.encoder.layers.{i}."
        mha(pre + "self_attn.")
        ffn_norms(pre, ("norm1", "norm2"))
    for i in range(cfg["n_dec"]):
        pre = f"fp.transformer.decoder.layers.{i}."
        mha(pre + "self_attn.")
        mha(pre + "multihead_attn.")
        ffn_norms(pre, ("norm1", "norm2", "norm3"))
    p["fp.transformer.decoder.norm.weight"] = vec(D, 1.0)
    p["fp.transformer.decoder.norm.bias"] = vec(D)
    dims = [4, D // 4, D, D]                                        # MLP([4, d/4, d, d]) (filter_predictor.py:6-17,27)
    for li, idx in enumerate((0, 3, 6)):
        p[f"fp.box_encoding.{idx}.weight"] = _xavier(rng, (dims[li + 1], dims[li], 1), dims[li], dims[li + 1])
        p[f"fp.box_encoding.{idx}.bias"] = vec(dims[li + 1])
    for li, idx in enumerate((1, 4)):
        n = dims[li + 1]
        p[f"fp.box_encoding.{idx}.weight"] = vec(n, 1.0)
        p[f"fp.box_encoding.{idx}.bias"] = vec(n)
        p[f"fp.box_encoding.{idx}.running_mean"] = vec(n, 0.0, 0.2)
        p[f"fp.box_encoding.{idx}.running_var"] = (0.5 + rng.random(n, dtype=np.float32)).astype(np.float32)
    p["fp.query_embed_fg.weight"] = rng.standard_normal((1, D), dtype=np.float32)
    p["fp.query_embed_test.weight"] = rng.standard_normal((1, D), dtype=np.float32)
    p["cls.linear.weight"] = _xavier(rng, (D, D), D, D)
    p["cls.linear.bias"] = vec(D)
    p["reg.linear.weight"] = _xavier(rng, (D, D), D, D)
    p["reg.linear.bias"] = vec(D)
    for i in range(4):                                              # conv_layer x4 (heads.py:9-16,110-115)
        p[f"reg.tower.{3 * i}.weight"] = _xavier(rng, (D, D, 3, 3), 9 * D, 9 * D)
        p[f"reg.tower.{3 * i}.bias"] = vec(D)
        p[f"reg.tower.{3 * i + 1}.weight"] = vec(D, 1.0)
        p[f"reg.tower.{3 * i + 1}.bias"] = vec(D)
    p["reg.bbreg_layer.weight"] = _xavier(rng, (4, D, 3, 3), 9 * D, 9 * 4) * np.float32(0.3)
    p["reg.bbreg_layer.bias"] = vec(4)
    return p


def tomp_inputs(seed, cfg=TOMP):
    """Head features of the two memory frames and the test frame, Gaussian train labels and ltrb box maps
    (tomp.py:282-295, 552-570): shapes (n_train,1,D,H,W), (1,1,D,H,W), (n_train,1,H,W), (n_train,1,4,H,W)."""
    rng = np.random.default_rng(seed)
    D, H, W, n = cfg["D"], cfg["H"], cfg["W"], cfg["n_train"]
    scale = np.float32(1.0 / math.sqrt(D))
    train = rng.standard_normal((n, 1, D, H, W), dtype=np.float32) * scale * np.float32(4.0)
    test = rng.standard_normal((1, 1, D, H, W), dtype=np.float32) * scale * np.float32(4.0)
    ctr = np.stack((H / 2.0 + rng.uniform(-2, 2, n), W / 2.0 + rng.uniform(-2, 2, n)), axis=1)
    yy = np.arange(H, dtype=np.float64).reshape(1, -1, 1)
    xx = np.arange(W, dtype=np.float64).reshape(1, 1, -1)
    lab = np.exp(-0.5 * ((yy - ctr[:, 0].reshape(-1, 1, 1)) ** 2 + (xx - ctr[:, 1].reshape(-1, 1, 1)) ** 2) / 1.5 ** 2)
    half = rng.uniform(1.5, 4.0, (n, 2))
    l = (xx - (ctr[:, 1] - half[:, 1]).reshape(-1, 1, 1)) / W + 0 * yy
    r = ((ctr[:, 1] + half[:, 1]).reshape(-1, 1, 1) - xx) / W + 0 * yy
    t = (yy - (ctr[:, 0] - half[:, 0]).reshape(-1, 1, 1)) / H + 0 * xx
    b = ((ctr[:, 0] + half[:, 0]).reshape(-1, 1, 1) - yy) / H + 0 * xx
    ltrb = np.stack((l, t, r, b), axis=1)
    return (train.astype(np.float32), test.astype(np.float32), lab.astype(np.float32)[:, None],
            ltrb.astype(np.float32)[:, None])


# ------------------------------------------------------------------------------------------------------
# LWL few-shot learner and the IoU-guided refinement at deployed sizes
# ------------------------------------------------------------------------------------------------------
LWL = dict(n=32, F=16, C=512, H=30, W=52, K=3, filter_reg=0.05)   # lwl_ytvos.py:17,23; lwl_stage2.py:94-100


def lwl_problem(seed, cfg=LWL):
    """(w0, feat, label, sw) of one `GNSteepestDescent(LWTLResidual)` call: zero initial filter, per-element sample
    weights (`lwl_net` feeds a (n,1,F,H,W) weight tensor), labels in [0,1)."""
    rng = np.random.default_rng(seed)
    n, F, C, H, W, K = (cfg[k] for k in ("n", "F", "C", "H", "W", "K"))
    feat = clf_features(rng, n, C, H, W, K)
    label = rng.random((n, F, H, W), dtype=np.float32)
    sw = (np.float32(0.2) + np.float32(0.8) * rng.random((n, F, H, W), dtype=np.float32)).astype(np.float32)
    w0 = np.zeros((F, C, K, K), np.float32)
    return w0, feat, label, sw


IOU50 = dict(C=256, I=256, H3=36, W3=36, H4=18, W4=18, proposals=10)   # dimpnet50: AtomIoUNet(pred_input_dim=(256,256),
#                                                                        pred_inter_dim=(256,256)), dimpnet.py:189-190


def iou_net_params(seed, cfg=IOU50):
    """Seeded weights of the IoU predictor's test branch (atom_iou_net.py:44-49) keyed by the reference's state_dict
    names: two LinearBlocks (Linear + BatchNorm2d + ReLU) and Linear(2I, 1), magnitudes as `kaiming_normal_(fan_in)`
    (atom_iou_net.py:53-64) with the BatchNorm statistics moved off their initial 0/1."""
    rng = np.random.default_rng(seed)
    C, I = cfg["C"], cfg["I"]
    p = {}
    for name, k in (("fc3_rt", 5), ("fc4_rt", 3)):
        fan = C * k * k
        p[f"{name}.linear.weight"] = rng.standard_normal((I, fan), dtype=np.float32) * np.float32(math.sqrt(2.0 / fan))
        p[f"{name}.linear.bias"] = rng.standard_normal(I, dtype=np.float32) * np.float32(0.1)
        p[f"{name}.bn.weight"] = (np.float32(1.0) + np.float32(0.1) * rng.standard_normal(I, dtype=np.float32)).astype(np.float32)
        p[f"{name}.bn.bias"] = rng.standard_normal(I, dtype=np.float32) * np.float32(0.1)
        p[f"{name}.bn.running_mean"] = rng.standard_normal(I, dtype=np.float32) * np.float32(0.1)
        p[f"{name}.bn.running_var"] = (np.float32(0.5) + rng.random(I, dtype=np.float32)).astype(np.float32)
    p["iou_predictor.weight"] = rng.standard_normal((1, 2 * I), dtype=np.float32) * np.float32(math.sqrt(2.0 / (2 * I)))
    p["iou_predictor.bias"] = np.full(1, 0.3, np.float32)
    return p


def iou_inputs(seed, cfg=IOU50):
    """(c3, c4, mod3, mod4, boxes): IoU features of the test frame, modulation vectors, 10 jittered xywh proposals."""
    rng = np.random.default_rng(seed)
    C = cfg["C"]
    c3 = rng.standard_normal((1, C, cfg["H3"], cfg["W3"]), dtype=np.float32)
    c4 = rng.standard_normal((1, C, cfg["H4"], cfg["W4"]), dtype=np.float32)
    mod3 = (np.float32(1.0) + np.float32(0.5) * rng.standard_normal((1, C), dtype=np.float32)).astype(np.float32)
    mod4 = (np.float32(1.0) + np.float32(0.5) * rng.standard_normal((1, C), dtype=np.float32)).astype(np.float32)
    base = np.array([100.0, 90.0, 80.0, 110.0], np.float32)
    boxes = np.stack([base] + [base + np.concatenate((rng.uniform(-12, 12, 2), rng.uniform(-25, 25, 2))).astype(np.float32)
                               for _ in range(cfg["proposals"] - 1)])
    return c3, c4, mod3, mod4, boxes.astype(np.float32)


def atom_gn_problem(seed, n=30, M=256, Kc=64, H=18, W=18, K=4, cfg=ATOM18):
    """ATOM first frame (parameter/atom/default.py:27-28,40-45; atom.py:140-176): n augmented samples of M backbone
    channels, zero initial filter, PCA-like projection matrix.  Returns (f0, P0, samples, y, sw)."""
    rng = np.random.default_rng(seed)
    samples = rng.standard_normal((n, M, H, W), dtype=np.float32) * np.float32(0.1)
    _, _, y, sw = atom_problem(seed, n, cfg, small=dict(C=Kc, H=H, W=W))
    f0 = np.zeros((Kc, K, K), np.float32)
    P0 = rng.standard_normal((Kc, M), dtype=np.float32) * np.float32(1.0 / math.sqrt(M))
    return f0, P0, samples, y, sw


# ------------------------------------------------------------------------------------------------------
# Tracker-level replay (tests/tracker_replay.py): what stays on stock PyTorch in front of the hot path is synthetic
# ------------------------------------------------------------------------------------------------------
def tracker_backbone(seed, n, dims):
    """Backbone feature maps of `n` image patches: {'layer2': (n,C_layer2,H2,W2), 'layer3': (n,C_backbone,H,W)}.
    Every patch shows the sequence's appearance pattern (drawn from dims['base_seed'], the same in every call) plus
    per-call noise, so that a filter learnt on the first frame finds the target again in the later ones."""
    base = np.random.default_rng(dims.get("base_seed", 0))
    b3 = base.standard_normal((1, dims["C_backbone"], dims["H"], dims["W"]), dtype=np.float32)
    b2 = base.standard_normal((1, dims["C_layer2"], dims["H2"], dims["W2"]), dtype=np.float32)
    rng = np.random.default_rng(seed)
    sg = np.float32(dims.get("noise", 1.0))
    l3 = b3 + sg * rng.standard_normal((n, dims["C_backbone"], dims["H"], dims["W"]), dtype=np.float32)
    l2 = b2 + sg * rng.standard_normal((n, dims["C_layer2"], dims["H2"], dims["W2"]), dtype=np.float32)
    out = {"layer2": l2, "layer3": l3}
    # the segmentation trackers' decoder also reads layer1 (stride 4) and layer4 (stride 32); drawn BEHIND the two maps above, so the
    # streams of the dims without them are what they always were
    if "C_layer4" in dims:
        b4 = base.standard_normal((1, dims["C_layer4"], (dims["H"] + 1) // 2, (dims["W"] + 1) // 2), dtype=np.float32)
        b1 = base.standard_normal((1, dims["C_layer1"], 2 * dims["H2"], 2 * dims["W2"]), dtype=np.float32)
        out["layer4"] = b4 + sg * rng.standard_normal((n,) + b4.shape[1:], dtype=np.float32)
        out["layer1"] = b1 + sg * rng.standard_normal((n,) + b1.shape[1:], dtype=np.float32)
    return out


def tracker_iou_feat(seed, n, dims):
    """IoU features of the test frame (the output of `AtomIoUNet.get_iou_feat`, stock convolutions)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, dims["C_iou"], dims["H2"], dims["W2"]), dtype=np.float32),
            rng.standard_normal((n, dims["C_iou"], dims["H"], dims["W"]), dtype=np.float32))


def tracker_dimp_params(seed, dims):
    """Seeded hot-path weights of a DiMP network: classification-feature head conv ('head.weight'), the filter
    initialiser's conv ('init.weight', 'init.bias') and the IoU predictor's test branch ('iou.*', synth.iou_net_params)."""
    rng = np.random.default_rng(seed + 900)
    C, Cb = dims["C"], dims["C_backbone"]
    p = {"head.weight": rng.standard_normal((C, Cb, 3, 3), dtype=np.float32) * np.float32(math.sqrt(2.0 / (9 * C))),
         "init.weight": rng.standard_normal((C, C, 3, 3), dtype=np.float32) * np.float32(math.sqrt(2.0 / (9 * C))),
         "init.bias": rng.standard_normal(C, dtype=np.float32) * np.float32(0.01)}
    for k, v in iou_net_params(seed + 901, dict(C=dims["C_iou"], I=dims["C_iou"])).items():
        p["iou." + k] = v
    return p


def tracker_tomp_params(seed, dims, cfg=None):
    """Seeded hot-path weights of a ToMP network: the head's final conv ('head.weight') + synth.tomp_params."""
    cfg = cfg or TOMP
    rng = np.random.default_rng(seed + 910)
    C, Cb = dims["C"], dims["C_backbone"]
    p = {"head.weight": rng.standard_normal((C, Cb, 3, 3), dtype=np.float32) * np.float32(math.sqrt(2.0 / (9 * C)))}
    p.update(tomp_params(seed + 911, cfg))
    # random-init scores come out negative everywhere, which degenerates the tracker's peak logic (masked cells are 0):
    # flip the sign of the classifier's filter projection so that the score maps are positive
    p["cls.linear.weight"] = -p["cls.linear.weight"]
    p["cls.linear.bias"] = -p["cls.linear.bias"]
    return p


# GNSteepestDescent on LinearFilterHinge (dimpnet50_simple, super_dimp_simple.py:105-108 / the RTS classifier, rts_net.py:325-333)
DIMP_SIMPLE = dict(n=50, C=512, H=22, W=22, K=4, hinge_threshold=0.05, activation_leak=0.1, filter_reg=0.1)
RTS_CLF = dict(n=50, C=512, H=15, W=26, K=4, hinge_threshold=0.05, activation_leak=0.0, filter_reg=0.1)


def hinge_labels(rng, n, S, OH, OW, sigma=1.5):
    """(n, S, OH, OW) Gaussian label maps around jittered centres (the trackers' `init_target_labels` shape), values in (0, 1]."""
    cy = (OH - 1) / 2.0 + rng.uniform(-2.0, 2.0, size=(n, S, 1, 1))
    cx = (OW - 1) / 2.0 + rng.uniform(-2.0, 2.0, size=(n, S, 1, 1))
    y = np.arange(OH, dtype=np.float64).reshape(1, 1, OH, 1)
    x = np.arange(OW, dtype=np.float64).reshape(1, 1, 1, OW)
    return np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma)).astype(np.float32)


def gn_hinge_problem(seed, n, C, H, W, K, S=1, sw_mode="none"):
    """(w0, feat, label, sw) of one `GNSteepestDescent(LinearFilterHinge)` call: feat (n, S, C, H, W), w0 (S, C, K, K) small
    random, label (n, S, OH, OW), sw None or (n,) per-image weights summing to 1 (the trackers' memory weights)."""
    rng = np.random.default_rng(seed)
    OH, OW = H + (K + 1) % 2, W + (K + 1) % 2
    feat = np.stack([clf_features(rng, n, C, H, W, K) for _ in range(S)], axis=1)
    w0 = (rng.standard_normal((S, C, K, K), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    label = hinge_labels(rng, n, S, OH, OW)
    sw = None
    if sw_mode == "per_image":
        u = rng.uniform(0.5, 1.5, size=n)
        sw = (u / u.sum()).astype(np.float32)
    return w0, feat, label, sw


# KeepTrack target-candidate matching (ltr/models/target_candidate_matching): layer3 maps, the descriptor conv and SuperGlue's
# state as KeepTrack builds it (target_candidate_matching_net_resnet50: GNN_layers ['self', 'cross'] * 2)
TCM_FAST = dict(C=1024, H=22, W=22, D=256)        # parameter/keep_track/default_fast.py: image_sample_size 22*16
TCM_DEFAULT = dict(C=1024, H=30, W=30, D=256)     # parameter/keep_track/default.py: image_sample_size 30*16


def tcm_layer3(seed, B, C, H, W):
    """A non-negative layer3-like map (B, C, H, W)."""
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((B, C, H, W), dtype=np.float32), 0.0).astype(np.float32)


def tcm_desc_conv(seed, D=256, C=1024):
    """(weight (D, C, 4, 4), bias (D,)) of DescriptorExtractor.conv at a kaiming-like scale."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((D, C, 4, 4), dtype=np.float32) * np.float32(1.0 / np.sqrt(C * 16))).astype(np.float32)
    b = (rng.standard_normal(D, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    return w, b


def tcm_superglue_state(seed, n_layers=4, skip_gnn=False, bin_score=1.0):
    """A SuperGlue state_dict (numpy, float32) for the KeepTrack conf: 1/sqrt(fan_in) weights, and BatchNorm running statistics,
    gains and shifts away from their defaults so that folding them is exercised."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(name, o, i, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((o, i, 1), dtype=np.float32) * np.float32(gain / np.sqrt(i))).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)

    def bn(name, c):
        sd[name + ".weight"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(c) * 0.2).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.5, 2.0, c).astype(np.float32)
        sd[name + ".num_batches_tracked"] = np.array(100, dtype=np.int64)

    dims = [3, 32, 64, 128, 256, 256]
    for k in range(5):
        conv(f"kenc.encoder.{3 * k}", dims[k + 1], dims[k], gain=1.4)
        if k < 4:
            bn(f"kenc.encoder.{3 * k + 1}", dims[k + 1])
    if not skip_gnn:
        for l in range(n_layers):
            p = f"gnn.layers.{l}.update."
            conv(p + "attn.merge", 256, 256)
            for j in range(3):
                conv(p + f"attn.proj.{j}", 256, 256, gain=1.5)
            conv(p + "mlp.0", 512, 512, gain=1.4)
            bn(p + "mlp.1", 512)
            conv(p + "mlp.3", 256, 512, gain=0.5)
    conv("final_proj", 256, 256, gain=0.6)
    sd["bin_score"] = np.array(bin_score, dtype=np.float32)
    return sd


def tcm_match_inputs(seed, M, N, image_shape=(480, 640)):
    """descriptors (1, 256, M) / (1, 256, N), image coordinates (M, 2) / (N, 2) as (y, x) like KeepTrack's, scores (1, M) / (1, N)."""
    rng = np.random.default_rng(seed)
    h, w = image_shape
    out = {}
    for s, n in (("0", M), ("1", N)):
        out["descriptors" + s] = rng.standard_normal((1, 256, n), dtype=np.float32)
        out["img_coords" + s] = np.stack([rng.uniform(0, h, n), rng.uniform(0, w, n)], 1).astype(np.float32)
        out["scores" + s] = rng.uniform(0.05, 1.0, (1, n)).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# KYS response prediction (ltr/models/kys): motion features, module state, per-frame inputs
KYS = dict(C=1024, H=18, W=18, md=9, state_dim=8, rep_dims=(64, 32))    # kysnet.py:120-123 at the deployed search area


def kys_features(seed, B, C, H, W, shift=(1, -1)):
    """(cur, prev) layer3-like motion features (B, C, H, W): `prev` is `cur` displaced by `shift` plus noise, scaled so that a
    matching 3x3 window correlates to about 10 and a non-matching one to about 0.1 (a trained net's BatchNorm sees such a range)."""
    rng = np.random.default_rng(seed)
    a = np.float32(np.sqrt(10.0 / (9.0 * C)))
    cur = rng.standard_normal((B, C, H, W), dtype=np.float32) * a
    prev = np.roll(cur, shift, axis=(2, 3)) * np.float32(0.8) + rng.standard_normal((B, C, H, W), dtype=np.float32) * (a * np.float32(0.6))
    return cur.astype(np.float32), prev.astype(np.float32)


def kys_predictor_state(seed, conf_measure="max", state_dim=8, rep_dims=(64, 32)):
    """A ResponsePredictor state_dict (numpy, float32): kaiming-like conv weights, small biases, and BatchNorm running statistics,
    gains and shifts away from their defaults (the second cost-volume stack sees softmax outputs: its statistics are small)."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(name, o, i, bias=True, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((o, i, 3, 3), dtype=np.float32) * np.float32(gain * np.sqrt(2.0 / (9 * i)))).astype(np.float32)
        if bias:
            sd[name + ".bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)

    def bn(name, c, mean=0.2, var=(0.5, 2.0)):
        sd[name + ".weight"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(c) * mean).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(var[0], var[1], c).astype(np.float32)
        sd[name + ".num_batches_tracked"] = np.array(100, dtype=np.int64)

    for stack, mean, var in (("cost_volume_proc1", 0.2, (0.5, 2.0)), ("cost_volume_proc2", 0.002, (1e-4, 4e-4))):
        conv(stack + ".0.0", 8, 1)
        bn(stack + ".0.1", 8, mean, var)
        conv(stack + ".1.0", 1, 8)
        bn(stack + ".1.1", 1)
    in_dim = state_dim + 1 + (conf_measure != "none")
    for k, out_dim in enumerate(rep_dims):
        conv(f"representation_predictor.{k}.0", out_dim, in_dim)
        in_dim = out_dim
    conv("response_predictor.0.0", 1, in_dim)
    for g in ("conv_reset", "conv_update", "conv_state_new"):
        conv("state_predictor." + g, state_dim, 4 + state_dim)
    conv("init_hidden_state_predictor.0.0", state_dim, 1, bias=False, gain=2.0)
    conv("is_target_predictor.0.0", 4, state_dim)
    conv("is_target_predictor.1.0", 1, 4)
    return sd


def kys_frame_inputs(seed, B, H, W, state_dim=8):
    """Per-frame inputs: dimp_score (B, 1, H, W) (a peak near the centre, a distractor, noise), label_prev (B, 1, H, W) (a Gaussian
    label), state_prev (B, state_dim, H, W) in (-1, 1), window (1, H, W) (a Hann-like output window)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def bump(cy, cx, s):
        return np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))

    score = np.zeros((B, 1, H, W))
    label = np.zeros((B, 1, H, W))
    for b in range(B):
        cy, cx = (H - 1) / 2 + rng.uniform(-1, 1), (W - 1) / 2 + rng.uniform(-1, 1)
        score[b, 0] = 0.9 * bump(cy, cx, 1.2) + 0.5 * bump(rng.uniform(0, H - 1), rng.uniform(0, W - 1), 1.0) + 0.03 * rng.standard_normal((H, W))
        label[b, 0] = bump(cy + rng.uniform(-1, 1), cx + rng.uniform(-1, 1), 1.0)
    state = np.tanh(rng.standard_normal((B, state_dim, H, W)) * 0.7)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * (y + 1) / (H + 1))) * (0.5 - 0.5 * np.cos(2 * np.pi * (x + 1) / (W + 1)))
    return dict(dimp_score_cur=score.astype(np.float32), label_prev=label.astype(np.float32), state_prev=state.astype(np.float32),
                window=win[None].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# IoU feature extraction (ltr/models/bbreg/atom_iou_net.py:172-179): the four test-branch blocks and their backbone inputs
IOU_FEAT_CASES = {   # name: (n, (Cin3, Cmid3, Cout3, H3, W3), (Cin4, Cmid4, Cout4, H4, W4))
    "a": (1, (64, 16, 16, 1, 1), (64, 16, 16, 1, 1)),
    "b": (2, (64, 32, 16, 5, 7), (128, 16, 32, 3, 2)),
    "c": (1, (128, 48, 32, 11, 13), (64, 32, 48, 9, 4)),
    "d": (3, (64, 16, 16, 4, 33), (64, 16, 16, 33, 4)),
    "wide": (1, (64, 16, 16, 2, 172), (64, 64, 16, 1, 200)),      # rows wider than a band of the correlation kernel: the GEMM route
    "dimp50": (1, (512, 256, 256, 36, 36), (1024, 256, 256, 18, 18)),
    "prdimp50": (1, (512, 256, 256, 44, 44), (1024, 256, 256, 22, 22)),
    "atom18": (1, (128, 256, 256, 36, 36), (256, 256, 256, 18, 18)),
}


def iou_feat_state(seed, cin3, cin4, cmid3=256, cout3=256, cmid4=256, cout4=256):
    """A state dict (numpy, float32) for conv3_1t, conv3_2t, conv4_1t, conv4_2t of an AtomIoUNet: kaiming (fan-in) weights, non-zero
    biases, and BatchNorm gains, shifts and running statistics away from their defaults so that the epilogue constants are exercised."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, i, o in (("conv3_1t", cin3, cmid3), ("conv3_2t", cmid3, cout3), ("conv4_1t", cin4, cmid4), ("conv4_2t", cmid4, cout4)):
        sd[name + ".0.weight"] = (rng.standard_normal((o, i, 3, 3), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * i)))).astype(np.float32)
        sd[name + ".0.bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
        sd[name + ".1.weight"] = rng.uniform(0.5, 1.5, o).astype(np.float32)
        sd[name + ".1.bias"] = (rng.standard_normal(o) * 0.1).astype(np.float32)
        sd[name + ".1.running_mean"] = (rng.standard_normal(o) * 0.2).astype(np.float32)
        sd[name + ".1.running_var"] = rng.uniform(0.5, 2.0, o).astype(np.float32)
        sd[name + ".1.num_batches_tracked"] = np.array(100, dtype=np.int64)
    return sd


def iou_feat_inputs(seed, n, cin3, h3, w3, cin4, h4, w4):
    """(layer2 (n, cin3, h3, w3), layer3 (n, cin4, h4, w4)): non-negative maps, as the outputs of ResNet blocks are."""
    rng = np.random.default_rng(seed)
    f3 = np.maximum(rng.standard_normal((n, cin3, h3, w3), dtype=np.float32), 0.0).astype(np.float32)
    f4 = np.maximum(rng.standard_normal((n, cin4, h4, w4), dtype=np.float32), 0.0).astype(np.float32)
    return f3, f4


# ---------------------------------------------------------------------------------------------------------------------------
# IoU modulation vectors (ltr/models/bbreg/atom_iou_net.py:138-170): the five reference-branch blocks, the first-frame maps and boxes
IOU_MOD_DEPLOYED = (128, 256, 256, 256, 256)
IOU_MOD_CASES = {   # name: (n, (Cin3, H3, W3), (Cin4, H4, W4), (A, B, D, P3, P4)); the image is 8 H3 x 8 W3 (strides 8 and 16)
    "one": (1, (64, 1, 1), (64, 1, 1), (16, 16, 16, 16, 16)),                  # every tap but the centre is padding
    "edges": (6, (64, 9, 11), (64, 5, 6), (16, 32, 16, 32, 16)),               # the six box conditions of IOU_MOD_EDGE_BOXES
    "tiles": (2, (64, 20, 19), (64, 10, 9), (16, 16, 16, 16, 16)),             # a 17-column window; bins wider than 6 pixels
    "batch": (32, (64, 6, 6), (64, 3, 3), (16, 16, 16, 16, 16)),               # one map, 32 boxes: per-image window indexing
    "chan": (3, (128, 7, 5), (192, 4, 3), (48, 32, 80, 16, 48)),               # unequal B and D: the concatenation order
    "dimp50": (9, (512, 36, 36), (1024, 18, 18), IOU_MOD_DEPLOYED),
    "prdimp50": (9, (512, 44, 44), (1024, 22, 22), IOU_MOD_DEPLOYED),
    "atom18": (11, (128, 36, 36), (256, 18, 18), IOU_MOD_DEPLOYED),
}
IOU_MOD_EDGE_BOXES = ((8, 8, 40, 30),          # inside the map
                      (-20, -5, 30, 50),       # over the top-left edge
                      (200, 200, 10, 10),      # wholly outside: pooled values 0, the output is the tail's response to zero
                      (10, 10, 0, 5),          # zero width
                      (0, 0, 88, 72),          # the whole map: every tile live
                      (17, 9, 1, 1))           # inside one pixel


def iou_mod_state(seed, cin3, cin4, A=128, B=256, D=256, P3=256, P4=256):
    """A state dict (numpy, float32) for conv3_1r, conv4_1r, fc3_1r, fc34_3r, fc34_4r of an AtomIoUNet: kaiming (fan-in) weights, non-zero
    biases, and BatchNorm gains, shifts and running statistics away from their defaults, as iou_feat_state."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, i, o, k in (("conv3_1r", cin3, A, 3), ("conv4_1r", cin4, D, 3), ("fc3_1r", A, B, 3), ("fc34_3r", B + D, P3, 1),
                          ("fc34_4r", B + D, P4, 1)):
        sd[name + ".0.weight"] = (rng.standard_normal((o, i, k, k), dtype=np.float32) * np.float32(np.sqrt(2.0 / (k * k * i)))).astype(np.float32)
        sd[name + ".0.bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
        sd[name + ".1.weight"] = rng.uniform(0.5, 1.5, o).astype(np.float32)
        sd[name + ".1.bias"] = (rng.standard_normal(o) * 0.1).astype(np.float32)
        sd[name + ".1.running_mean"] = (rng.standard_normal(o) * 0.2).astype(np.float32)
        sd[name + ".1.running_var"] = rng.uniform(0.5, 2.0, o).astype(np.float32)
        sd[name + ".1.num_batches_tracked"] = np.array(100, dtype=np.int64)
    return sd


def iou_mod_boxes(name, seed=0):
    """(n, 4) float32 xywh boxes of a case of IOU_MOD_CASES, every coordinate a multiple of 1/4 (x + w is then exact in fp32).  The
    deployed cases carry the boxes of the first-frame augmentations that keep a box (dimp.py:469-490): the centred target, a fifth of
    the search side; the four `relativeshift` copies at +-0.6 of its size; the horizontally flipped copy; blur (and, for ATOM, rotation)
    copies, which keep the centred box."""
    n, (_, h3, w3), _, _ = IOU_MOD_CASES[name]
    Hi, Wi = 8 * h3, 8 * w3
    if name == "one":
        bb = [(2, 1, 5, 6)]
    elif name == "edges":
        bb = IOU_MOD_EDGE_BOXES
    elif name == "tiles":
        bb = [(10, 20, 120, 60),            # stride-8 columns 1 .. 17: straddles a 16-position tile; bins 5 pixels wide
              (0, 0, Wi, Hi)]               # bins 6.33 x 6.67 pixels at stride 8, 9.5 x 10 at stride 16: the general loop
    elif name in ("batch", "chan"):
        rng = np.random.default_rng(seed)
        xy = rng.uniform(-0.25, 0.8, (n, 2)) * (Wi, Hi)
        wh = rng.uniform(0.05, 0.7, (n, 2)) * (Wi, Hi)
        bb = np.round(np.concatenate([xy, wh], 1) * 4) / 4
    else:
        w, h = np.round(Wi / 5.0) + 0.5, np.round(Hi / 5.6) + 0.25
        x, y = np.round((Wi - w) / 2 * 4) / 4 + 1.25, np.round((Hi - h) / 2 * 4) / 4 - 2.5
        dx, dy = np.round(0.6 * w * 4) / 4, np.round(0.6 * h * 4) / 4
        bb = [(x, y, w, h), (x + dx, y + dy, w, h), (x - dx, y + dy, w, h), (x + dx, y - dy, w, h), (x - dx, y - dy, w, h),
              (Wi - x - w, y, w, h)] + [(x, y, w, h)] * (n - 6)
    bb = np.asarray(bb, dtype=np.float32).reshape(n, 4)
    assert np.array_equal(bb * 4, np.round(bb * 4))
    return bb


def iou_mod_inputs(seed, name):
    """(layer2 (n, Cin3, H3, W3), layer3 (n, Cin4, H4, W4), bb (n, 4) xywh): non-negative maps, as the outputs of ResNet blocks are;
    `batch` repeats one map in every image."""
    n, (c3, h3, w3), (c4, h4, w4), _ = IOU_MOD_CASES[name]
    rng = np.random.default_rng(seed)
    m = 1 if name == "batch" else n
    f3 = np.maximum(rng.standard_normal((m, c3, h3, w3), dtype=np.float32), 0.0).astype(np.float32)
    f4 = np.maximum(rng.standard_normal((m, c4, h4, w4), dtype=np.float32), 0.0).astype(np.float32)
    if m != n:
        f3, f4 = np.repeat(f3, n, 0), np.repeat(f4, n, 0)
    return f3, f4, iou_mod_boxes(name, seed + 7)


LABEL_ENC_DIMS = (16, 32, 64, 16)       # layer_dims of the deployed label encoders (lwl_stage2.py:94-99, rts50.py:130-135)
LABEL_ENC_CASES = {   # name: (n, H, W, layer_dims, use_bn)
    "one": (1, 7, 9, LABEL_ENC_DIMS, False),                 # every stage collapses to 1 x 1: all taps but the centre are padding
    "sixteen": (1, 16, 16, LABEL_ENC_DIMS, False),           # exact / 16
    "odd": (3, 33, 50, LABEL_ENC_DIMS, False),               # odd sizes, output 3 x 4, per-mask indexing
    "bands": (2, 40, 72, LABEL_ENC_DIMS, False),             # several row bands of the stem and of the first block
    "wide": (1, 24, 300, LABEL_ENC_DIMS, False),             # wider than a workgroup's tile at every stage (75 / 38 / 19 / 19 columns)
    "deployed": (2, 480, 832, LABEL_ENC_DIMS, False),        # lwl_ytvos.py image_sample_size; the tracker runs up to 32 of them
    "bn_odd": (3, 33, 50, LABEL_ENC_DIMS, True),
    "bn_wide": (1, 24, 300, LABEL_ENC_DIMS, True),
    "dims": (2, 37, 70, (16, 16, 32, 32), False),            # channel counts other than the deployed ones
}


def label_enc_state(seed, dims=LABEL_ENC_DIMS, use_bn=False):
    """A state dict (numpy, float32) of a ResidualDS16SW(dims, use_bn): kaiming (fan-in) weights, non-zero biases, a non-zero
    samp_w_pred.weight (the reference initialises it to 0, which would hide a broken head) and, with use_bn, BatchNorm gains, shifts and
    running statistics away from their defaults."""
    rng = np.random.default_rng(seed)
    c0, c1, c2, f = dims
    sd = {}

    def conv(name, i, o, bias):
        sd[name + ".weight"] = (rng.standard_normal((o, i, 3, 3), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * i)))).astype(np.float32)
        if bias:
            sd[name + ".bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)

    def bn(name, o):
        if not use_bn:
            return
        sd[name + ".weight"] = rng.uniform(0.5, 1.5, o).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(o) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(o) * 0.2).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.5, 2.0, o).astype(np.float32)
        sd[name + ".num_batches_tracked"] = np.array(100, dtype=np.int64)

    conv("conv_block.0", 1, c0, True); bn("conv_block.1", c0)
    for blk, i, o in (("res1", c0, c1), ("res2", c1, c2)):
        conv(blk + ".conv1", i, o, False); bn(blk + ".bn1", o)
        conv(blk + ".conv2", o, o, False); bn(blk + ".bn2", o)
        conv(blk + ".downsample", i, o, True)
    conv("label_pred.0", c2, f, True); bn("label_pred.1", f)
    conv("samp_w_pred", c2, f, True)
    return sd


def label_enc_masks(seed, n, H, W):
    """(n, H, W) float32 soft masks in [0, 1] as `sample_patch(..., is_mask=True)` yields them: an elliptical blob per mask with an exact-1
    interior, an exact-0 background and a bilinear-looking edge a few pixels wide in between."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((n, H, W), dtype=np.float32)
    for k in range(n):
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        ry, rx = rng.uniform(0.15, 0.35) * H + 1.0, rng.uniform(0.15, 0.35) * W + 1.0
        edge = rng.uniform(1.5, 4.0)
        d = (np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) - 1.0) * min(ry, rx)      # signed distance to the ellipse, about px
        out[k] = np.clip(0.5 - d / edge, 0.0, 1.0).astype(np.float32)
    return out


# Segmentation decoder (ltr/models/lwl/decoder.py:87-160).  name: dict(n, mdim, ic, use_bn, levels = ((layer, fc, H, W), ...) deepest first,
# image (H, W), scores (h, w)).  Feature maps are inputs: their sizes need not come from a real backbone.
LWL_DECODER_CASES = {
    # every resize ratio is non-integral
    "tiny": dict(n=1, mdim=32, ic=16, use_bn=True, levels=(("layer4", 32, 2, 2), ("layer3", 32, 3, 4), ("layer2", 16, 5, 7), ("layer1", 16, 9, 13)),
                 image=(33, 50), scores=(3, 4)),
    # no layer4: layer3 is the deepest level; no BatchNorm
    "three": dict(n=2, mdim=32, ic=16, use_bn=False, levels=(("layer3", 32, 4, 6), ("layer2", 16, 7, 11), ("layer1", 16, 14, 22)),
                  image=(56, 88), scores=(4, 6)),
    # several bands and channel splits on the banded route
    "bands": dict(n=2, mdim=32, ic=16, use_bn=True, levels=(("layer4", 64, 5, 9), ("layer3", 32, 10, 18), ("layer2", 32, 20, 36), ("layer1", 16, 40, 72)),
                  image=(160, 288), scores=(10, 18)),
    # rows wider than the banded route stages: the GEMM route at layer1 and in the Upsampler
    "wide": dict(n=1, mdim=32, ic=16, use_bn=True, levels=(("layer4", 32, 1, 23), ("layer3", 32, 2, 45), ("layer2", 16, 3, 90), ("layer1", 16, 6, 180)),
                 image=(24, 720), scores=(2, 45)),
    # a score map of another size than every level: a real bilinear down- and up-resize
    "ratio": dict(n=1, mdim=32, ic=32, use_bn=True, levels=(("layer4", 32, 3, 5), ("layer3", 32, 6, 10), ("layer2", 16, 12, 20), ("layer1", 16, 24, 40)),
                  image=(96, 160), scores=(8, 13)),
    # lwl_ytvos.py / lwl_stage2.py: 480 x 832 image, ResNet-50 layers 4..1, decoder_mdim 64, 16 score channels, BatchNorm
    "deployed": dict(n=1, mdim=64, ic=16, use_bn=True,
                     levels=(("layer4", 2048, 15, 26), ("layer3", 1024, 30, 52), ("layer2", 512, 60, 104), ("layer1", 256, 120, 208)),
                     image=(480, 832), scores=(30, 52)),
}
_LWL_DECODER_OC = {"layer1": 1, "layer2": 2, "layer3": 2, "layer4": 4}


def lwl_decoder_state(seed, mdim, ic, use_bn, levels):
    """A state dict (numpy, float32) of an LWTLDecoder(ic, mdim, {layer: fc}, use_bn): fan-in scaled weights (the residual branches and the
    CAB sum scaled down so that activations stay O(1) through all levels), non-zero biases and, with use_bn, BatchNorm gains, shifts and
    running statistics away from their defaults."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(name, i, o, k, bias=True, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((o, i, k, k), dtype=np.float32) * np.float32(gain * np.sqrt(1.0 / (k * k * i)))).astype(np.float32)
        if bias:
            sd[name + ".bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)

    def rrb(name, oc):
        conv(name + ".conv1x1", oc, oc, 1, gain=0.8)
        conv(name + ".bblock.0", oc, oc, 3, gain=1.4)
        if use_bn:
            sd[name + ".bblock.1.weight"] = rng.uniform(0.5, 1.5, oc).astype(np.float32)
            sd[name + ".bblock.1.bias"] = (rng.standard_normal(oc) * 0.1).astype(np.float32)
            sd[name + ".bblock.1.running_mean"] = (rng.standard_normal(oc) * 0.2).astype(np.float32)
            sd[name + ".bblock.1.running_var"] = rng.uniform(0.5, 2.0, oc).astype(np.float32)
            sd[name + ".bblock.1.num_batches_tracked"] = np.array(100, dtype=np.int64)
        conv(name + ".bblock.%d" % (3 if use_bn else 2), oc, oc, 3, bias=False, gain=0.7)

    prev = None
    for L, fc, _, _ in levels:
        oc = _LWL_DECODER_OC[L] * mdim
        nc = oc + ic
        if prev is not None:
            conv("proj.%s.0" % L, prev, oc, 1, gain=0.7)
        conv("TSE.%s.reduce.0" % L, fc, oc, 1, gain=1.4)
        conv("TSE.%s.reduce.2" % L, oc, oc, 1, gain=1.4)
        for k in (0, 2, 4):
            conv("TSE.%s.transform.%d" % (L, k), nc, oc if k == 4 else nc, 3, gain=1.4)
        rrb("RRB1.%s" % L, oc)
        conv("CAB.%s.convreluconv.0" % L, 2 * oc, oc, 1, gain=1.4)
        conv("CAB.%s.convreluconv.2" % L, oc, oc, 1, gain=2.0)
        rrb("RRB2.%s" % L, oc)
        prev = oc
    conv("project.conv1", mdim, mdim // 2, 3, gain=1.4)
    conv("project.conv2", mdim // 2, 1, 3, gain=1.4)
    return sd


def lwl_decoder_inputs(seed, n, ic, levels, scores):
    """(scores (n, 1, ic, h, w), {layer: (n, fc, H, W)}) float32: signed score channels, rectified features."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n, 1, ic) + tuple(scores), dtype=np.float32)
    feats = {L: np.maximum(rng.standard_normal((n, fc, H, W), dtype=np.float32), 0.0).astype(np.float32) for L, fc, H, W in levels}
    return s, feats


# ---------------------------------------------------------------------------------------------------------------------------
# Feature heads of LWL / RTS: Conv2d(Cin, Cout, 3, stride 1 or 2, padding 1, no bias) + InstanceL2Norm
# (ltr/models/target_classifier/features.py:9-28, 49-73)
FEAT_HEAD_CASES = {   # name: (n, Cin, Cout, H, W); every case runs at stride 2 and at stride 1
    "one": (1, 64, 16, 1, 1),            # one output: only the centre tap is inside the map
    "two_three": (1, 64, 16, 2, 3),      # smallest map with an even and an odd side
    "cout36": (1, 64, 36, 6, 7),         # Cout no multiple of 16; even H: last row fully inside, odd W: last column padded
    "odd_h": (2, 128, 32, 5, 8),         # odd H, two images
    "straddle": (3, 192, 16, 5, 22),     # 33 output tokens per image: a 32-token tile straddles images; three K-steps per tap
    "map": (3, 64, 16, 30, 52),          # the deployed map at a small width, 390 output tokens per image
}
FEAT_HEAD_DEPLOYED = (1, 1024, 512, 30, 52)   # lwl_net.py:173-177, rts_net.py:294-298 (stride 1); rts_net.py:339-344 (stride 2)
FEAT_HEAD_SCALE = 0.1                         # norm_scale of the cases: the RMS of every output


def feat_head_problem(seed, n, Cin, Cout, H, W, integers=False):
    """(x (n, Cin, H, W), weight (Cout, Cin, 3, 3)) float32: non-negative maps, as the outputs of ResNet blocks are, and kaiming (fan-in)
    weights; `integers`: both drawn from -2 ... 2, so that every convolution sum is exact in fp32 in any order."""
    rng = np.random.default_rng(seed)
    if integers:
        return (rng.integers(-2, 3, (n, Cin, H, W)).astype(np.float32), rng.integers(-2, 3, (Cout, Cin, 3, 3)).astype(np.float32))
    x = np.maximum(rng.standard_normal((n, Cin, H, W), dtype=np.float32), 0.0).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * Cin)))).astype(np.float32)
    return x, w


# ---------------------------------------------------------------------------------------------------------------------------
# RTS instance-score encoder (ltr/models/rts/label_encoder.py:57-103) and learners fusion (rts_net.py:219-236, learners_fusion.py).
# The encoder has the parameter names and shapes of the mask label encoder (every stride is 1 instead of 2): its states are
# `label_enc_state`.  The classifier score map of the deployed tracker is 16 x 27 (15 x 26 features, 4 x 4 filter; rts50.py) and is fused
# with the 30 x 52 mask encoding.
SCORE_ENC_CASES = {   # name: (n, H, W, layer_dims, use_bn)
    "one": (1, 1, 1, LABEL_ENC_DIMS, False),                 # every tap but the centre is padding; the pool window has one member
    "row": (1, 1, 19, LABEL_ENC_DIMS, False),                # a single row wider than a 16-pixel tile
    "odd": (3, 5, 7, LABEL_ENC_DIMS, False),                 # per-map indexing
    "edge": (1, 17, 33, LABEL_ENC_DIMS, False),              # one past a tile boundary in both directions
    "deployed": (2, 16, 27, LABEL_ENC_DIMS, False),          # the tracker's size; n = 2 so that the batch stride is exercised
    "bn": (2, 9, 20, LABEL_ENC_DIMS, True),                  # BatchNorm folding
    "dims": (2, 11, 13, (16, 16, 32, 32), False),            # channel counts other than the deployed ones
}
LEARNERS_FUSE_CASES = {   # name: (n, F, (Hs, Ws), (Ht, Wt)); every case runs as 'add' and as 'concat'
    "same": (1, 16, (6, 9), (6, 9)),                         # the no-resize branch
    "up1": (1, 16, (1, 1), (3, 4)),                          # every neighbour clamped
    "deployed": (1, 16, (16, 27), (30, 52)),                 # the tracker's size
    "down": (2, 16, (9, 11), (4, 5)),                        # shrinking without antialiasing
    "edge": (1, 16, (8, 14), (17, 33)),                      # one past a tile boundary
    "f32": (1, 32, (5, 7), (9, 13)),                         # F other than 16
}
FUSION_TYPES = ("add", "concat")
RTS_CHAIN_CASE = dict(H=16, W=27, dims=LABEL_ENC_DIMS, target=(30, 52))     # chain_deployed: the encoder, then the fuse


def score_maps(seed, n, H, W):
    """(n, H, W) float32 classifier score maps, roughly in [-0.2, 1]: one peaked target response, two weaker distractors and noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((n, H, W), dtype=np.float32)
    for k in range(n):
        s = rng.standard_normal((H, W)) * 0.04 - 0.02
        for amp in (rng.uniform(0.8, 1.0), rng.uniform(0.2, 0.45), rng.uniform(0.1, 0.3)):
            cy, cx = rng.uniform(0.0, 1.0) * (H - 1), rng.uniform(0.0, 1.0) * (W - 1)
            sig = rng.uniform(0.8, 1.6)
            s = s + amp * np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / sig ** 2)
        out[k] = np.clip(s, -0.2, 1.0).astype(np.float32)
    return out


def learners_fusion_state(seed, f, fusion_type):
    """A state dict (numpy, float32) of a LearnersFusion: empty for 'add'; for 'concat' the Conv2d(2F, F, 3, padding=1) with fan-in scaled
    weights and a non-zero bias."""
    if fusion_type == "add":
        return {}
    rng = np.random.default_rng(seed)
    return {"fusion_conv1.weight": (rng.standard_normal((f, 2 * f, 3, 3), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * 2 * f)))).astype(np.float32),
            "fusion_conv1.bias": (rng.standard_normal(f, dtype=np.float32) * np.float32(0.1)).astype(np.float32)}


def learners_fuse_inputs(seed, n, f, source, target):
    """(seg_enc (1, n, F, Ht, Wt) signed, as a target model's mask encoding; clf_enc (1, n, F, Hs, Ws) non-negative, as the encoder's
    rectified output) float32."""
    rng = np.random.default_rng(seed)
    seg = rng.standard_normal((1, n, f) + tuple(target), dtype=np.float32)
    clf = np.maximum(rng.standard_normal((1, n, f) + tuple(source), dtype=np.float32), 0.0).astype(np.float32)
    return seg, clf


# ---------------------------------------------------------------------------------------------------------------------------
# ECO (pytracking/tracker/eco): inputs of the Fourier-domain per-frame path

def eco_features(seed, S, C, H, W, smooth=2):
    """Spatially correlated feature maps (S, C, H, W), float32: white noise box-filtered `smooth` times along both axes (periodic) and
    rescaled to unit variance, so that their spectrum decays with the frequency as a real backbone's does."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, C, H, W))
    for _ in range(smooth):
        x = (np.roll(x, 1, 2) + x + np.roll(x, -1, 2)) / 3.0 if H > 2 else x
        x = (np.roll(x, 1, 3) + x + np.roll(x, -1, 3)) / 3.0 if W > 2 else x
    return (x / max(x.std(), 1e-6)).astype(np.float32)


def eco_projection(seed, Cin, c):
    """A projection matrix (Cin, c) with orthonormal columns, as the PCA initialisation of eco.py:110-113 gives."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((Cin, c)))
    return np.ascontiguousarray(q[:, :c]).astype(np.float32)


def eco_window(H, W):
    """dcf.hann2d (dcf.py:8-18), centred: (1, 1, H, W) float32."""
    def hann(n):
        return 0.5 * (1.0 - np.cos((2.0 * math.pi / (n + 1)) * np.arange(1, n + 1)))
    return (hann(H)[:, None] * hann(W)[None, :]).astype(np.float32).reshape(1, 1, H, W)


def eco_interp(seed, H, W):
    """Complex interpolation factors in get_interp_fourier's shapes and magnitudes (dcf.py:74-94): interp_y (1, 1, Hf, 1, 2) of modulus about
    1 / H with the centring phase -pi ky / Hf, interp_x (1, 1, 1, Wh, 2) likewise; the moduli are seeded instead of the cubic spline's."""
    rng = np.random.default_rng(seed)
    Hf, Wh = H + (H + 1) % 2, W // 2 + 1
    ky, kx = np.arange(Hf) - (Hf - 1) // 2, np.arange(Wh)
    my, mx = rng.uniform(0.5, 1.0, Hf) / Hf, rng.uniform(0.5, 1.0, Wh) / (2 * Wh - 1)
    iy = np.stack((my * np.cos(-math.pi * ky / Hf), my * np.sin(-math.pi * ky / Hf)), -1)
    ix = np.stack((mx * np.cos(-math.pi * kx / (2 * Wh - 1)), mx * np.sin(-math.pi * kx / (2 * Wh - 1))), -1)
    return iy.astype(np.float32).reshape(1, 1, Hf, 1, 2), ix.astype(np.float32).reshape(1, 1, 1, Wh, 2)


def eco_series(seed, S, c, Hf, Wh, decay=0.35):
    """Half-spectrum coefficients (S, c, Hf, Wh, 2), float32, Hermitian-consistent in the kx = 0 column (row r is the conjugate of row
    Hf - 1 - r there, the centre real) with moduli that decay with the frequency: what the sample transform produces, without running it."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((S, c, Hf, Wh, 2))
    ky, kx = np.abs(np.arange(Hf) - (Hf - 1) // 2)[:, None], np.arange(Wh)[None, :]
    a *= (1.0 / (1.0 + decay * np.hypot(ky, kx)) ** 2)[None, None, :, :, None]
    col = a[:, :, :, 0, :]
    flip = col[:, :, ::-1, :] * np.array([1.0, -1.0])
    a[:, :, :, 0, :] = 0.5 * (col + flip)
    return a.astype(np.float32)


# Box label encoders (ltr/models/lwl/label_encoder.py:58-216, ltr/models/rts/label_encoder.py:106-265), use_gauss = False.
# ResidualDS16FeatSWBox: dims = (c0, c1, c2, c3, F); the feature map has the trunk's output size (four stride-2 stages of `image`).
BOX_ENC_DIMS = (16, 32, 64, 128, 16)    # sta_net.py:137-142, rts_net.py:546-553: label_encoder_dims + (num_filters,)
BOX_ENC_CASES = {
    "one": dict(n=1, image=(7, 9), dims=(16, 16, 32, 32, 16), feat_dim=16, boxes=[(2, 1, 4, 3)]),       # 1 x 1 map: every tap but the centre is padding
    "odd": dict(n=3, image=(33, 50), dims=BOX_ENC_DIMS, feat_dim=48,                                      # 3 x 4 map, Cin = 112, per-image indexing
                boxes=[(10.7, 5.2, 20.9, 15.1), (-6.5, -4.2, 20.3, 18.8), (-3, -2, 80, 60)]),            # inside; left of / above; everything
    "ragged": dict(n=2, image=(40, 72), dims=(16, 16, 32, 48, 32), feat_dim=80, boxes=[(30, 10, 25, 20), (5.5, 20.5, 40, 12)]),
    "edge": dict(n=1, image=(70, 260), dims=(16, 32, 64, 80, 16), feat_dim=32, boxes=[(200, 40, 100, 50)]),   # 5 x 17 map; past right / bottom
    "wrap": dict(n=2, image=(33, 50), dims=BOX_ENC_DIMS, feat_dim=32, boxes=[(5, -30, 20, 10), (-40, 3, 15, 20)]),   # negative stops
    "nosw": dict(n=2, image=(33, 50), dims=BOX_ENC_DIMS, feat_dim=32, use_sample_w=False, boxes=[(12, 8, 20, 14), (30, 2, 15, 28)]),
    "bn": dict(n=2, image=(40, 72), dims=BOX_ENC_DIMS, feat_dim=32, use_bn=True, final_relu=False, boxes=[(20, 10, 30, 20), (-5, 15, 40, 40)]),
    "deployed": dict(n=1, image=(480, 832), dims=BOX_ENC_DIMS, feat_dim=512, boxes=[(301.4, 151.7, 190.2, 222.9)]),
    "deployed2": dict(n=2, image=(480, 832), dims=BOX_ENC_DIMS, feat_dim=512, boxes=[(301.4, 151.7, 190.2, 222.9), (-20.5, 300.2, 400.6, 250.3)]),
}
# ResidualDS16FeatSWBoxCatMultiBlock: dims = the block widths, then F; `feat` = (h, w) of the feature map, any size.
BOX_CAT_ENC_CASES = {
    "one": dict(n=1, image=(7, 9), feat=(1, 1), dims=(16, 16), feat_dim=16, boxes=[(4, 3, 4, 3)]),     # the one sample (row 3, column 4) is the box's corner
    "odd": dict(n=3, image=(33, 50), feat=(3, 4), dims=(64, 64, 16), feat_dim=48,                         # a non-integer resize ratio
                boxes=[(10.7, 5.2, 20.9, 15.1), (-6.5, -4.2, 20.3, 18.8), (0, 0, 80, 60)]),
    "ragged": dict(n=2, image=(40, 72), feat=(5, 7), dims=(48, 32), feat_dim=80, boxes=[(30, 10, 25, 20), (5.5, 20.5, 40, 12)]),
    "edge": dict(n=1, image=(70, 260), feat=(5, 17), dims=(80, 16), feat_dim=32, boxes=[(206, 40, 100, 50)]),     # column 206 is a resize tap
    "wrap": dict(n=3, image=(33, 50), feat=(5, 7), dims=(32, 16), feat_dim=32,                            # negative stop; negative start; both (empty)
                 boxes=[(5, -30, 20, 10), (-45, 3, 15, 20), (-10, 4, 25, 10)]),
    "same": dict(n=2, image=(6, 9), feat=(6, 9), dims=(32, 16), feat_dim=16, boxes=[(2, 1, 4, 3), (-3, 2, 5, 3)]),   # the resize is the identity
    "blocks1": dict(n=2, image=(40, 72), feat=(6, 10), dims=(32, 16), feat_dim=32, final_relu=False, final_bn=False, boxes=[(20, 10, 30, 20), (3, 15, 40, 20)]),
    "blocks3": dict(n=2, image=(40, 72), feat=(6, 10), dims=(32, 48, 16, 16), feat_dim=32, boxes=[(20, 10, 30, 20), (3, 15, 40, 20)]),
    "deployed": dict(n=1, image=(480, 832), feat=(30, 52), dims=(64, 64, 16), feat_dim=512, final_bn=False,    # lwl_boxinit.py:90-95, lwl_box_net.py:169-173
                     boxes=[(301.4, 151.7, 190.2, 222.9)]),
}
_BOX_ENC_DEFAULTS = dict(use_bn=False, use_sample_w=True, final_relu=True)
_BOX_CAT_ENC_DEFAULTS = dict(use_bn=True, final_relu=True, final_bn=True)


def box_enc_case(name):
    """BOX_ENC_CASES[name] with the defaults filled in and `feat` = the trunk's output size."""
    c = dict(_BOX_ENC_DEFAULTS, **BOX_ENC_CASES[name])
    h, w = c["image"]
    for _ in range(4):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    c["feat"] = (h, w)
    return c


def box_cat_enc_case(name):
    return dict(_BOX_CAT_ENC_DEFAULTS, **BOX_CAT_ENC_CASES[name])


def _box_enc_layers(rng, sd, use_bn):
    def conv(name, i, o, bias):
        sd[name + ".weight"] = (rng.standard_normal((o, i, 3, 3), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * i)))).astype(np.float32)
        if bias:
            sd[name + ".bias"] = (rng.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)

    def bn(name, o, on=use_bn):
        if not on:
            return
        sd[name + ".weight"] = rng.uniform(0.5, 1.5, o).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(o) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(o) * 0.2).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.5, 2.0, o).astype(np.float32)
        sd[name + ".num_batches_tracked"] = np.array(100, dtype=np.int64)

    def block(name, i, o):
        conv(name + ".conv1", i, o, False); bn(name + ".bn1", o)
        conv(name + ".conv2", o, o, False); bn(name + ".bn2", o)
        conv(name + ".downsample", i, o, True)

    return conv, bn, block


def box_enc_state(seed, dims=BOX_ENC_DIMS, feat_dim=512, use_bn=False, use_sample_w=True):
    """A state dict (numpy, float32) of a ResidualDS16FeatSWBox(dims, feat_dim, use_bn=..., use_sample_w=...): kaiming (fan-in) weights,
    non-zero biases, a non-zero samp_w_pred.weight and BatchNorm statistics away from their defaults.  label_pred is a conv_block with
    its default BatchNorm whatever use_bn says (the class does not pass the flag on)."""
    rng = np.random.default_rng(seed)
    c0, c1, c2, c3, f = dims
    sd = {}
    conv, bn, block = _box_enc_layers(rng, sd, use_bn)
    conv("conv_block.0", 1, c0, True); bn("conv_block.1", c0)
    block("res1", c0, c1); block("res2", c1, c2); block("res3", c2 + feat_dim, c3)
    conv("label_pred.0", c3, f, True); bn("label_pred.1", f, True)
    if use_sample_w:
        conv("samp_w_pred", c3, f, True)
    return sd


def box_cat_enc_state(seed, dims=(64, 64, 16), feat_dim=512, use_bn=True, final_bn=True):
    """A state dict (numpy, float32) of a ResidualDS16FeatSWBoxCatMultiBlock(dims, feat_dim, use_bn=..., final_bn=...)."""
    rng = np.random.default_rng(seed)
    sd = {}
    conv, bn, block = _box_enc_layers(rng, sd, use_bn)
    cin = feat_dim + 1
    for k, c in enumerate(dims[:-1]):
        block(f"res.{k}", cin, c)
        cin = c
    conv("label_pred.0", cin, dims[-1], True); bn("label_pred.1", dims[-1], final_bn)
    return sd


def box_enc_feat(seed, n, feat_dim, h, w):
    """(n, feat_dim, h, w) float32 target-model features: rectified, roughly unit scale, as the feature head leaves them."""
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((n, feat_dim, h, w), dtype=np.float32), np.float32(0.0)) * np.float32(0.5)
