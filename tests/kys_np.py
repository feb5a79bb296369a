"""TEST INFRASTRUCTURE ONLY -- float64 numpy restatement of the KYS response prediction (ltr/models/kys): the cost-volume definition
of include/pt_hot.h as a brute-force loop over sequences, current rows / columns and previous rows / columns, and the eval-mode
ResponsePredictor chain with the shift_features calls of PredictorWrapper.predict_response around it.

The cost volume is the UNPINNED piece: `spatial_correlation_sampler` (a CUDA extension) is not installable here, so its semantics are
written from its documented behaviour -- kernel_size 3, stride 1, padding 1, patch_size 2 md + 1, a tap contributing only where both
indices are inside the map, no normalisation."""
import numpy as np

SHIFT_PX = 0.25     # |0.5 / size| * size / 2: affine_grid / grid_sample at align_corners=False (checked against torch in test_kys_cpu)


def cost_volume(cur, prev, md, remap=True):
    """Brute force.  cur, prev (B, C, H, W) -> (B, (2 md + 1)^2, H, W), or (B, H*W, H, W) through `remap`.  Zero padding by md + 1
    makes a tap outside either map a zero product, which is the 'both indices inside' rule."""
    cur, prev = np.asarray(cur, np.float64), np.asarray(prev, np.float64)
    B, C, H, W = cur.shape
    P, D = md + 1, 2 * md + 1
    cp = np.pad(cur, ((0, 0), (0, 0), (P, P), (P, P)))
    pp = np.pad(prev, ((0, 0), (0, 0), (P, P), (P, P)))
    out = np.zeros((B, D * D, H, W))
    for b in range(B):
        for r in range(H):
            for c in range(W):
                a = cp[b, :, r + P - 1:r + P + 2, c + P - 1:c + P + 2]
                for r2 in range(r - md, r + md + 1):
                    for c2 in range(c - md, c + md + 1):
                        out[b, (r2 - r + md) * D + (c2 - c + md), r, c] = np.vdot(a, pp[b, :, r2 + P - 1:r2 + P + 2, c2 + P - 1:c2 + P + 2])
    return remap_cost_volume(out) if remap else out


def remap_cost_volume(cv):
    """(B, (2 md + 1)^2, H, W) -> (B, H*W, H, W): channel (r', c') of position (r, c) is displacement (r' - r, c' - c), zero outside
    the window (cost_volume.py:29-75)."""
    B, DD, H, W = cv.shape
    D = int(round(np.sqrt(DD)))
    md = (D - 1) // 2
    out = np.zeros((B, H * W, H, W), cv.dtype)
    for r in range(H):
        for c in range(W):
            for r2 in range(max(0, r - md), min(H, r + md + 1)):
                for c2 in range(max(0, c - md), min(W, c + md + 1)):
                    out[:, r2 * W + c2, r, c] = cv[:, (r2 - r + md) * D + (c2 - c + md), r, c]
    return out


def cost_volume_shifted(cur, prev, md):
    """The displacement form (B, (2 md + 1)^2, H, W) by pad + shifted products, one displacement at a time: the same definition as
    `cost_volume`, vectorised over positions (a second at the deployed 1024 x 18 x 18, where the brute force takes ten)."""
    cur, prev = np.asarray(cur, np.float64), np.asarray(prev, np.float64)
    B, C, H, W = cur.shape
    D = 2 * md + 1
    pp = np.pad(prev, ((0, 0), (0, 0), (md, md), (md, md)))
    out = np.zeros((B, D * D, H, W))
    for di in range(D):
        for dj in range(D):
            s = np.pad(np.einsum("bchw,bchw->bhw", cur, pp[:, :, di:di + H, dj:dj + W]), ((0, 0), (1, 1), (1, 1)))
            out[:, di * D + dj] = sum(s[:, i:i + H, j:j + W] for i in range(3) for j in range(3))
    return out


def cost_volume_gram(cur, prev, md):
    """The remapped cost volume through the channel Gram matrix and its 9-tap diagonal sum, in float64: milliseconds where the brute
    force takes seconds (the predictor tests use it; test_kys_cpu checks it against the brute force)."""
    cur, prev = np.asarray(cur, np.float64), np.asarray(prev, np.float64)
    B, C, H, W = cur.shape
    out = np.zeros((B, H, W, H, W))
    for b in range(B):
        G = np.pad((prev[b].reshape(C, -1).T @ cur[b].reshape(C, -1)).reshape(H, W, H, W), ((1, 1),) * 4)
        for i in range(3):
            for j in range(3):
                out[b] += G[i:i + H, j:j + W, i:i + H, j:j + W]
    r = np.arange(H)[:, None, None, None]
    c = np.arange(W)[None, :, None, None]
    mask = (np.abs(r - np.arange(H)[None, None, :, None]) <= md) & (np.abs(c - np.arange(W)[None, None, None, :]) <= md)
    return (out * mask[None]).reshape(B, H * W, H, W)


def shift(m, s):
    """Bilinear resampling with zero padding at (y + s, x + s) of maps (..., H, W)."""
    m = np.asarray(m, np.float64)
    H, W = m.shape[-2:]
    f = int(np.floor(s))
    w1 = s - f
    p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(2, 2), (2, 2)])

    def at(dy, dx):
        return p[..., 2 + f + dy:2 + f + dy + H, 2 + f + dx:2 + f + dx + W]
    return at(0, 0) * (1 - w1) * (1 - w1) + at(0, 1) * (1 - w1) * w1 + at(1, 0) * w1 * (1 - w1) + at(1, 1) * w1 * w1


def conv3(x, w, b=None):
    """x (N, Ci, H, W), w (Co, Ci, 3, 3): zero-padded 3x3 convolution."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, Ci, H, W = x.shape
    p = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((N, w.shape[0], H, W))
    for i in range(3):
        for j in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, i, j], p[:, :, i:i + H, j:j + W])
    if b is not None:
        out += np.asarray(b, np.float64)[None, :, None, None]
    return out


def _bn(x, sd, name, eps=1e-5):
    g, be, mu, var = (np.asarray(sd[name + k], np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    return (x - mu[None, :, None, None]) / np.sqrt(var[None, :, None, None] + eps) * g[None, :, None, None] + be[None, :, None, None]


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _cvproc(x, sd, stack):
    x = np.maximum(_bn(conv3(x, sd[stack + ".0.0.weight"], sd[stack + ".0.0.bias"]), sd, stack + ".0.1"), 0)
    return _bn(conv3(x, sd[stack + ".1.0.weight"], sd[stack + ".1.0.bias"]), sd, stack + ".1.1")


def is_target(h, sd):
    t = np.maximum(conv3(h, sd["is_target_predictor.0.0.weight"], sd["is_target_predictor.0.0.bias"]), 0)
    return conv3(t, sd["is_target_predictor.1.0.weight"], sd["is_target_predictor.1.0.bias"])


def predict_response(sd, cv, dimp_score, state_prev=None, label_prev=None, dimp_thresh=None, window=None, conf_measure="max",
                     shift_px=SHIFT_PX):
    """cv (B, H*W, H, W); dimp_score, label_prev (B, 1, H, W); state_prev (B, 8, H, W) or None; window broadcastable to (B, 1, H, W).
    Returns the dict of PredictorWrapper.predict_response (without 'cost_volume') in float64."""
    cv = np.asarray(cv, np.float64)
    B, HW, H, W = cv.shape
    score = shift(dimp_score, -shift_px).reshape(B, 1, H, W)
    p1 = _softmax(_cvproc(cv.reshape(B * HW, 1, H, W), sd, "cost_volume_proc1").reshape(B * HW, HW), 1)
    z = _cvproc(p1.reshape(B * HW, 1, H, W), sd, "cost_volume_proc2").reshape(B, HW, H, W)
    w = _softmax(z, 1)
    if state_prev is None:
        h = np.tanh(conv3(shift(label_prev, -shift_px).reshape(B, 1, H, W), sd["init_hidden_state_predictor.0.0.weight"]))
    else:
        h = np.asarray(state_prev, np.float64)
    aux = {"cost_volume_processed": w.reshape(B, HW, 1, H, W), "propagation_weights": w.reshape(B, HW, 1, H, W)}
    aux["is_target"] = shift(is_target(h, sd), shift_px)
    hp = np.einsum("bqp,bdq->bdp", w.reshape(B, HW, HW), h.reshape(B, -1, HW)).reshape(B, -1, H, W)
    aux["propagated_h"] = hp
    aux["is_target_after_prop"] = shift(is_target(hp, sd), shift_px)
    parts = [hp, score]
    if conf_measure != "none":
        conf = w.max(axis=1).reshape(B, 1, H, W)
        aux["propagation_conf"] = conf
        parts.append(conf)
    x = np.concatenate(parts, 1)
    k = 0
    while f"representation_predictor.{k}.0.weight" in sd:
        x = np.maximum(conv3(x, sd[f"representation_predictor.{k}.0.weight"], sd[f"representation_predictor.{k}.0.bias"]), 0)
        k += 1
    fused = _sigmoid(conv3(x, sd["response_predictor.0.0.weight"], sd["response_predictor.0.0.bias"]))
    aux["fused_score_orig"] = fused.copy()
    if dimp_thresh is not None:
        fused = fused * (score > dimp_thresh)
    if window is not None:
        fused = fused * np.asarray(window, np.float64)
    cat = np.concatenate([score, fused], 1)
    pool = np.broadcast_to(cat.max(axis=(2, 3), keepdims=True), cat.shape)
    gin = np.concatenate([cat, pool], 1)
    xs = np.concatenate([gin, hp], 1)
    g = "state_predictor."
    r = _sigmoid(conv3(xs, sd[g + "conv_reset.weight"], sd[g + "conv_reset.bias"]))
    u = _sigmoid(conv3(xs, sd[g + "conv_update.weight"], sd[g + "conv_update.bias"]))
    n = np.tanh(conv3(np.concatenate([gin, r * hp], 1), sd[g + "conv_state_new.weight"], sd[g + "conv_state_new.bias"]))
    state = (1 - u) * hp + u * n
    aux["is_target_new"] = shift(is_target(state, sd), shift_px)
    return {"response": shift(fused, shift_px), "state_cur": state, "auxiliary_outputs": aux, "score_shifted": score}
