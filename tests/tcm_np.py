"""Float64 numpy restatement of KeepTrack's target-candidate matching (the reference's find_local_maxima, processing_utils.py:669-705;
DescriptorExtractor.get_descriptors, target_candidate_matching.py:28-36; SuperGlue._forward, superglue.py:299-361), written from the
reference's semantics: the max-pool padding never wins, the 4x4 conv with padding 2 read at the points, the interleaved head layout
c = 4*d + head, the (y, x) / (w, h) keypoint normalisation quirk, the dustbin coupling and log-Sinkhorn, the mutual check."""
import numpy as np


def find_local_maxima(scores, th, ks):
    """scores (H, W) -> coords (P, 2) (y, x), values (P,), highest first, ties in ascending raster order."""
    s = np.asarray(scores, np.float64)
    H, W = s.shape
    r = ks // 2
    pad = np.full((H + 2 * r, W + 2 * r), -np.inf)
    pad[r:r + H, r:r + W] = s
    mx = np.full_like(s, -np.inf)
    for dy in range(ks):
        for dx in range(ks):
            mx = np.maximum(mx, pad[dy:dy + H, dx:dx + W])
    hit = (s == mx) & (s > np.float32(th))
    idx = np.flatnonzero(hit.reshape(-1))
    vals = s.reshape(-1)[idx]
    order = np.lexsort((idx, -vals))
    idx = idx[order]
    return np.stack([idx // W, idx % W], 1).astype(np.int64), vals[order]


def get_descriptors(x, weight, bias, coords):
    """x (B, C, H, W), weight (D, C, 4, 4), bias (D,), coords (B, P, 2) -> (B, D, P)."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 4, W + 4))
    xp[:, :, 2:2 + H, 2:2 + W] = x
    w = np.asarray(weight, np.float64).reshape(weight.shape[0], -1)
    out = np.empty((B, weight.shape[0], coords.shape[1]))
    for b in range(B):
        for p, (y, xx) in enumerate(coords[b]):
            out[b, :, p] = w @ xp[b, :, y:y + 4, xx:xx + 4].reshape(-1) + bias
    return out


def _conv(sd, name, x):
    w = sd[name + ".weight"].astype(np.float64)[:, :, 0]
    return w @ x + sd[name + ".bias"].astype(np.float64)[:, None]


def _bn(sd, name, x, eps=1e-5):
    g = lambda k: sd[name + "." + k].astype(np.float64)[:, None]
    return (x - g("running_mean")) / np.sqrt(g("running_var") + eps) * g("weight") + g("bias")


def _mlp(sd, prefix, convs, x):
    for k, ci in enumerate(convs):
        x = _conv(sd, f"{prefix}.{ci}", x)
        if k < len(convs) - 1:
            x = np.maximum(_bn(sd, f"{prefix}.{ci + 1}", x), 0.0)
    return x


def _normalize(kpts, shape):
    h, w = shape[-2:]
    size = np.array([[w, h]], np.float64)
    return (kpts - size / 2) / (size.max() * 0.7)


def _attn_prop(sd, p, x, src):
    q, k, v = (_conv(sd, f"{p}attn.proj.{j}", t) for j, t in enumerate((x, src, src)))
    n, m = x.shape[1], src.shape[1]
    q, k, v = q.reshape(64, 4, n), k.reshape(64, 4, m), v.reshape(64, 4, m)     # channel c = 4*d + head
    s = np.einsum("dhn,dhm->hnm", q, k) / 8.0
    s = np.exp(s - s.max(-1, keepdims=True))
    prob = s / s.sum(-1, keepdims=True)
    msg = np.einsum("hnm,dhm->dhn", prob, v).reshape(256, n)
    msg = _conv(sd, f"{p}attn.merge", msg)
    return _mlp(sd, p + "mlp", [0, 3], np.concatenate([x, msg], 0))


def _lse(a, axis):
    m = a.max(axis, keepdims=True)
    return (np.log(np.exp(a - m).sum(axis, keepdims=True)) + m).squeeze(axis)


def match(sd, layers, iters, data, filter_threshold=0.2):
    """sd: SuperGlue state (numpy); layers: GNN layer types ([] = skip_gnn); data: the KeepTrack data dict (numpy, batch 1).
    Returns (log_assignment (M+1, N+1), matches0 (M), matches1 (N), match_scores0, match_scores1, Z rows/cols for margins)."""
    d = [data["descriptors0"][0].astype(np.float64), data["descriptors1"][0].astype(np.float64)]
    for s in range(2):
        k = _normalize(data[f"img_coords{s}"].astype(np.float64), data[f"image_size{s}"])
        inp = np.concatenate([k.T, data[f"scores{s}"].astype(np.float64).reshape(1, -1)], 0)
        d[s] = d[s] + _mlp(sd, "kenc.encoder", [0, 3, 6, 9, 12], inp)
    for l, t in enumerate(layers):
        p = f"gnn.layers.{l}.update."
        src = (d[1], d[0]) if t == "cross" else (d[0], d[1])
        d = [d[0] + _attn_prop(sd, p, d[0], src[0]), d[1] + _attn_prop(sd, p, d[1], src[1])]
    md0, md1 = _conv(sd, "final_proj", d[0]), _conv(sd, "final_proj", d[1])
    sc = md0.T @ md1 / 16.0
    M, N = sc.shape
    alpha = float(sd["bin_score"])
    Z = np.full((M + 1, N + 1), alpha)
    Z[:M, :N] = sc
    norm = -np.log(M + N)
    log_mu = np.r_[np.full(M, norm), np.log(N) + norm]
    log_nu = np.r_[np.full(N, norm), np.log(M) + norm]
    u, v = np.zeros(M + 1), np.zeros(N + 1)
    for _ in range(iters):
        u = log_mu - _lse(Z + v[None, :], 1)
        v = log_nu - _lse(Z + u[:, None], 0)
    Z = Z + u[:, None] + v[None, :] - norm
    inner = Z[:M, :N]
    m0, m1 = inner.argmax(1), inner.argmax(0)
    mutual0 = m1[m0] == np.arange(M)
    mutual1 = m0[m1] == np.arange(N)
    ms0 = np.where(mutual0, np.exp(inner.max(1)), 0.0)
    ms1 = np.where(mutual1, ms0[m1], 0.0)
    valid0 = mutual0 & (ms0 > filter_threshold)
    valid1 = mutual1 & valid0[m1]
    return Z, np.where(valid0, m0, -1), np.where(valid1, m1, -1), ms0, ms1


def margins(Z, ms0, filter_threshold=0.2):
    """Conditioning of the discrete outputs: the smallest gap between each row's / column's maximum and its runner-up, and the
    smallest distance of a match score from the threshold."""
    inner = Z[:-1, :-1]
    M, N = inner.shape
    rows = np.inf if N < 2 else float(np.min(np.abs(np.diff(-np.sort(-inner, axis=1), axis=1)[:, 0])))
    cols = np.inf if M < 2 else float(np.min(np.abs(np.diff(-np.sort(-inner, axis=0), axis=0)[0, :])))
    pos = ms0[ms0 > 0]
    thr = np.inf if pos.size == 0 else float(np.min(np.abs(pos - filter_threshold)))
    return rows, cols, thr
