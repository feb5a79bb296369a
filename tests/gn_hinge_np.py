"""Float64 numpy restatement of GNSteepestDescent on LinearFilterHinge (ltr/models/meta/steepestdescent.py:32-105,
ltr/models/target_classifier/residual_modules.py:109-135) for one sequence, written from the recurrence:
    s = F w;  m = min((label > thr) + leak, 1);  r = sw * (act(s, m) - m*label);  g = F^T(sw * act'(s, m) * r) + reg*w
    q = sw * act'(s, m) * F g;  alpha = |g|^2 / max(|q|^2 + reg|g|^2 + steplength_reg|g|^2, 1e-8);  w <- w - alpha g
    loss = (sum r^2 + reg |w|^2) / (n*OH*OW + C*K*K),   reg = filter_reg^2."""
import numpy as np


def _pad(feat, K):
    p = K // 2
    return np.pad(feat, ((0, 0), (0, 0), (p, p), (p, p)))


def corr(fp, w, OH, OW):
    """apply_filter: scores[i,y,x] = sum_{c,u,v} feat_pad[i,c,y+u,x+v] w[c,u,v]."""
    K = w.shape[-1]
    s = np.zeros((fp.shape[0], OH, OW))
    for u in range(K):
        for v in range(K):
            s += np.einsum("ncyx,c->nyx", fp[:, :, u:u + OH, v:v + OW], w[:, u, v], optimize=True)
    return s


def adj(fp, r, K):
    """apply_feat_transpose: g[c,u,v] = sum_{i,y,x} feat_pad[i,c,y+u,x+v] r[i,y,x]."""
    OH, OW = r.shape[1:]
    g = np.zeros((fp.shape[1], K, K))
    for u in range(K):
        for v in range(K):
            g[:, u, v] = np.einsum("ncyx,nyx->c", fp[:, :, u:u + OH, v:v + OW], r, optimize=True)
    return g


def act_pair(x, m, score_act, b):
    if score_act == "relu":
        return (1 - m) / 2 * np.abs(x) + (1 + m) / 2 * x, (1 - m) / 2 * np.sign(x) + (1 + m) / 2
    rt = np.sqrt(x * x + 4 * b * b)
    return (1 - m) / 2 * (rt - 2 * b) + (1 + m) / 2 * x, (1 - m) / 2 * (x / rt) + (1 + m) / 2


def gn_hinge(w0, feat, label, sw, num_iter, score_act="relu", act_param=0.0, thr=0.05, leak=0.0, filter_reg=0.1,
             steplength_reg=0.0):
    """w0 (C,K,K), feat (n,C,H,W), label (n,OH,OW), sw (n,) or None -> (iterates (T+1,C,K,K), losses (T+1,))."""
    w = w0.astype(np.float64)
    K = w.shape[-1]
    n, C, H, W = feat.shape
    OH, OW = H + (K + 1) % 2, W + (K + 1) % 2
    fp = _pad(feat.astype(np.float64), K)
    lab = label.astype(np.float64).reshape(n, OH, OW)
    m = np.minimum((lab > thr).astype(np.float64) + leak, 1.0)
    y = m * lab
    sws = (np.sqrt(1.0 / n) if sw is None else np.sqrt(sw.astype(np.float64)).reshape(n, 1, 1)) * np.ones((n, 1, 1))
    reg = float(filter_reg) ** 2
    numel = n * OH * OW + C * K * K
    its, losses = [w.copy()], []

    def loss(s, w):
        a, _ = act_pair(s, m, score_act, act_param)
        r = sws * (a - y)
        return ((r * r).sum() + reg * (w * w).sum()) / numel

    for _ in range(num_iter):
        s = corr(fp, w, OH, OW)
        a, d = act_pair(s, m, score_act, act_param)
        r = sws * (a - y)
        losses.append(((r * r).sum() + reg * (w * w).sum()) / numel)
        g = adj(fp, sws * d * r, K) + reg * w
        q = sws * d * corr(fp, g, OH, OW)
        gg = (g * g).sum()
        alpha = gg / max((q * q).sum() + reg * gg + steplength_reg * gg, 1e-8)
        w = w - alpha * g
        its.append(w.copy())
    losses.append(loss(corr(fp, w, OH, OW), w))
    return np.stack(its), np.array(losses)
