"""numpy restatement of the TaMOs heads (ltr/models/transformer/heads.py:119-162), in the dtype of its arguments: the two-level FPN
(torchvision's FeaturePyramidNetwork as documented: 1x1 laterals, nearest top-down resize, 3x3 output convolutions) and the
DenseBoxRegressor with T filters per sequence.  Shared by tests/tamos_heads_f64.py and the two test files; `defect` seeds one of the
mistakes the bound has to catch.  Reads nothing outside the repository.  Test infrastructure only."""
import numpy as np

DEFECTS = ("gn_eps", "halo", "stats_nobias", "nearest_round")


def conv3x3(x, w, b, pad=None):
    """x (n, C, H, W), w (O, C, 3, 3), b (O) -> (n, O, H, W); stride 1, zero padding 1 (or the per-(image, channel) value `pad`)."""
    n, C, H, W = x.shape
    xt = np.zeros((n, H + 2, W + 2, C), dtype=x.dtype)
    if pad is not None:
        xt[:] = pad.reshape(n, 1, 1, C)
    xt[:, 1:-1, 1:-1] = x.transpose(0, 2, 3, 1)
    out = np.zeros((n, H, W, w.shape[0]), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += xt[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].T
    return (out + b).transpose(0, 3, 1, 2)


def regressor(p, feat, filters, defect=None):
    """feat (n_img, D, H, W), filters (n_img, T, D) -> ltrb (n_img, T, 4, H, W)  (heads.py:119-141, `attention.dim() == 5`)"""
    dt = feat.dtype
    n_img, D, H, W = feat.shape
    T = filters.shape[1]
    eps = dt.type(2e-5 if defect == "gn_eps" else 1e-5)
    fproj = filters @ p["linear.weight"].T + p["linear.bias"]                           # (n_img, T, D)
    att = np.einsum("nchw,ntc->nthw", feat, fproj)
    x = (feat[:, None] * att[:, :, None]).reshape(n_img * T, D, H, W)
    pad = None
    for i in range(4):
        bias = p[f"tower.{3 * i}.bias"]
        x = conv3x3(x, p[f"tower.{3 * i}.weight"], bias, pad)
        s = x - bias.reshape(1, -1, 1, 1) if defect == "stats_nobias" else x
        mu = s.mean(axis=(1, 2, 3), keepdims=True)
        var = ((s - mu) ** 2).mean(axis=(1, 2, 3), keepdims=True)
        g, b = p[f"tower.{3 * i + 1}.weight"].reshape(1, -1, 1, 1), p[f"tower.{3 * i + 1}.bias"].reshape(1, -1, 1, 1)
        rstd = 1 / np.sqrt(var + eps)
        x = np.maximum((x - mu) * rstd * g + b, 0)
        if defect == "halo":                                                            # the padding normalised like a pixel of value 0
            pad = np.maximum((0 - mu) * rstd * g + b, 0).reshape(n_img * T, D)
    out = np.exp(conv3x3(x, p["bbreg_layer.weight"], p["bbreg_layer.bias"], pad))
    assert out.dtype == dt
    return out.reshape(n_img, T, 4, H, W)


def nearest_index(n_out, n_in, defect=None):
    """Source index of F.interpolate(mode='nearest', size=n_out): min(floor(dst * (float)n_in / n_out), n_in - 1), in fp32 as ATen does."""
    scale = np.float32(n_in) / np.float32(n_out)
    v = np.arange(n_out, dtype=np.float32) * scale
    idx = np.round(v) if defect == "nearest_round" else np.floor(v)
    return np.minimum(idx.astype(np.int64), n_in - 1)


def fpn(p, feat_hi, feat_lo, defect=None):
    """feat_hi (n, C_hi, H2, W2), feat_lo (n, C_lo, H3, W3) -> feat2 (n, D, H2, W2), feat3 (n, D, H3, W3)"""
    dt = feat_hi.dtype
    lat = lambda x, w, b: np.einsum("nchw,oc->nohw", x, w[:, :, 0, 0]) + b.reshape(1, -1, 1, 1)
    lat3 = lat(feat_lo, p["fpn.inner_blocks.1.0.weight"], p["fpn.inner_blocks.1.0.bias"])
    lat2 = lat(feat_hi, p["fpn.inner_blocks.0.0.weight"], p["fpn.inner_blocks.0.0.bias"])
    iy = nearest_index(feat_hi.shape[2], feat_lo.shape[2], defect)
    ix = nearest_index(feat_hi.shape[3], feat_lo.shape[3], defect)
    lat2 = lat2 + lat3[:, :, iy][:, :, :, ix]
    feat2 = conv3x3(lat2, p["fpn.layer_blocks.0.0.weight"], p["fpn.layer_blocks.0.0.bias"])
    feat3 = conv3x3(lat3, p["fpn.layer_blocks.1.0.weight"], p["fpn.layer_blocks.1.0.bias"])
    assert feat2.dtype == dt and feat3.dtype == dt
    return feat2, feat3
