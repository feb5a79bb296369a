"""float64 numpy restatement of AtomIoUNet.get_modulation (ltr/models/bbreg/atom_iou_net.py:138-170) as iou_mod.hip computes it: the two
3x3 convolutions only on the pixel window under each box, PrRoIPool (oracle.np_oracle.prroi_forward), fc3_1r as a linear map 9 A -> B,
the concatenation [fc3, roi4] and the two 1x1 blocks.  Every block ends in BatchNorm2d (eval) -> ReLU.  `defect` names one seeded fault
(DEFECTS) for the CPU tests that show the bound rejects it.  Test infrastructure only."""
import math

import numpy as np

from oracle import np_oracle

BN_EPS = 1e-5          # torch.nn.BatchNorm2d default, which atom_iou_net.conv() keeps
DEFECTS = ("window_short", "s4_for_level3", "cat_swapped", "fc3_shift_dropped", "box0_everywhere", "wh_as_x1y1")


def window(box, s, H, W):
    """Inclusive (x0, y0, x1, y1) of the pixels PrRoIPool can read for the xywh box at scale s on an H x W map (empty: x1 < x0 or y1 < y0)."""
    x, y, w, h = (float(v) for v in box)
    return (max(0, math.floor(x * s)), max(0, math.floor(y * s)), min(W - 1, math.ceil((x + w) * s)), min(H - 1, math.ceil((y + h) * s)))


def affine(sd, name, eps=BN_EPS, shift=True):
    """(scale, shift) of bias + eval BatchNorm of block `name`, float64"""
    g, b = sd[name + ".1.weight"].astype(np.float64), sd[name + ".1.bias"].astype(np.float64)
    m, var = sd[name + ".1.running_mean"].astype(np.float64), sd[name + ".1.running_var"].astype(np.float64)
    s = g / np.sqrt(var + eps)
    return s, ((sd[name + ".0.bias"].astype(np.float64) - m) * s + b if shift else np.zeros_like(s))


def windowed_block(x, sd, name, wins):
    """x (n, Cin, H, W) float64 -> relu(bn(conv3x3 pad 1 (x) + bias)) inside each image's window, 0 elsewhere"""
    w = sd[name + ".0.weight"].astype(np.float64)
    n, C, H, W = x.shape
    s, b = affine(sd, name)
    xp = np.zeros((n, C, H + 2, W + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    out = np.zeros((n, w.shape[0], H, W))
    for i, (x0, y0, x1, y1) in enumerate(wins):
        if x1 < x0 or y1 < y0:
            continue
        hh, ww = y1 - y0 + 1, x1 - x0 + 1
        y = np.zeros((w.shape[0], hh, ww))
        for u in range(3):
            for v in range(3):
                y += np.einsum("oc,chw->ohw", w[:, :, u, v], xp[i, :, y0 + u:y0 + u + hh, x0 + v:x0 + v + ww], optimize=True)
        out[i, :, y0:y1 + 1, x0:x1 + 1] = np.maximum(y * s[:, None, None] + b[:, None, None], 0.0)
    return out


def get_modulation(sd, feat3, feat4, bb, s3=1.0 / 8, s4=1.0 / 16, defect=None):
    """(out3 (n, P3), out4 (n, P4)) in float64 from a synth.iou_mod_state dict, the two (n, C, H, W) maps and the (n, 4) xywh boxes."""
    assert defect is None or defect in DEFECTS, defect
    bb = np.asarray(bb, dtype=np.float64)
    n = bb.shape[0]
    if defect == "box0_everywhere":
        bb = np.repeat(bb[:1], n, 0)
    if defect == "s4_for_level3":
        s3 = s4
    f3, f4 = feat3.astype(np.float64), feat4.astype(np.float64)
    wins = [[window(b, s, f.shape[2], f.shape[3]) for b in bb] for s, f in ((s3, f3), (s4, f4))]
    if defect == "window_short":
        wins = [[(x0, y0, x1 - 1, y1) for x0, y0, x1, y1 in lv] for lv in wins]
    c3, c4 = windowed_block(f3, sd, "conv3_1r", wins[0]), windowed_block(f4, sd, "conv4_1r", wins[1])
    far = bb[:, 2:4] if defect == "wh_as_x1y1" else bb[:, 0:2] + bb[:, 2:4]
    rois = np.concatenate([np.arange(n, dtype=np.float64)[:, None], bb[:, 0:2], far], 1)
    roi3 = np_oracle.prroi_forward(c3, rois, 3, 3, s3)                   # (n, A, 3, 3)
    roi4 = np_oracle.prroi_forward(c4, rois, 1, 1, s4)[:, :, 0, 0]      # (n, D)
    s, b = affine(sd, "fc3_1r", shift=defect != "fc3_shift_dropped")
    fc3 = np.maximum(np.einsum("napq,bapq->nb", roi3, sd["fc3_1r.0.weight"].astype(np.float64), optimize=True) * s + b, 0.0)
    cat = np.concatenate([roi4, fc3] if defect == "cat_swapped" else [fc3, roi4], 1)
    out = []
    for name in ("fc34_3r", "fc34_4r"):
        s, b = affine(sd, name)
        out.append(np.maximum(cat @ sd[name + ".0.weight"].astype(np.float64)[:, :, 0, 0].T * s + b, 0.0))
    return out[0], out[1]
