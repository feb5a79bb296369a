"""float64 numpy restatement of AtomIoUNet.get_iou_feat (ltr/models/bbreg/atom_iou_net.py:7-12, 172-179): two towers of two blocks,
each Conv2d(3x3, stride 1, padding 1, bias) -> BatchNorm2d in eval mode -> ReLU.  Test infrastructure: the goldens' `ref_fp32_err` is the
distance of the reference's own fp32 CPU output from this."""
import numpy as np

BN_EPS = 1e-5          # torch.nn.BatchNorm2d default, which atom_iou_net.conv() keeps


def block(x, sd, name, eps=BN_EPS):
    """x (n, Cin, H, W) float64 -> relu(bn(conv3x3(x) + bias)) (n, Cout, H, W) with the state-dict entries `name`.0.* / `name`.1.*."""
    w = sd[name + ".0.weight"].astype(np.float64)
    n, C, H, W = x.shape
    xp = np.zeros((n, C, H + 2, W + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    y = np.zeros((n, w.shape[0], H, W))
    for u in range(3):
        for v in range(3):
            y += np.einsum("oc,nchw->nohw", w[:, :, u, v], xp[:, :, u:u + H, v:v + W], optimize=True)
    y += sd[name + ".0.bias"].astype(np.float64)[None, :, None, None]
    g, b = sd[name + ".1.weight"].astype(np.float64), sd[name + ".1.bias"].astype(np.float64)
    m, var = sd[name + ".1.running_mean"].astype(np.float64), sd[name + ".1.running_var"].astype(np.float64)
    y = (y - m[None, :, None, None]) / np.sqrt(var + eps)[None, :, None, None] * g[None, :, None, None] + b[None, :, None, None]
    return np.maximum(y, 0.0)


def get_iou_feat(sd, feat3, feat4):
    """(c3_t, c4_t) in float64 from a synth.iou_feat_state dict and the two (n, C, H, W) maps."""
    c3 = block(block(feat3.astype(np.float64), sd, "conv3_1t"), sd, "conv3_2t")
    c4 = block(block(feat4.astype(np.float64), sd, "conv4_1t"), sd, "conv4_2t")
    return c3, c4
