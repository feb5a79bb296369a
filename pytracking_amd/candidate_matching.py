"""Target-candidate matching of KeepTrack (pytracking/tracker/keep_track/keep_track.py:437-475) on gfx950 (tcm.hip):

  find_local_maxima(scores, th, ks)        ltr.data.processing_utils.find_local_maxima          -> pt_tcm_peaks_f32
  get_descriptors(extractor, x, coords)    DescriptorExtractor.get_descriptors                   -> pt_tcm_desc_f32
  match(superglue, data)                   SuperGlue._forward ('sinkhorn', eval, batch 1)        -> pt_tcm_match_f32

Each function takes the reference's own module objects and returns the reference's types, dtypes and shapes.  `covered_*`
say whether a call runs here; install() hands every other call to the reference.

The matcher's weights are packed once per module state (BatchNorm folded into the weights, see include/pt_hot.h for the layout)
and cached outside the module (_packs.py: the key, here with the GNN layer config, and when `refresh(module)` is needed).
"""
import ctypes

import torch

from . import _lib, _packs
from ._packs import no_grad_needed as _no_grad_needed
from .filter import _ptr, _stream, device_guarded, workspace

MAX_POINTS = _lib.PT_TCM_MAX_POINTS
_PACKS = _packs.PackCache()


# ---------------------------------------------------------------------------------------------------------------------------
# local maxima

def covered_find_local_maxima(scores, th, ks) -> bool:
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32):
        return False
    if scores.dim() == 4 and scores.shape[1] != 1:           # channels are merged per image by the reference: not covered
        return False
    if scores.dim() not in (2, 4) or scores.numel() == 0 or scores.shape[-1] > 64 or scores.shape[-2] > 64:
        return False
    if not isinstance(ks, int) or isinstance(ks, bool) or ks <= 0 or ks % 2 == 0 or ks > 127:
        return False
    if not isinstance(th, (int, float)) or isinstance(th, bool):
        return False
    return _no_grad_needed(scores)


@device_guarded
def find_local_maxima(scores, th, ks):
    """reference: processing_utils.py:669-705.  Peaks sorted by value, highest first, ties in ascending raster order.  Reads the
    per-map counts back to the host (the reference's torch.nonzero synchronises in the same place)."""
    if not covered_find_local_maxima(scores, th, ks):
        raise NotImplementedError("find_local_maxima: device fp32 maps up to 64x64 (one channel), odd ks, float threshold")
    ndims = scores.dim()
    H, W = scores.shape[-2:]
    B = 1 if ndims == 2 else scores.shape[0]
    s = scores.contiguous()
    count = torch.empty(B, dtype=torch.int32, device=s.device)
    coords = torch.empty((B, H * W, 2), dtype=torch.int64, device=s.device)
    values = torch.empty((B, H * W), dtype=torch.float32, device=s.device)
    rc = _lib.lib().pt_tcm_peaks_f32(_ptr(s), B, H, W, ks, ctypes.c_float(th), _ptr(count), _ptr(coords), _ptr(values), _stream())
    _lib.check(rc, "pt_tcm_peaks_f32")
    n = count.cpu().tolist()
    if ndims == 2:
        return coords[0, :n[0]], values[0, :n[0]]
    from pytracking import TensorList
    return TensorList([coords[b, :n[b]] for b in range(B)]), TensorList([values[b, :n[b]] for b in range(B)])


# ---------------------------------------------------------------------------------------------------------------------------
# descriptors

def covered_get_descriptors(extractor, x, coords) -> bool:
    conv = getattr(extractor, "conv", None)
    if not isinstance(conv, torch.nn.Conv2d) or conv.bias is None:
        return False
    if (tuple(conv.kernel_size) != (4, 4) or tuple(conv.padding) != (2, 2) or tuple(conv.stride) != (1, 1)
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros"):
        return False
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    w = conv.weight
    if not (w.is_cuda and w.dtype == torch.float32 and conv.bias.dtype == torch.float32 and w.device == x.device):
        return False
    if x.shape[1] != w.shape[1] or w.shape[1] % 16 != 0 or w.shape[0] % 64 != 0:
        return False
    if not isinstance(coords, torch.Tensor) or coords.dtype not in (torch.int64, torch.int32) or coords.device != x.device:
        return False
    c3 = coords.unsqueeze(0) if coords.dim() == 2 else coords
    if c3.dim() != 3 or c3.shape[-1] != 2 or c3.shape[1] == 0 or c3.shape[0] not in (1, x.shape[0]):
        return False
    return _no_grad_needed(x, w, conv.bias)


@device_guarded
def get_descriptors(extractor, x, coords):
    """reference: target_candidate_matching.py:28-36 -> (B, D, P), the conv evaluated at the P points only.  The reference's
    range assertion on `coords` (a host synchronisation) is not repeated: a point outside the output map reads zeros only."""
    if not covered_get_descriptors(extractor, x, coords):
        raise NotImplementedError("get_descriptors: device fp32, 4x4 conv with padding 2 and bias, C % 16 == 0, D % 64 == 0")
    conv = extractor.conv
    B, C, H, W = x.shape
    D = conv.weight.shape[0]
    c3 = coords.unsqueeze(0) if coords.dim() == 2 else coords
    c3 = c3.expand(B, -1, -1).to(torch.int64).contiguous()
    P = c3.shape[1]
    xc = x.contiguous()
    wt = conv.weight.detach().contiguous()
    bias = conv.bias.detach().contiguous()
    out = torch.empty((B, D, P), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = workspace(L.pt_tcm_desc_ws_bytes(B, P, C, D), x.device)
    rc = L.pt_tcm_desc_f32(_ptr(xc), _ptr(wt), _ptr(bias), _ptr(c3), B, C, H, W, P, D, _ptr(out), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_tcm_desc_f32")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# matcher

def _conf_covered(sg) -> bool:
    conf = getattr(sg, "conf", None)
    if not isinstance(conf, dict):
        return False
    if conf.get("bottleneck_dim") is not None or conf.get("input_dim") != 256 or conf.get("descriptor_dim") != 256:
        return False
    if conf.get("output_normalization") != "sinkhorn" or list(conf.get("keypoint_encoder", ())) != [32, 64, 128, 256]:
        return False
    layers = [] if conf.get("skip_gnn") else list(conf.get("GNN_layers", ()))
    if len(layers) > _lib.PT_TCM_MAX_LAYERS or any(t not in ("self", "cross") for t in layers):
        return False
    return isinstance(conf.get("num_sinkhorn_iterations"), int) and conf["num_sinkhorn_iterations"] >= 0


def _kpts2(k):
    """(M, 2) view of the caller's keypoints ((M, 2) as KeepTrack passes them, or (1, M, 2)), or None."""
    if not isinstance(k, torch.Tensor) or k.dtype != torch.float32:
        return None
    if k.dim() == 3 and k.shape[0] == 1:
        k = k[0]
    return k if k.dim() == 2 and k.shape[-1] == 2 else None


def zero_keypoint_branch(data) -> bool:
    """The reference's own early return (superglue.py:304-312): a keypoint tensor whose dim 1 is empty."""
    return any(isinstance(k, torch.Tensor) and k.dim() >= 2 and k.shape[1] == 0 for k in (data.get("img_coords0"), data.get("img_coords1")))


def covered_match(sg, data) -> bool:
    if sg.training or not _conf_covered(sg):
        return False
    try:
        d0, d1 = data["descriptors0"], data["descriptors1"]
        k0, k1 = data["img_coords0"], data["img_coords1"]
        s0, s1 = data["scores0"], data["scores1"]
        z0, z1 = data["image_size0"], data["image_size1"]
    except KeyError:
        return False
    if zero_keypoint_branch(data):
        return False
    k0, k1 = _kpts2(k0), _kpts2(k1)
    if k0 is None or k1 is None:
        return False
    M, N = k0.shape[0], k1.shape[0]
    if not (1 <= M <= MAX_POINTS and 1 <= N <= MAX_POINTS):
        return False
    for z in (z0, z1):
        if not isinstance(z, (tuple, list)) or len(z) < 2:
            return False
    dev = d0.device if isinstance(d0, torch.Tensor) else None
    for t, shape in ((d0, (1, 256, M)), (d1, (1, 256, N)), (s0, None), (s1, None)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == dev):
            return False
        if shape is not None and tuple(t.shape) != shape:
            return False
    if s0.numel() != M or s1.numel() != N or k0.device != dev or k1.device != dev:
        return False
    params = list(sg.parameters())
    if any(p.device != dev or p.dtype != torch.float32 for p in params):
        return False
    return _no_grad_needed(d0, d1, k0, k1, s0, s1, *params)


def refresh(sg):
    """Drop the packed weights of `sg` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(sg)


def _fold(conv, bn=None):
    """(W, b) of a 1x1 Conv1d in float64, with an eval-mode BatchNorm1d behind it folded in."""
    w, b = _packs.bn_fold_weights(conv, bn)
    return w.reshape(w.shape[0], -1), b


def pack_weights(sg):
    """The pt_tcm_match_f32 weight pack of a SuperGlue module (float32, on its device; include/pt_hot.h)."""
    parts = []
    enc = sg.kenc.encoder
    convs = [m for m in enc if isinstance(m, torch.nn.Conv1d)]
    bns = [m for m in enc if isinstance(m, torch.nn.BatchNorm1d)]
    if len(convs) != 5 or len(bns) != 4:
        raise NotImplementedError("keypoint encoder of five layers expected")
    for i, conv in enumerate(convs):
        parts += list(_fold(conv, bns[i] if i < 4 else None))
    if not sg.conf["skip_gnn"]:
        for layer in sg.gnn.layers:
            up = layer.update
            qkv = [_fold(p) for p in up.attn.proj]
            parts += [torch.cat([w for w, _ in qkv]), torch.cat([b for _, b in qkv])]
            parts += list(_fold(up.attn.merge))
            parts += list(_fold(up.mlp[0], up.mlp[1]))
            parts += list(_fold(up.mlp[3]))
    parts += list(_fold(sg.final_proj))
    pack = torch.cat([p.reshape(-1) for p in parts]).float().contiguous()
    n_layers = 0 if sg.conf["skip_gnn"] else len(sg.gnn.layers)
    assert pack.numel() == _lib.lib().pt_tcm_match_weight_floats(n_layers)
    return pack


def packed_weights(sg):
    key = _packs.state_key(list(sg.parameters()) + list(sg.buffers()), str(sg.conf.get("GNN_layers")), bool(sg.conf.get("skip_gnn")))
    return _PACKS.get(sg, key, pack_weights)


def _kpt_norm(kpts, shape):
    """center (2) and scale of normalize_keypoints' tuple branch (superglue.py:96-107), in the reference's float32 ops."""
    h, w = shape[-2:]
    size = kpts.new_tensor([[w, h]], device="cpu")
    c = size / 2
    f = size.max(1, keepdim=True).values * 0.7
    return (float(c[0, 0]), float(c[0, 1])), float(f[0, 0])


@device_guarded
def match(sg, data, checked=False):
    """reference: SuperGlue._forward (superglue.py:299-361) -> the reference's dict: log_assignment (1, M+1, N+1), matches0 / 1
    int64 (1, M) / (1, N), match_scores0 / 1 float32, bin_score (the module's Parameter).  `checked`: the caller has just
    evaluated covered_match on these arguments (install()'s dispatcher), so it is not evaluated again."""
    if not checked and not covered_match(sg, data):
        raise NotImplementedError("SuperGlue: batch 1, eval mode, 'sinkhorn', 256-dim descriptors, 1 <= M, N <= 64, no grad")
    k0, k1 = _kpts2(data["img_coords0"]).contiguous(), _kpts2(data["img_coords1"]).contiguous()
    M, N = k0.shape[0], k1.shape[0]
    dev = k0.device
    d0, d1 = data["descriptors0"].contiguous(), data["descriptors1"].contiguous()
    s0, s1 = data["scores0"].reshape(-1).contiguous(), data["scores1"].reshape(-1).contiguous()
    pack = packed_weights(sg)
    conf = sg.conf
    layers = [] if conf["skip_gnn"] else list(conf["GNN_layers"])
    (c0, f0), (c1, f1) = _kpt_norm(k0, data["image_size0"]), _kpt_norm(k1, data["image_size1"])
    prm = _lib.TcmMatchParams(M, N, len(layers), sum(1 << i for i, t in enumerate(layers) if t == "cross"), int(bool(conf["skip_gnn"])),
                              int(conf["num_sinkhorn_iterations"]), float(conf["filter_threshold"]), (ctypes.c_float * 2)(*c0), f0,
                              (ctypes.c_float * 2)(*c1), f1, pack.numel())
    la = torch.empty((1, M + 1, N + 1), dtype=torch.float32, device=dev)
    m0 = torch.empty((1, M), dtype=torch.int64, device=dev)
    m1 = torch.empty((1, N), dtype=torch.int64, device=dev)
    ms0 = torch.empty((1, M), dtype=torch.float32, device=dev)
    ms1 = torch.empty((1, N), dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = workspace(L.pt_tcm_match_ws_bytes(ctypes.byref(prm)), dev)
    rc = L.pt_tcm_match_f32(ctypes.byref(prm), _ptr(pack), _ptr(sg.bin_score), _ptr(d0), _ptr(d1), _ptr(k0), _ptr(k1), _ptr(s0),
                            _ptr(s1), _ptr(la), _ptr(m0), _ptr(m1), _ptr(ms0), _ptr(ms1), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_tcm_match_f32")
    return {"log_assignment": la, "matches0": m0, "matches1": m1, "match_scores0": ms0, "match_scores1": ms1,
            "bin_score": sg.bin_score}
