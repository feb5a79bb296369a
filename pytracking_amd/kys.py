"""KYS state-aware response prediction (pytracking/tracker/kys/kys.py:314) on gfx950 (kys.hip):

  SpatialCorrelationSampler(3, 2 md + 1, 1, 1)    the class ltr/models/kys/cost_volume.py:5 imports         -> pt_kys_cost_volume_f32
  CostVolume(kernel_size, max_displacement, ...)  ltr.models.kys.cost_volume.CostVolume (remap fused)        -> pt_kys_cost_volume_f32
  predict_response(wrapper, data, ...)            PredictorWrapper.predict_response (eval, one reference)    -> pt_kys_predict_response_f32
                                                  representation_predictor_dims (16,) with conf_measure 'entropy' / 'max' / 'none' (the network
                                                  ltr/train_settings/kys/kys.py:110-114 trains) or (64, 32) with 'max' / 'none'

`spatial_correlation_sampler` is a CUDA extension without a ROCm build: importing ltr.models.kys fails on this platform until install()
registers this module under that name.  Its semantics are written here from the extension's documented behaviour (kernel_size 3,
stride 1, padding 1, patch_size 2 md + 1, a tap contributing only where both indices are inside the map, no normalisation); the package
is not installable next to this code, so parity of the cost volume with it is UNPINNED, as for PrRoIPool.  Everything behind the cost
volume is pinned by goldens of the unmodified reference.

Each function takes the reference's own module objects and returns the reference's types and shapes; `covered_*` say whether a call runs
here, install() hands every other call to the reference.  The predictor's weights are packed once per module state (eval BatchNorm
folded into the weights; layout in include/pt_hot.h) and cached outside the module (_packs.py: the key, here with `conf_measure`, and
when `refresh(module)` is needed).
"""
import ctypes
import warnings

import torch

from . import _lib, _packs
from ._packs import dev_f32 as _dev_f32, no_grad_needed as _no_grad_needed, one
from .filter import _ptr, _stream, device_guarded, workspace

_PACKS = _packs.PackCache()
_SHIFT_PX = []


# ---------------------------------------------------------------------------------------------------------------------------
# cost volume

def _covered_cv(feat1, feat2, kernel_size, md, stride) -> bool:
    if not (_dev_f32(feat1, 4) and _dev_f32(feat2, 4) and feat1.shape == feat2.shape and feat1.device == feat2.device):
        return False
    if kernel_size != 3 or stride != 1 or not isinstance(md, int) or md < 1 or md > 1024:
        return False
    B, C, H, W = feat1.shape
    if min(B, C, H, W) < 1 or H * W > _lib.PT_KYS_CV_MAX_HW or B > 1024:
        return False
    return _no_grad_needed(feat1, feat2)


@device_guarded
def cost_volume(feat_cur, feat_prev, max_displacement, remap=True, kernel_size=3, stride=1):
    """(B, C, H, W) x 2 -> (B, H*W, H, W) (remap: channel = previous position, zero outside the displacement window) or
    (B, (2 md + 1)^2, H, W) (channel = displacement).  Definition in include/pt_hot.h."""
    for t in (feat_cur, feat_prev):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(_packs.CPU_TENSOR)
    if not _covered_cv(feat_cur, feat_prev, kernel_size, max_displacement, stride):
        raise NotImplementedError("cost volume: device fp32 (B, C, H, W) pairs, kernel_size 3, stride 1, max_displacement >= 1, "
                                  f"H*W <= {_lib.PT_KYS_CV_MAX_HW}, no grad")
    B, C, H, W = feat_cur.shape
    md = max_displacement
    a, b = feat_cur.contiguous(), feat_prev.contiguous()
    out = torch.empty((B, H * W if remap else (2 * md + 1) ** 2, H, W), dtype=torch.float32, device=a.device)
    L = _lib.lib()
    ws = workspace(L.pt_kys_cost_volume_ws_bytes(B, C, H, W), a.device)
    rc = L.pt_kys_cost_volume_f32(_ptr(a), _ptr(b), B, C, H, W, kernel_size, md, stride, int(bool(remap)), _ptr(out), _ptr(ws), ws.numel(),
                                  _stream())
    _lib.check(rc, "pt_kys_cost_volume_f32")
    return out


class SpatialCorrelationSampler(torch.nn.Module):
    """The class cost_volume.py constructs as SpatialCorrelationSampler(kernel_size, patch_size, stride, padding) and calls as
    layer(input1, input2) -> (B, patch, patch, H, W).  Covered: kernel_size 3, stride 1, padding 1, odd patch_size >= 3, no dilation."""

    def __init__(self, kernel_size=1, patch_size=1, stride=1, padding=0, dilation=1, dilation_patch=1):
        super().__init__()
        self.kernel_size, self.patch_size, self.stride, self.padding = kernel_size, patch_size, stride, padding
        self.dilation, self.dilation_patch = dilation, dilation_patch

    def forward(self, input1, input2):
        md = _sampler_md(self)
        if md is None:
            raise NotImplementedError("SpatialCorrelationSampler: kernel_size 3, stride 1, padding 1, odd patch_size >= 3, no dilation")
        out = cost_volume(input1, input2, md, remap=False)
        return out.view(out.shape[0], self.patch_size, self.patch_size, out.shape[-2], out.shape[-1])


def _sampler_md(layer):
    """max_displacement of a sampler object this module covers (this module's class or the upstream one), else None."""
    try:
        k, p, s, pad = one(layer.kernel_size), one(layer.patch_size), one(layer.stride), one(layer.padding)
        dil, dilp = one(getattr(layer, "dilation", 1)), one(getattr(layer, "dilation_patch", 1))
    except AttributeError:
        return None
    if k != 3 or s != 1 or pad != 1 or dil != 1 or dilp != 1 or not isinstance(p, int) or p < 3 or p % 2 != 1:
        return None
    return (p - 1) // 2


class CostVolume(torch.nn.Module):
    """ltr.models.kys.cost_volume.CostVolume: same constructor, same output shapes, remap_cost_volume fused into the store."""

    def __init__(self, kernel_size, max_displacement, stride=1, abs_coordinate_output=False):
        super().__init__()
        self.correlation_layer = SpatialCorrelationSampler(kernel_size, 2 * max_displacement + 1, stride, int((kernel_size - 1) / 2))
        self.abs_coordinate_output = abs_coordinate_output

    def forward(self, feat1, feat2):
        assert feat1.dim() == 4 and feat2.dim() == 4, 'Expect 4 dimensional inputs'
        return cost_volume_forward(self, feat1, feat2)


def covered_cost_volume(cv_module, feat1, feat2) -> bool:
    md = _sampler_md(getattr(cv_module, "correlation_layer", None))
    return md is not None and _covered_cv(feat1, feat2, 3, md, 1)


def cost_volume_forward(cv_module, feat1, feat2):
    """CostVolume.forward (cost_volume.py:15-26) of a reference (or this module's) CostVolume object."""
    md = _sampler_md(cv_module.correlation_layer)
    if md is None:
        raise NotImplementedError("CostVolume: kernel_size 3, stride 1 only")
    return cost_volume(feat1, feat2, md, remap=bool(cv_module.abs_coordinate_output))


# ---------------------------------------------------------------------------------------------------------------------------
# response predictor

def shift_px():
    """Pixel offset of shift_features' 0.5 / size translation, read off the installed torch's affine_grid / grid_sample defaults
    on a CPU ramp (0.25 with align_corners=False)."""
    if not _SHIFT_PX:
        import torch.nn.functional as F
        W = 8
        ramp = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, 4, W).contiguous()
        theta = torch.tensor([[[1.0, 0.0, 0.5 / W], [0.0, 1.0, 0.5 / 4]]])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = F.grid_sample(ramp, F.affine_grid(theta, ramp.shape))
        _SHIFT_PX.append(float(out[0, 0, 1, 3] - ramp[0, 0, 1, 3]))
    return _SHIFT_PX[0]


COVERED = ("state_dim 8, gru_ksz 3, representation_predictor_dims (64, 32) with conf_measure 'max' / 'none' or (16,) with "
           "'max' / 'none' / 'entropy'")


def _conf_codes():
    return {"none": _lib.PT_KYS_CONF_NONE, "max": _lib.PT_KYS_CONF_MAX, "entropy": _lib.PT_KYS_CONF_ENTROPY}


def _dims(pred):
    """(state_dim, rep_dim0, rep_dim1 or 0, gru_ksz, conf code) of a ResponsePredictor whose structure is on the covered list of
    include/pt_hot.h, else None.  A one-layer representation stack has rep_dim1 0."""
    try:
        convs = [blk[0] for blk in pred.representation_predictor]
        gru = pred.state_predictor
        if len(convs) not in (1, 2) or not all(isinstance(c, torch.nn.Conv2d) for c in convs + [gru.conv_reset, gru.conv_update, gru.conv_state_new]):
            return None
        code = _conf_codes().get(pred.conf_measure)
        if code is None or pred.prev_max_pool_ksz != 1:
            return None
        d = (int(gru.hidden_dim), convs[0].out_channels, convs[1].out_channels if len(convs) == 2 else 0, int(gru.conv_reset.kernel_size[0]), code)
        if d[:4] == (8, 64, 32, 3):
            return d if code != _lib.PT_KYS_CONF_ENTROPY else None
        return d if d[:4] == (8, 16, 0, 3) else None
    except (AttributeError, TypeError, IndexError):
        return None


def _fold(conv, bn=None):
    w, b = _packs.bn_fold_weights(conv, bn)
    return [w] + ([b] if b is not None else [])


def pack_weights(pred):
    """The pt_kys_predict_response_f32 weight pack of a ResponsePredictor (float32, on its device; include/pt_hot.h)."""
    d = _dims(pred)
    n = _lib.lib().pt_kys_weight_floats(*d) if d is not None else 0
    if n == 0:
        raise NotImplementedError("ResponsePredictor: " + COVERED + " only")
    parts = []
    for stack in (pred.cost_volume_proc1, pred.cost_volume_proc2):
        parts += _fold(stack[0][0], stack[0][1]) + _fold(stack[1][0], stack[1][1])
    parts += _fold(pred.init_hidden_state_predictor[0][0])
    parts += _fold(pred.is_target_predictor[0][0]) + _fold(pred.is_target_predictor[1][0])
    for blk in pred.representation_predictor:
        parts += _fold(blk[0])
    parts += _fold(pred.response_predictor[0][0])
    g = pred.state_predictor
    parts += _fold(g.conv_reset) + _fold(g.conv_update) + _fold(g.conv_state_new)
    pack = torch.cat([p.reshape(-1) for p in parts]).float().contiguous()
    if pack.numel() != n:
        raise NotImplementedError("ResponsePredictor: layer shapes differ from the covered structures")
    return pack


def refresh(pred):
    """Drop the packed weights of `pred` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(pred)


def packed_weights(pred):
    return _PACKS.get(pred, _packs.state_key(list(pred.parameters()) + list(pred.buffers()), pred.conf_measure), pack_weights)


def covered_predict_response(wrapper, data, dimp_thresh=None, output_window=None) -> bool:
    pred, cvm = getattr(wrapper, "predictor", None), getattr(wrapper, "cost_volume", None)
    if pred is None or cvm is None or wrapper.training or _dims(pred) is None:
        return False
    if _lib.lib().pt_kys_weight_floats(*_dims(pred)) == 0 or not getattr(cvm, "abs_coordinate_output", False):
        return False
    try:
        feat1, feat2, score = data["feat1"], data["feat2"], data["dimp_score_cur"]
        state = data["state_prev"]
    except (KeyError, TypeError):
        return False
    label = data.get("label_prev", None)
    if not (_dev_f32(feat1) and _dev_f32(feat2) and _dev_f32(score)) or feat1.dim() < 3 or score.dim() < 2 or feat1.shape != feat2.shape:
        return False
    H, W = score.shape[-2:]
    if feat1.shape[-2:] != (H, W) or H * W > _lib.PT_KYS_PRED_MAX_HW or H * W == 0:
        return False
    B = score.numel() // (H * W)
    f1 = feat1.reshape(-1, *feat1.shape[-3:])
    if f1.shape[0] != B or not covered_cost_volume(cvm, f1, feat2.reshape(f1.shape)):
        return False
    dev = score.device
    sd = _dims(pred)[0]
    if state is None:
        if not (_dev_f32(label) and label.numel() == B * H * W and label.device == dev):
            return False
    elif not (_dev_f32(state) and state.numel() == B * sd * H * W and state.device == dev):
        return False
    if output_window is not None and not (_dev_f32(output_window) and output_window.device == dev and output_window.numel() in (H * W, B * H * W)
                                          and output_window.shape[-2:] == (H, W)):
        return False
    th = pred.dimp_thresh if dimp_thresh is None else dimp_thresh
    if th is not None and (isinstance(th, bool) or not isinstance(th, (int, float))):
        return False
    params = list(pred.parameters())
    if any(p.device != dev or p.dtype != torch.float32 for p in params) or feat1.device != dev:
        return False
    return _no_grad_needed(feat1, feat2, score, state, label, output_window, *params)


@device_guarded
def predict_response(wrapper, data, dimp_thresh=None, output_window=None, checked=False):
    """reference: PredictorWrapper.predict_response (predictor_wrapper.py:88-153) -> the reference's dict: response (the shape of
    dimp_score_cur), state_cur (B, 8, H, W), cost_volume (B, H*W, H, W), auxiliary_outputs with exactly the keys the reference fills
    ('propagation_conf' for conf_measure 'max' and 'entropy')."""
    _packs.require_device(data.get("feat1"), data.get("feat2"), data.get("dimp_score_cur"))
    if not checked and not covered_predict_response(wrapper, data, dimp_thresh, output_window):
        raise NotImplementedError(f"predict_response: eval mode, one reference frame, device fp32, {COVERED}, "
                                  f"H*W <= {_lib.PT_KYS_PRED_MAX_HW}, no grad")
    pred = wrapper.predictor
    score = data["dimp_score_cur"]
    score_shape = score.shape
    H, W = score_shape[-2:]
    HW = H * W
    B = score.numel() // HW
    dev = score.device
    feat1 = data["feat1"].reshape(-1, *data["feat1"].shape[-3:])
    feat2 = data["feat2"].reshape(feat1.shape)
    cv = cost_volume_forward(wrapper.cost_volume, feat2, feat1)           # compute_cost_volume(feat1, feat2, True): current frame first
    sdim, r0, r1, gk, with_conf = _dims(pred)
    pack = packed_weights(pred)
    state, label = data["state_prev"], data.get("label_prev", None)
    state_c = state.contiguous() if state is not None else None
    label_c = label.contiguous() if (state is None and label is not None) else None
    th = pred.dimp_thresh if dimp_thresh is None else dimp_thresh
    win = output_window.contiguous() if output_window is not None else None
    prm = _lib.KysPredictParams(B, H, W, sdim, r0, r1, gk, with_conf, int(th is not None), float(th) if th is not None else 0.0,
                                shift_px() if wrapper.fix_coordinate_shift else 0.0,
                                HW if (win is not None and win.numel() == B * HW and B > 1) else 0, pack.numel())
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
    response, state_cur = new(*score_shape), new(B, sdim, H, W)
    pw, hp, fused = new(B, HW, 1, H, W), new(B, sdim, H, W), new(B, 1, H, W)
    conf = new(B, 1, H, W) if with_conf else None
    it0, it1, it2 = new(*score_shape), new(*score_shape), new(*score_shape)
    sc = score.contiguous()
    L = _lib.lib()
    ws = workspace(L.pt_kys_predict_ws_bytes(B, H, W), dev)
    null = ctypes.c_void_p(None)
    rc = L.pt_kys_predict_response_f32(ctypes.byref(prm), _ptr(pack), _ptr(cv), _ptr(state_c) if state_c is not None else null,
                                       _ptr(label_c) if label_c is not None else null, _ptr(sc), _ptr(win) if win is not None else null,
                                       _ptr(response), _ptr(state_cur), _ptr(pw), _ptr(hp), _ptr(conf) if conf is not None else null,
                                       _ptr(fused), _ptr(it0), _ptr(it1), _ptr(it2), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_kys_predict_response_f32")
    aux = {"cost_volume_processed": pw, "is_target": it0, "propagation_weights": pw, "propagated_h": hp, "is_target_after_prop": it1}
    if conf is not None:
        aux["propagation_conf"] = conf
    aux["fused_score_orig"] = fused
    aux["is_target_new"] = it2
    return {"response": response, "state_cur": state_cur, "auxiliary_outputs": aux, "cost_volume": cv}
