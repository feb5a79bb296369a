"""Fused `ltr.models.meta.steepestdescent.GNSteepestDescent` for the hinge residual
`ltr.models.target_classifier.residual_modules.LinearFilterHinge` (DiMP-simple / super-DiMP-simple, the RTS classifier branch).

The residual module is the reference's own object: it is recognised, never replaced, so its `state_dict` and attributes stay the
reference's.  `filter_reg` (a Parameter, or a plain float when `learn_filter_reg=False`), `hinge_threshold`, `activation_leak` and the
score activation (LeakyReluPar, or BentIdentPar with its `b`) are read at call time.  The reference's double-autograd formulation is
replaced by the explicit Gauss-Newton recurrence of the fused gfx950 solver (pt_gn_hinge_solve_f32); the return value keeps the
reference's form: `(meta_parameter, iterates, losses)`, TensorList in -> TensorLists out.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from .filter import _ptr, _require_device, _stream, device_guarded, workspace
from .optimizer import _host_scalar


def is_hinge_residual(res) -> bool:
    """A reference `LinearFilterHinge` (by class name and the attributes its forward reads)."""
    return (type(res).__name__ == "LinearFilterHinge" and all(hasattr(res, k) for k in
            ("filter_reg", "hinge_threshold", "activation_leak", "score_activation")))


def activation_of(res):
    """(PT_ACT_*, act_param) of the residual's score activation, or None when the kernels do not cover it."""
    act = res.score_activation
    name = type(act).__name__
    if name == "LeakyReluPar":
        return _lib.PT_ACT_RELU, 0.0
    if name == "BentIdentPar" and isinstance(getattr(act, "b", None), (int, float)):
        return _lib.PT_ACT_BENTPAR, float(act.b)
    return None


def _filter_reg(res):
    fr = res.filter_reg
    if isinstance(fr, torch.Tensor):
        return _host_scalar(res, "filter_reg")             # the trackers overwrite filter_reg[0] in place (dimp_simple.py:645-647)
    return float(fr)


def covered(res, meta_parameter, kwargs, parameter_batch_dim=0, residual_batch_dim=1) -> bool:
    """True when this call runs on the fused solver: hinge residual with a covered activation, one filter per sequence on the
    device, no gradient wanted, label and sample_weight of a shape the solver takes."""
    if not is_hinge_residual(res) or activation_of(res) is None or parameter_batch_dim != 0 or residual_batch_dim != 1:
        return False
    w = meta_parameter[0] if isinstance(meta_parameter, (list, tuple)) else meta_parameter
    feat, label, sw = kwargs.get("feat"), kwargs.get("train_label"), kwargs.get("sample_weight")
    if not all(isinstance(t, torch.Tensor) for t in (w, feat, label)):
        return False
    if isinstance(meta_parameter, (list, tuple)) and len(meta_parameter) != 1:
        return False
    if not (w.is_cuda and feat.is_cuda and label.is_cuda) or w.dtype != torch.float32 or feat.dtype != torch.float32:
        return False
    if isinstance(res.filter_reg, torch.Tensor) and not res.filter_reg.is_cuda:
        return False
    if torch.is_grad_enabled() and (w.requires_grad or feat.requires_grad or
                                    (isinstance(res.filter_reg, torch.Tensor) and res.filter_reg.requires_grad)):
        return False
    if feat.dim() not in (4, 5) or w.dim() != 4 or w.shape[-1] != w.shape[-2] or w.shape[-1] ** 2 > 16:
        return False
    n = feat.shape[0]
    S = feat.shape[1] if feat.dim() == 5 else 1
    C, H, W = feat.shape[-3:]
    K = w.shape[-1]
    if w.shape[0] != S or w.shape[1] != C:
        return False
    OH, OW = H + (K + 1) % 2, W + (K + 1) % 2
    if label.numel() != n * S * OH * OW or label.dtype != torch.float32 or label.device != feat.device:
        return False
    # None, or one weight per image broadcast over the score maps as dimp_simple.py:679 shapes it: (n, 1, 1, 1) or (n, S, 1, 1)
    if sw is not None and not (isinstance(sw, torch.Tensor) and sw.device == feat.device and sw.dtype == torch.float32
                               and sw.dim() == 4 and sw.shape[0] == n and sw.shape[1] in (1, S) and tuple(sw.shape[2:]) == (1, 1)):
        return False
    return 0 <= int(kwargs.get("_num_iter", 0)) <= 64


class GNSteepestDescent(nn.Module):
    """reference: steepestdescent.py:8-105, for a LinearFilterHinge residual module."""

    def __init__(self, residual_module, num_iter=1, compute_losses=False, detach_length=float('Inf'),
                 parameter_batch_dim=0, residual_batch_dim=0, steplength_reg=0.0):
        super().__init__()
        self.residual_module = residual_module
        self.num_iter = num_iter
        self.compute_losses = compute_losses
        self.detach_length = detach_length
        self.steplength_reg = steplength_reg
        self._parameter_batch_dim = parameter_batch_dim
        self._residual_batch_dim = residual_batch_dim
        self.last_routes = None             # per sequence, the route ("fast" / "generic") the last solve took

    @device_guarded
    def forward(self, meta_parameter, num_iter=None, *args, feat=None, bb=None, train_label=None, sample_weight=None,
                is_distractor=None):
        res = self.residual_module
        num_iter = self.num_iter if num_iter is None else num_iter
        kw = dict(feat=feat, train_label=train_label, sample_weight=sample_weight, _num_iter=num_iter)
        if args or not covered(res, meta_parameter, kw, self._parameter_batch_dim, self._residual_batch_dim):
            raise NotImplementedError("fused GNSteepestDescent covers LinearFilterHinge at inference (device fp32, K*K <= 16, "
                                      "parameter_batch_dim=0, residual_batch_dim=1, per-image or no sample_weight)")
        input_is_list = isinstance(meta_parameter, (list, tuple))
        weights = meta_parameter[0] if input_is_list else meta_parameter
        _require_device(weights, feat, train_label)
        f5 = feat if feat.dim() == 5 else feat.unsqueeze(1)
        n, S, C, H, W = f5.shape
        K = weights.shape[-1]
        OH, OW = H + (K + 1) % 2, W + (K + 1) % 2
        if f5.stride()[2:] != (H * W, W, 1) or f5.stride(0) % 4 != 0:
            f5 = f5.contiguous()
        lab = train_label.reshape(n, S, OH, OW).to(torch.float32)
        sw = None
        if sample_weight is not None:
            sw = sample_weight.reshape(n, -1).to(torch.float32)     # (n, 1): one weight per image for every sequence, or (n, S)
        act, b = activation_of(res)
        prm = _lib.GnHingeParams(act, b, float(res.hinge_threshold), float(res.activation_leak), _filter_reg(res),
                                 float(self.steplength_reg))
        L = _lib.lib()
        ws = workspace(L.pt_gn_hinge_ws_bytes(n, C, H, W, K), feat.device)
        w_in = weights.detach().to(torch.float32).contiguous()
        iters = torch.empty((S, num_iter + 1, C, K, K), dtype=torch.float32, device=feat.device)
        losses = torch.zeros((S, num_iter + 1), dtype=torch.float32, device=feat.device) if self.compute_losses else None
        keep = []
        routes = []
        for s in range(S):
            fs = f5[:, s]
            ls = lab[:, s].contiguous()
            ss = sw[:, s if sw.shape[1] > 1 else 0].contiguous() if sw is not None else None
            keep.extend((ls, ss))
            # the route the solve below takes: its own predicate on the very pointers it is handed
            routes.append("fast" if L.pt_gn_hinge_route(_ptr(fs), fs.stride(0), _ptr(w_in[s]), _ptr(iters[s]), n, C, H, W, K) == 1
                          else "generic")
            rc = L.pt_gn_hinge_solve_f32(ctypes.byref(prm), _ptr(w_in[s]), _ptr(fs), fs.stride(0), _ptr(ls),
                                         _ptr(ss) if ss is not None else None, n, C, H, W, K, int(num_iter), _ptr(iters[s]),
                                         _ptr(losses[s]) if losses is not None else None, _ptr(ws), ws.numel(), _stream())
            _lib.check(rc, "pt_gn_hinge_solve_f32")
        self.last_routes = routes
        its = [iters[:, t] for t in range(1, num_iter + 1)]
        loss_list = []
        if self.compute_losses:
            # steepestdescent.py:27-28: sum(r^2) / numel(r) over ALL sequences; the C ABI returns each sequence's value, and with
            # equal-sized sequences the overall value is their mean
            tot = losses.mean(dim=0)
            loss_list = [tot[t] for t in range(num_iter + 1)]
        if input_is_list:
            wrap = type(meta_parameter) if isinstance(meta_parameter, list) else list
            return wrap([its[-1] if its else weights]), [meta_parameter] + [wrap([w]) for w in its], loss_list
        return (its[-1] if its else weights), [weights] + its, loss_list
