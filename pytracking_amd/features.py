"""Host-side mirror of the classification-feature head: `ltr/models/target_classifier/features.py:49-73`
(`residual_bottleneck`) with `ltr/models/layers/normalization.py:7-20` (`InstanceL2Norm`), for the configuration every
tracker of the reference instantiates -- no residual blocks, a final 3x3 convolution without bias, instance L2
normalisation (dimpnet.py:169-172, tompnet.py:99-102): `nn.Sequential(Conv2d, InstanceL2Norm)`, state_dict key `0.weight`.
The same two layers are the target-model head of LWL and RTS (`residual_basic_block`, features.py:9-28; lwl_net.py:173-177,
rts_net.py:294-298) and, with a stride-2 convolution, the RTS classifier head (`final_stride=2`, rts_net.py:339-344).

The returned module is an `nn.Sequential` with those two children (so checkpoints load unchanged) whose forward runs both
as one fused call of the C ABI (`pt_clf_head_f32`; `pt_feat_head_f32` at stride 2).  Inference only; other configurations
raise NotImplementedError.
"""
import torch
import torch.nn as nn

from . import _lib
from .filter import _ptr, _require_device, _stream, device_guarded, workspace


class InstanceL2Norm(nn.Module):
    """Parameter-free holder with the reference's constructor; executed inside `ClfHead`."""

    def __init__(self, size_average=True, eps=1e-5, scale=1.0):
        super().__init__()
        self.size_average = size_average
        self.eps = eps
        self.scale = scale

    def forward(self, input):
        raise NotImplementedError("InstanceL2Norm runs fused with the preceding convolution (ClfHead)")


class ClfHead(nn.Sequential):
    """Conv2d(Cin, Cout, 3, stride 1 or 2, padding=1, bias=False) -> InstanceL2Norm(size_average=True) as one device call."""

    def __init__(self, conv, norm):
        super().__init__(conv, norm)
        self._key, self._wt = None, None

    def _weight_tap_major(self):
        w = self[0].weight
        key = (w.data_ptr(), w._version)
        if key != self._key:
            with torch.no_grad():
                self._wt = w.detach().permute(0, 2, 3, 1).contiguous()      # (Cout, ky, kx, Cin)
            self._key = key
        return self._wt

    @device_guarded
    def forward(self, x):
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or self[0].weight.requires_grad)):
            raise NotImplementedError("ClfHead: the gfx950 path is inference only (eval() under torch.no_grad())")
        _require_device(x)
        lead = x.shape[:-3]
        x4 = x.reshape(-1, *x.shape[-3:]).contiguous()
        n, Cin, H, W = x4.shape
        conv, norm = self[0], self[1]
        Cout = conv.out_channels
        stride = conv.stride[0] if conv.stride[0] == conv.stride[1] else 0
        L = _lib.lib()
        nb = L.pt_clf_head_ws_bytes(n, Cin, Cout, H, W) if stride == 1 else L.pt_feat_head_ws_bytes(n, Cin, Cout, H, W, stride)
        if nb == 0:
            raise NotImplementedError("ClfHead: configuration not covered by the gfx950 kernels")
        ws = workspace(nb, x4.device)
        if stride == 1:
            out = torch.empty(n, Cout, H, W, dtype=torch.float32, device=x4.device)
            rc = L.pt_clf_head_f32(_ptr(x4), _ptr(self._weight_tap_major()), _ptr(out), n, Cin, Cout, H, W, float(norm.scale),
                                   float(norm.eps), _ptr(ws), ws.numel(), _stream())
            _lib.check(rc, "pt_clf_head_f32")
        else:
            out = torch.empty(n, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=torch.float32, device=x4.device)
            rc = L.pt_feat_head_f32(_ptr(x4), _ptr(self._weight_tap_major()), _ptr(out), n, Cin, Cout, H, W, stride,
                                    float(norm.scale), float(norm.eps), _ptr(ws), ws.numel(), _stream())
            _lib.check(rc, "pt_feat_head_f32")
        return out.reshape(*lead, *out.shape[1:])


def covered(feature_dim=256, num_blocks=1, l2norm=True, final_conv=False, norm_scale=1.0, out_dim=None, interp_cat=False,
            final_relu=False, final_pool=False, input_dim=None, final_stride=1):
    """True for the argument sets `residual_bottleneck` turns into Conv2d(3x3, no bias) + InstanceL2Norm."""
    cin = 4 * feature_dim if input_dim is None else input_dim
    cout = feature_dim if out_dim is None else out_dim
    return (num_blocks == 0 and final_conv and l2norm and not interp_cat and not final_relu and not final_pool
            and final_stride == 1 and cin % 64 == 0 and cout % 4 == 0)


def covered_strided(feature_dim=256, num_blocks=1, l2norm=True, final_conv=False, norm_scale=1.0, out_dim=None, interp_cat=False,
                    final_relu=False, final_pool=False, input_dim=None, final_stride=1):
    """`covered` plus the stride-2 final convolution (the RTS classifier head): what `install(feature_heads=True)` and the mirror take."""
    return final_stride in (1, 2) and covered(feature_dim, num_blocks, l2norm, final_conv, norm_scale, out_dim, interp_cat, final_relu,
                                              final_pool, input_dim, 1)


def covered_basic_block(feature_dim=256, num_blocks=1, l2norm=True, final_conv=False, norm_scale=1.0, out_dim=None, interp_cat=False,
                        final_relu=False, init_pool=False):
    """True for the argument sets `residual_basic_block` turns into Conv2d(3x3, no bias) + InstanceL2Norm."""
    cout = feature_dim if out_dim is None else out_dim
    return (num_blocks == 0 and final_conv and l2norm and not interp_cat and not final_relu and not init_pool
            and feature_dim % 64 == 0 and cout % 4 == 0)


def residual_bottleneck(feature_dim=256, num_blocks=1, l2norm=True, final_conv=False, norm_scale=1.0, out_dim=None,
                        interp_cat=False, final_relu=False, final_pool=False, input_dim=None, final_stride=1):
    if not covered_strided(feature_dim, num_blocks, l2norm, final_conv, norm_scale, out_dim, interp_cat, final_relu, final_pool,
                           input_dim, final_stride):
        raise NotImplementedError("residual_bottleneck: only num_blocks=0 + final 3x3 conv (stride 1 or 2) + InstanceL2Norm is on the "
                                  "hot path")
    cin = 4 * feature_dim if input_dim is None else input_dim
    cout = feature_dim if out_dim is None else out_dim
    return ClfHead(nn.Conv2d(cin, cout, kernel_size=3, padding=1, bias=False, stride=final_stride), InstanceL2Norm(scale=norm_scale))


def residual_basic_block(feature_dim=256, num_blocks=1, l2norm=True, final_conv=False, norm_scale=1.0, out_dim=None,
                         interp_cat=False, final_relu=False, init_pool=False):
    if not covered_basic_block(feature_dim, num_blocks, l2norm, final_conv, norm_scale, out_dim, interp_cat, final_relu, init_pool):
        raise NotImplementedError("residual_basic_block: only num_blocks=0 + final 3x3 conv + InstanceL2Norm is on the hot path")
    cout = feature_dim if out_dim is None else out_dim
    return ClfHead(nn.Conv2d(feature_dim, cout, kernel_size=3, padding=1, bias=False), InstanceL2Norm(scale=norm_scale))
