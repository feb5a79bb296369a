"""TEST INFRASTRUCTURE ONLY -- a plain-torch stand-in for `spatial_correlation_sampler` (a CUDA extension that cannot be installed
here), put into sys.modules before the reference's ltr.models.kys is imported so that the UNMODIFIED reference runs on CPU (goldens)
and in stock torch on the GPU (tools/bench_kys.py's comparison leg).

THIS IS THE UNPINNED PIECE: it is written from the definition in include/pt_hot.h (the extension's documented behaviour: zero padding,
a tap contributes only where both indices are inside the map, no normalisation), not checked against the extension itself."""
import sys
import types

import torch
import torch.nn.functional as F


class SpatialCorrelationSampler(torch.nn.Module):
    def __init__(self, kernel_size=1, patch_size=1, stride=1, padding=0, dilation=1, dilation_patch=1):
        super().__init__()
        assert kernel_size == 3 and stride == 1 and padding == 1 and dilation == 1 and dilation_patch == 1 and patch_size % 2 == 1
        self.kernel_size, self.patch_size, self.stride, self.padding = kernel_size, patch_size, stride, padding
        self.dilation, self.dilation_patch = dilation, dilation_patch

    def forward(self, input1, input2):
        """(B, C, H, W) x 2 -> (B, patch, patch, H, W): pad + shifted products summed over channels, then the 3x3 window sum."""
        B, C, H, W = input1.shape
        D, md = self.patch_size, (self.patch_size - 1) // 2
        p2 = F.pad(input2, (md, md, md, md))
        box = torch.ones(1, 1, 3, 3, dtype=input1.dtype, device=input1.device)
        out = input1.new_zeros(B, D, D, H, W)
        for di in range(D):
            for dj in range(D):
                s = (input1 * p2[:, :, di:di + H, dj:dj + W]).sum(dim=1, keepdim=True)
                out[:, di, dj] = F.conv2d(s, box, padding=1)[:, 0]
        return out


def register():
    """Put the stand-in under the extension's name unless something is there already."""
    if "spatial_correlation_sampler" not in sys.modules:
        m = types.ModuleType("spatial_correlation_sampler")
        m.SpatialCorrelationSampler = SpatialCorrelationSampler
        sys.modules[m.__name__] = m
    return sys.modules["spatial_correlation_sampler"]
