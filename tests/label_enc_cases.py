"""Shared by tests/test_label_enc_cpu.py, tests/test_gpu_label_enc.py and tools/bench_label_enc.py: the golden cases
(synth.LABEL_ENC_CASES) with their seeded state and masks, a plain-torch module with the layer structure of ResidualDS16SW
(label_encoder.py:9-55; resnet.py:15-53 for the block) for the tests that must not read the reference tree, and the restatement of the
folded-pack arithmetic the kernels implement (include/pt_hot.h).  Test infrastructure only."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tuple(synth.LABEL_ENC_CASES)
_CACHE = {}


class BasicBlock(torch.nn.Module):
    def __init__(self, cin, cout, use_bn):
        super().__init__()
        self.use_bn = use_bn
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, stride=2, padding=1, bias=False)
        self.conv2 = torch.nn.Conv2d(cout, cout, 3, stride=1, padding=1, bias=False)
        if use_bn:
            self.bn1, self.bn2 = torch.nn.BatchNorm2d(cout), torch.nn.BatchNorm2d(cout)
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = torch.nn.Conv2d(cin, cout, 3, stride=2, padding=1)

    def forward(self, x):
        out = self.conv1(x)
        out = self.relu(self.bn1(out) if self.use_bn else out)
        out = self.conv2(out)
        out = self.bn2(out) if self.use_bn else out
        return self.relu(out + self.downsample(x))


def _block(cin, cout, stride, use_bn):
    layers = [torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1)] + ([torch.nn.BatchNorm2d(cout)] if use_bn else [])
    return torch.nn.Sequential(*layers, torch.nn.ReLU(inplace=True))


class ResidualDS16SW(torch.nn.Module):
    """The layers of the reference's label encoder under the reference's attribute names."""

    def __init__(self, dims, use_bn=True):
        super().__init__()
        self.conv_block = _block(1, dims[0], 2, use_bn)
        self.pool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res1, self.res2 = BasicBlock(dims[0], dims[1], use_bn), BasicBlock(dims[1], dims[2], use_bn)
        self.label_pred = _block(dims[2], dims[3], 1, use_bn)
        self.samp_w_pred = torch.nn.Conv2d(dims[2], dims[3], 3, padding=1)

    def forward(self, label_mask, feature=None):
        shape = label_mask.shape
        out = self.res2(self.res1(self.pool(self.conv_block(label_mask.reshape(-1, 1, *shape[-2:])))))
        enc, sw = self.label_pred(out), self.samp_w_pred(out)
        return enc.view(shape[0], shape[1], *enc.shape[-3:]), sw.view(shape[0], shape[1], *sw.shape[-3:])


def case(name):
    """(golden dict, n, H, W, dims, use_bn, state dict (numpy), masks (n, H, W) numpy), generated once per session."""
    if name not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, f"label_enc_{name}.npz")))
        n, H, W, dims, use_bn = synth.LABEL_ENC_CASES[name]
        assert (int(g["n"]), int(g["H"]), int(g["W"]), tuple(int(v) for v in g["dims"]), bool(g["use_bn"])) == (n, H, W, dims, use_bn)
        sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
        masks = synth.label_enc_masks(int(g["mask_seed"]), n, H, W)
        _CACHE[name] = (g, n, H, W, dims, use_bn, sd, masks)
    return _CACHE[name]


def state_tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def module(name, device="cpu"):
    _, _, _, _, dims, use_bn, sd, _ = case(name)
    net = ResidualDS16SW(dims, use_bn)
    net.load_state_dict(state_tensors(sd))
    return net.to(device).eval()


def out_hw(H, W):
    for _ in range(4):
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return H, W


def against_golden(g, enc, sw):
    """Largest |output - golden| over both outputs, (n, F, h, w) each."""
    errs = []
    for tag, c in (("label_enc", enc), ("sample_w", sw)):
        c = np.asarray(c).reshape(g[tag].shape)
        errs.append(float(np.abs(c - g[tag]).max()))
    return max(errs)


def from_pack(pack, dims, masks, dtype=torch.float64):
    """What pt_label_enc_f32 computes from its pack (include/pt_hot.h), restated with torch on the CPU in `dtype`: per layer
    conv_without_bias(x) * scale + shift on the tap-major weights, the pooling between the stem and the first block, the residual of a
    block taken from the second half of its first layer.  -> (label_enc, sample_w), (n, F, h, w) numpy."""
    c0, c1, c2, f = dims
    pack = torch.as_tensor(np.asarray(pack)).to(dtype)
    at = 0

    def layer(x, cin, cout, stride):
        nonlocal at
        w = pack[at:at + cout * 9 * cin].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
        at += cout * 9 * cin
        scale, shift = pack[at:at + cout], pack[at + cout:at + 2 * cout]
        at += 2 * cout
        return F.conv2d(x, w, None, stride=stride, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    x = torch.as_tensor(np.asarray(masks)).to(dtype)[:, None]
    x = F.max_pool2d(torch.relu(layer(x, 1, c0, 2)), 3, 2, 1)
    for cin, c in ((c0, c1), (c1, c2)):
        t = layer(x, cin, 2 * c, 2)
        x = torch.relu(layer(torch.relu(t[:, :c]), c, c, 1) + t[:, c:])
    t = layer(x, c2, 2 * f, 1)
    assert at == pack.numel()
    return torch.relu(t[:, :f]).numpy(), t[:, f:].numpy()
