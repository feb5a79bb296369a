"""Shared by tests/test_box_enc_cpu.py, tests/test_gpu_box_enc.py, tools/make_golden_box_enc.py and tools/bench_box_enc.py: the golden
cases (synth.BOX_ENC_CASES, synth.BOX_CAT_ENC_CASES) with their seeded state, features and boxes; plain-torch modules with the layer
structure of ResidualDS16FeatSWBox and ResidualDS16FeatSWBoxCatMultiBlock under the reference's attribute names (label_encoder.py:58-216;
resnet.py:15-53 for the block; blocks.py:4-20 for conv_block), for the tests that must not read the reference tree; the restatement of
what the kernels compute from the pack (include/pt_hot.h); and the float64 anchor of a case.  Test infrastructure only."""
import copy
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import f64_bound
from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOX, CAT = "box_enc", "box_cat_enc"
KINDS = (BOX, CAT)
CASES = {BOX: tuple(synth.BOX_ENC_CASES), CAT: tuple(synth.BOX_CAT_ENC_CASES)}
ALL = tuple((kind, name) for kind in KINDS for name in CASES[kind])
STORED_STATE_FLOATS = 150_000          # a golden holds the state dict up to this size, beyond it the seed and a float64 checksum
THREADS = f64_bound.THREADS            # of the fp32 CPU run whose distance from float64 is ref_err
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------------
# the box-to-mask rule

def box_ints(bb):
    """(x, y, w, h) as the reference makes them: int() truncates toward zero, then int(v + 0.5) on that integer."""
    return [int(int(v) + 0.5) for v in bb]


def box_mask(bbox, sz, clamp_start, dtype=torch.float32, shift=0):
    """(n, 1, H, W): 1 on rows y : y + h and columns x : x + w of each box (Python's slices; the starts clamped at 0 with `clamp_start`).
    `shift` moves the box by that many pixels (the discrimination tests)."""
    mask = torch.zeros((len(bbox), 1, int(sz[-2]), int(sz[-1])), dtype=dtype)
    for k, bb in enumerate(bbox):
        x, y, w, h = box_ints(bb.tolist())
        x, y = x + shift, y + shift
        ys, xs = (max(0, y), max(0, x)) if clamp_start else (y, x)
        mask[k, :, ys:y + h, xs:x + w] = 1.0
    return mask


def slice_rule(start, extent, length, clamp_start):
    """pt_box_slice restated: [lo, hi) of range(length)[a : b], a = start or max(0, start), b = start + extent."""
    a, b = (max(0, start) if clamp_start else start), start + extent
    a, b = (a + length if a < 0 else a), (b + length if b < 0 else b)
    return min(max(a, 0), length), min(max(b, 0), length)


def mask_from_rule(bbox, sz, clamp_start, dtype):
    H, W = int(sz[-2]), int(sz[-1])
    mask = torch.zeros((len(bbox), 1, H, W), dtype=dtype)
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    for k, bb in enumerate(bbox):
        x, y, w, h = box_ints(bb.tolist())
        (x0, x1), (y0, y1) = slice_rule(x, w, W, clamp_start), slice_rule(y, h, H, clamp_start)
        mask[k, 0] = ((yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)).to(dtype)
    return mask


# ---------------------------------------------------------------------------------------------------------------------------
# stand-ins

class BasicBlock(torch.nn.Module):
    def __init__(self, cin, cout, stride, use_bn):
        super().__init__()
        self.use_bn = use_bn
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.conv2 = torch.nn.Conv2d(cout, cout, 3, stride=1, padding=1, bias=False)
        if use_bn:
            self.bn1, self.bn2 = torch.nn.BatchNorm2d(cout), torch.nn.BatchNorm2d(cout)
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1)

    def forward(self, x):
        out = self.conv1(x)
        out = self.relu(self.bn1(out) if self.use_bn else out)
        out = self.conv2(out)
        out = self.bn2(out) if self.use_bn else out
        return self.relu(out + self.downsample(x))


def _block(cin, cout, stride, bn, relu):
    layers = [torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1)] + ([torch.nn.BatchNorm2d(cout)] if bn else [])
    return torch.nn.Sequential(*layers, *([torch.nn.ReLU(inplace=True)] if relu else []))


class ResidualDS16FeatSWBox(torch.nn.Module):
    """The layers of the reference's class under its attribute names; label_pred keeps conv_block's default BatchNorm."""

    def __init__(self, layer_dims, feat_dim, use_final_relu=True, use_gauss=False, use_bn=False, use_sample_w=True):
        super().__init__()
        d = layer_dims
        self.use_sample_w, self.use_gauss, self.box_shift = use_sample_w, use_gauss, 0
        self.conv_block = _block(1, d[0], 2, use_bn, True)
        self.pool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res1, self.res2 = BasicBlock(d[0], d[1], 2, use_bn), BasicBlock(d[1], d[2], 2, use_bn)
        self.res3 = BasicBlock(d[2] + feat_dim, d[3], 1, use_bn)
        self.label_pred = _block(d[3], d[4], 1, True, use_final_relu)
        if use_sample_w:
            self.samp_w_pred = torch.nn.Conv2d(d[3], d[4], 3, padding=1)

    def forward(self, bb, feat, sz):
        assert bb.dim() == 3 and not self.use_gauss
        frames, seq = bb.shape[:2]
        feat = feat.reshape(-1, *feat.shape[-3:])
        mask = box_mask(bb.reshape(-1, 4), sz, True, feat.dtype, self.box_shift).to(feat.device)
        enc = self.res2(self.res1(self.pool(self.conv_block(mask))))
        out = self.res3(torch.cat((enc, feat), 1))
        label = self.label_pred(out)
        label = label.view(frames, seq, *label.shape[-3:])
        if not self.use_sample_w:
            return label, None
        sw = self.samp_w_pred(out)
        return label, sw.view(frames, seq, *sw.shape[-3:])


class ResidualDS16FeatSWBoxCatMultiBlock(torch.nn.Module):
    def __init__(self, layer_dims, feat_dim, use_final_relu=True, use_gauss=False, use_bn=True, final_bn=True):
        super().__init__()
        self.use_gauss, self.box_shift = use_gauss, 0
        ins = (feat_dim + 1,) + tuple(layer_dims[:-2])
        self.res = torch.nn.Sequential(*[BasicBlock(i, o, 1, use_bn) for i, o in zip(ins, layer_dims[:-1])])
        self.label_pred = _block(layer_dims[-2], layer_dims[-1], 1, final_bn, use_final_relu)

    def forward(self, bb, feat, sz):
        assert not self.use_gauss
        feat = feat.reshape(-1, *feat.shape[-3:])
        mask = box_mask(bb, sz, False, feat.dtype, self.box_shift).to(feat.device)
        if tuple(mask.shape[-2:]) != tuple(feat.shape[-2:]):
            mask = F.interpolate(mask, tuple(feat.shape[-2:]), mode="bilinear", align_corners=False)
        label = self.label_pred(self.res(torch.cat([feat, mask], 1)))
        return label.view(bb.shape[0], 1, *label.shape[-3:])


def build(kind, c):
    if kind == BOX:
        return ResidualDS16FeatSWBox(c["dims"], c["feat_dim"], use_final_relu=c["final_relu"], use_bn=c["use_bn"], use_sample_w=c["use_sample_w"])
    return ResidualDS16FeatSWBoxCatMultiBlock(c["dims"], c["feat_dim"], use_final_relu=c["final_relu"], use_bn=c["use_bn"], final_bn=c["final_bn"])


# ---------------------------------------------------------------------------------------------------------------------------
# cases

def config(kind, name):
    return synth.box_enc_case(name) if kind == BOX else synth.box_cat_enc_case(name)


def state(kind, c, seed):
    if kind == BOX:
        return synth.box_enc_state(seed, c["dims"], c["feat_dim"], c["use_bn"], c["use_sample_w"])
    return synth.box_cat_enc_state(seed, c["dims"], c["feat_dim"], c["use_bn"], c["final_bn"])


def checksum(sd):
    """float64 sum of (k + 1) * sum(v) over the state's tensors in key order: the regenerated state of a case is the golden's."""
    return float(sum((k + 1) * float(np.asarray(sd[key], dtype=np.float64).sum()) for k, key in enumerate(sorted(sd))))


def state_floats(sd):
    return int(sum(np.asarray(v).size for v in sd.values()))


def outputs(kind, c):
    return ("label_enc", "sample_w") if kind == BOX and c["use_sample_w"] else ("label_enc",)


def case(kind, name):
    """(golden dict, config, state dict (numpy), boxes (n, 4) float32 numpy, feat (n, C, h, w) float32 numpy), once per session."""
    if (kind, name) not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, f"{kind}_{name}.npz")))
        c = config(kind, name)
        sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
        if not sd:
            sd = state(kind, c, int(g["state_seed"]))
            assert checksum(sd) == float(g["state_checksum"]), (kind, name)
        h, w = c["feat"]
        feat = synth.box_enc_feat(int(g["feat_seed"]), c["n"], c["feat_dim"], h, w)
        boxes = np.asarray(c["boxes"], dtype=np.float32).reshape(c["n"], 4)
        assert np.array_equal(boxes, g["boxes"]) and tuple(g["label_enc"].shape) == (c["n"], c["dims"][-1], h, w)
        _CACHE[(kind, name)] = (g, c, sd, boxes, feat)
    return _CACHE[(kind, name)]


def state_tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def module(kind, name, device="cpu"):
    _, c, sd, _, _ = case(kind, name)
    net = build(kind, c)
    net.load_state_dict(state_tensors(sd))
    return net.to(device).eval()


def call_args(kind, c, boxes, feat, device="cpu", dtype=torch.float32):
    """(bb, feat, sz) as the trackers hand them over: bb (frames, 1 sequence, 4) for FeatSWBox, (N, 4) for Cat."""
    bb = torch.as_tensor(np.asarray(boxes)).to(device)
    bb = bb[:, None] if kind == BOX else bb
    return bb, torch.as_tensor(np.asarray(feat)).to(device=device, dtype=dtype), tuple(c["image"])


def run(kind, net, args, c):
    """One call -> OrderedDict {output: (n, F, h, w) tensor}."""
    with torch.no_grad():
        out = net(*args)
    out = out if kind == BOX else (out,)
    return OrderedDict((q, out[k].reshape(-1, *out[k].shape[-3:])) for k, q in enumerate(outputs(kind, c)))


def anchor(kind, name):
    """Anchor (tests/f64_bound.py) of the fp32 CPU stand-in: `want` = the same module in float64, ref_err = the fp32 run's distance from
    it with the threads pinned (the CPU convolutions block their sums by the thread count)."""
    def in_dtype(dtype):
        _, c, _, boxes, feat = case(kind, name)
        net = module(kind, name)
        if dtype == np.float32:
            return run(kind, net, call_args(kind, c, boxes, feat), c)
        return run(kind, copy.deepcopy(net).double(), call_args(kind, c, boxes, feat, dtype=torch.float64), c)
    return f64_bound.anchor(("box_enc", kind, name), in_dtype, threads=THREADS)


def shift_visible(kind, name):
    """Can the case tell a box moved by one pixel from the box itself?  FeatSWBox: some box has an edge strictly inside the image, so the
    mask changes.  Cat: the RESIZED mask changes -- its bilinear resize without antialiasing reads two rows and two columns per output
    sample, so at a ratio of 16 most box edges fall between the taps and no implementation could see them move."""
    c = config(kind, name)
    bb = torch.tensor(c["boxes"], dtype=torch.float32)
    planes = []
    for shift in (0, 1):
        m = box_mask(bb, c["image"], kind == BOX, torch.float64, shift)
        if kind == CAT and tuple(c["image"]) != tuple(c["feat"]):
            m = F.interpolate(m, tuple(c["feat"]), mode="bilinear", align_corners=False)
        planes.append(m)
    return not torch.equal(*planes)


# ---------------------------------------------------------------------------------------------------------------------------
# what the kernels compute from the pack

def from_pack(kind, pack, c, boxes, feat, dtype=torch.float64):
    """pt_box_enc_f32 / pt_box_cat_enc_f32 restated with torch on the CPU in `dtype`: per layer conv_without_bias(x) * scale + shift on the
    tap-major, zero-padded weights; the mask from the slice rule; the residual of a block from the second half of its first layer; the
    FeatSWBox res3 over [feat | trunk]; the Cat mask by the explicit bilinear rule with fp32 tap positions.  -> {output: (n, F, h, w) numpy}."""
    pack = torch.as_tensor(np.asarray(pack)).to(dtype)
    at = 0

    def layer(x, cout, stride=1, padded=True):
        nonlocal at
        cin = x.shape[1]
        cinp = -(-cin // 16) * 16 if padded else cin
        w = pack[at:at + cout * 9 * cinp].reshape(cout, 3, 3, cinp).permute(0, 3, 1, 2)
        at += cout * 9 * cinp
        assert float(w[:, cin:].abs().sum()) == 0.0
        scale, shift = pack[at:at + cout], pack[at + cout:at + 2 * cout]
        at += 2 * cout
        return F.conv2d(x, w[:, :cin], None, stride=stride, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    def block(x, c_out, stride=1, padded=True):
        t = layer(x, 2 * c_out, stride, padded)
        return torch.relu(layer(torch.relu(t[:, :c_out]), c_out, 1, padded) + t[:, c_out:])

    ft = torch.as_tensor(np.asarray(feat)).to(dtype)
    bb = torch.as_tensor(np.asarray(boxes))
    d = c["dims"]
    if kind == BOX:
        x = mask_from_rule(bb, c["image"], True, dtype)
        x = F.max_pool2d(torch.relu(layer(x, d[0], 2, False)), 3, 2, 1)
        x = block(block(x, d[1], 2, False), d[2], 2, False)
        x = block(torch.cat([ft, x], 1), d[3])
        f = d[4]
        t = layer(x, 2 * f if c["use_sample_w"] else f)
        assert at == pack.numel()
        label = torch.relu(t[:, :f]) if c["final_relu"] else t[:, :f]
        return OrderedDict([("label_enc", label.numpy())] + ([("sample_w", t[:, f:].numpy())] if c["use_sample_w"] else []))
    m = mask_from_rule(bb, c["image"], False, dtype)
    (H, W), (h, w) = c["image"], c["feat"]
    if (H, W) != (h, w):
        def taps(n_in, n_out):
            # the source coordinate and the tap weight in fp32, as the kernel (and F.interpolate on the fp32 mask) computes them
            src = torch.clamp((torch.arange(n_out, dtype=torch.float32) + 0.5) * torch.tensor(n_in / n_out, dtype=torch.float32) - 0.5, min=0)
            i0 = src.floor().long().clamp(max=n_in - 1)
            return i0, (i0 + 1).clamp(max=n_in - 1), (src - i0).to(dtype)
        y0, y1, ly = taps(H, h)
        x0, x1, lx = taps(W, w)
        rows = m[:, :, y0] * (1 - ly)[:, None] + m[:, :, y1] * ly[:, None]
        m = rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx
    x = torch.cat([ft, m], 1)
    for width in d[:-1]:
        x = block(x, width)
    t = layer(x, d[-1])
    assert at == pack.numel()
    return OrderedDict([("label_enc", (torch.relu(t) if c["final_relu"] else t).numpy())])
