"""Shared by tests/test_rts_fusion_cpu.py, tests/test_gpu_rts_fusion.py, tools/make_golden_rts_fusion.py and tools/bench_rts_fusion.py:
the golden cases (synth.SCORE_ENC_CASES, synth.LEARNERS_FUSE_CASES, chain_deployed) with their seeded states and inputs, plain-torch modules
with the layer structure of ResidualDS16SW_Clf (ltr/models/rts/label_encoder.py:57-103; resnet.py:15-53 for the block) and LearnersFusion
(ltr/models/rts/learners_fusion.py) under the reference's attribute names for the tests that must not read the reference tree, the float64
restatement of the folded-pack arithmetic and of the resize rule the kernels implement (include/pt_hot.h), and the float64 anchor of a case
(tests/f64_bound.py: bound = FACTOR x the fp32 CPU stand-in's own distance from float64).  Test infrastructure only."""
import copy
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import f64_bound
from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENC_CASES = tuple(synth.SCORE_ENC_CASES)
FUSE_CASES = tuple(synth.LEARNERS_FUSE_CASES)
FUSION_TYPES = tuple(synth.FUSION_TYPES)
CHAIN = "chain_deployed"
ENC_STATE_SEED, ENC_INPUT_SEED, FUSE_STATE_SEED, FUSE_INPUT_SEED, CHAIN_SEED = 2600, 2700, 2800, 2900, 2990
_CACHE = {}


class BasicBlock(torch.nn.Module):
    def __init__(self, cin, cout, use_bn):
        super().__init__()
        self.use_bn = use_bn
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, stride=1, padding=1, bias=False)
        self.conv2 = torch.nn.Conv2d(cout, cout, 3, stride=1, padding=1, bias=False)
        if use_bn:
            self.bn1, self.bn2 = torch.nn.BatchNorm2d(cout), torch.nn.BatchNorm2d(cout)
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = torch.nn.Conv2d(cin, cout, 3, stride=1, padding=1)

    def forward(self, x):
        out = self.conv1(x)
        out = self.relu(self.bn1(out) if self.use_bn else out)
        out = self.conv2(out)
        out = self.bn2(out) if self.use_bn else out
        return self.relu(out + self.downsample(x))


def _block(cin, cout, use_bn):
    layers = [torch.nn.Conv2d(cin, cout, 3, stride=1, padding=1)] + ([torch.nn.BatchNorm2d(cout)] if use_bn else [])
    return torch.nn.Sequential(*layers, torch.nn.ReLU(inplace=True))


class ResidualDS16SW_Clf(torch.nn.Module):
    """The layers of the reference's instance-score encoder under the reference's attribute names."""

    def __init__(self, dims, use_bn=True):
        super().__init__()
        self.conv_block = _block(1, dims[0], use_bn)
        self.pool = torch.nn.MaxPool2d(kernel_size=3, stride=1, padding=1)
        self.res1, self.res2 = BasicBlock(dims[0], dims[1], use_bn), BasicBlock(dims[1], dims[2], use_bn)
        self.label_pred = _block(dims[2], dims[3], use_bn)
        self.samp_w_pred = torch.nn.Conv2d(dims[2], dims[3], 3, padding=1)

    def forward(self, label_mask, feature=None):
        shape = label_mask.shape
        out = self.res2(self.res1(self.pool(self.conv_block(label_mask.reshape(-1, 1, *shape[-2:])))))
        enc, sw = self.label_pred(out), self.samp_w_pred(out)
        return enc.view(shape[0], shape[1], *enc.shape[-3:]), sw.view(shape[0], shape[1], *sw.shape[-3:])


class LearnersFusion(torch.nn.Module):
    """The reference's fusion module under its attribute names; `f` generalises the reference's fixed 16 channels."""

    def __init__(self, fusion_type, f=16):
        super().__init__()
        self.fusion_type = fusion_type
        if fusion_type == "concat":
            self.fusion_conv1 = torch.nn.Conv2d(2 * f, f, kernel_size=3, padding=1, stride=1)

    def forward(self, seg_learner_out, clf_learner_out):
        assert seg_learner_out.shape == clf_learner_out.shape and seg_learner_out.shape[0] == 1
        if self.fusion_type == "add":
            return seg_learner_out + clf_learner_out
        return self.fusion_conv1(torch.cat([seg_learner_out, clf_learner_out], dim=2).squeeze(0)).unsqueeze(0)


def resize(t, size):
    """ltr/models/rts/utils.py interpolate: bilinear, align_corners=False, skipped for equal sizes."""
    return t if tuple(t.shape[-2:]) == tuple(size) else F.interpolate(t, tuple(size), mode="bilinear", align_corners=False)


def fuse_standin(fusion, seg, clf):
    """What RTSNet.segment_target does between the target model and the decoder: seg (1, n, F, Ht, Wt), clf (1, n, F, Hs, Ws)."""
    return fusion(seg, resize(clf[0], seg.shape[-2:]).unsqueeze(0))


def state_tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _golden(tag):
    return dict(np.load(os.path.join(GOLDEN, f"rts_fusion_{tag}.npz")))


def _sd(g, prefix="sd."):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def enc_case(name):
    """(golden dict, n, H, W, dims, use_bn, state dict (numpy), scores (n, H, W) numpy), loaded once per session."""
    if ("enc", name) not in _CACHE:
        g = _golden("enc_" + name)
        n, H, W, dims, use_bn = synth.SCORE_ENC_CASES[name]
        assert (int(g["n"]), int(g["H"]), int(g["W"]), tuple(int(v) for v in g["dims"]), bool(g["use_bn"])) == (n, H, W, dims, use_bn)
        _CACHE[("enc", name)] = (g, n, H, W, dims, use_bn, _sd(g), synth.score_maps(int(g["input_seed"]), n, H, W))
    return _CACHE[("enc", name)]


def enc_module(name, device="cpu"):
    _, _, _, _, dims, use_bn, sd, _ = enc_case(name)
    return new_encoder(dims, use_bn, sd, device)


def new_encoder(dims, use_bn, sd, device="cpu"):
    net = ResidualDS16SW_Clf(dims, use_bn)
    net.load_state_dict(state_tensors(sd))
    return net.to(device).eval()


def fuse_case(name):
    """(golden dict, n, F, (Hs, Ws), (Ht, Wt), {fusion type: state dict}, seg (1, n, F, Ht, Wt), clf (1, n, F, Hs, Ws)), loaded once."""
    if ("fuse", name) not in _CACHE:
        g = _golden("fuse_" + name)
        n, f, source, target = synth.LEARNERS_FUSE_CASES[name]
        assert (int(g["n"]), int(g["F"]), tuple(int(v) for v in g["source"]), tuple(int(v) for v in g["target"])) == (n, f, source, target)
        seg, clf = synth.learners_fuse_inputs(int(g["input_seed"]), n, f, source, target)
        _CACHE[("fuse", name)] = (g, n, f, source, target, {"add": {}, "concat": _sd(g, "sd.concat.")}, seg, clf)
    return _CACHE[("fuse", name)]


def new_fusion(kind, f, sd, device="cpu"):
    net = LearnersFusion(kind, f)
    net.load_state_dict(state_tensors(sd))
    return net.to(device).eval()


def fuse_module(name, kind, device="cpu"):
    _, _, f, _, _, sds, _, _ = fuse_case(name)
    return new_fusion(kind, f, sds[kind], device)


def chain_case():
    """(golden dict, encoder state, {fusion type: state}, scores (1, 1, H, W), seg (1, 1, F, Ht, Wt)) of chain_deployed."""
    if CHAIN not in _CACHE:
        g = _golden(CHAIN)
        c = synth.RTS_CHAIN_CASE
        scores = synth.score_maps(int(g["input_seed"]), 1, c["H"], c["W"])[None]
        seg, _ = synth.learners_fuse_inputs(int(g["input_seed"]) + 1, 1, c["dims"][3], (c["H"], c["W"]), c["target"])
        _CACHE[CHAIN] = (g, synth.label_enc_state(int(g["state_seed"]), c["dims"], False), {"add": {}, "concat": _sd(g, "sd.concat.")}, scores, seg)
    return _CACHE[CHAIN]


def chain_standin(enc, fusion, scores, seg):
    """encoder, then resize + fusion: -> decoder input (1, 1, F, Ht, Wt)."""
    return fuse_standin(fusion, seg, enc(scores)[0])


# ---- the float64 restatements -----------------------------------------------------------------------------------------------------------
def from_pack(pack, dims, scores, dtype=torch.float64):
    """What pt_score_enc_f32 computes from its pack (include/pt_hot.h), restated with torch on the CPU in `dtype`: per layer
    conv_without_bias(x) * scale + shift on the tap-major weights, the 3/1/1 pooling between the stem and the first block, the residual of
    a block taken from the second half of its first layer.  -> (label_enc, sample_w), (n, F, H, W) numpy."""
    c0, c1, c2, f = dims
    pack = torch.as_tensor(np.asarray(pack)).to(dtype)
    at = 0

    def layer(x, cin, cout):
        nonlocal at
        w = pack[at:at + cout * 9 * cin].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
        at += cout * 9 * cin
        scale, shift = pack[at:at + cout], pack[at + cout:at + 2 * cout]
        at += 2 * cout
        return F.conv2d(x, w, None, stride=1, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    x = torch.as_tensor(np.asarray(scores)).to(dtype)[:, None]
    x = F.max_pool2d(torch.relu(layer(x, 1, c0)), 3, 1, 1)
    for cin, c in ((c0, c1), (c1, c2)):
        t = layer(x, cin, 2 * c)
        x = torch.relu(layer(torch.relu(t[:, :c]), c, c) + t[:, c:])
    t = layer(x, c2, 2 * f)
    assert at == pack.numel()
    return torch.relu(t[:, :f]).numpy(), t[:, f:].numpy()


def resize_f64(x, size):
    """The resize rule of pt_learners_fuse_f32 in float64 (numpy): src = (dst + 0.5) * (in / out) - 0.5 clamped below at 0, i0 = floor(src),
    i1 = min(i0 + 1, in - 1), weight src - i0; no antialiasing; equal sizes: the input itself."""
    x = np.asarray(x, dtype=np.float64)
    if tuple(x.shape[-2:]) == tuple(size):
        return x
    for axis, o in ((-2, size[0]), (-1, size[1])):
        i = x.shape[axis]
        s = np.maximum((np.arange(o, dtype=np.float64) + 0.5) * (i / o) - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(int), i - 1)
        i1 = np.minimum(i0 + 1, i - 1)
        lam = s - i0
        shape = [1] * x.ndim
        shape[axis] = o
        x = np.take(x, i0, axis) * (1 - lam).reshape(shape) + np.take(x, i1, axis) * lam.reshape(shape)
    return x


def fuse_from_pack(kind, pack, seg, clf):
    """What pt_learners_fuse_f32 computes, in float64: seg (n, F, Ht, Wt), clf (n, F, Hs, Ws) numpy -> (n, F, Ht, Wt) numpy."""
    seg = np.asarray(seg, dtype=np.float64)
    r = resize_f64(clf, seg.shape[-2:])
    if kind == "add":
        return seg + r
    f = seg.shape[1]
    pack = torch.as_tensor(np.asarray(pack)).double()
    w = pack[:f * 9 * 2 * f].reshape(f, 3, 3, 2 * f).permute(0, 3, 1, 2)
    return F.conv2d(torch.from_numpy(np.concatenate([seg, r], 1)), w, pack[f * 9 * 2 * f:], padding=1).numpy()


# ---- the float64 anchor -----------------------------------------------------------------------------------------------------------------
def anchor(key, run, nets, args):
    """Anchor of one case, once per session: run(nets, args) -> OrderedDict {output: tensor} is called with float64 copies of the fp32 CPU
    stand-ins `nets` and inputs `args`, and with the fp32 ones under f64_bound.THREADS threads (the count the goldens' ref_fp32_err were
    written with); ref_err = the largest |fp32 - float64| over all outputs."""
    def in_dtype(dtype):
        with torch.no_grad():
            return run(nets, args) if dtype == np.float32 else run([copy.deepcopy(m).double() for m in nets], [a.double() for a in args])
    return f64_bound.anchor(("rts_fusion",) + key, in_dtype, threads=f64_bound.THREADS)


def run_enc(nets, args):
    enc, sw = nets[0](args[0])
    return OrderedDict((("label_enc", enc), ("sample_w", sw)))


def run_fuse(nets, args):
    return OrderedDict((("decoder_input", fuse_standin(nets[0], args[0], args[1])),))


def run_chain(nets, args):
    return OrderedDict((("decoder_input", chain_standin(nets[0], nets[1], args[0], args[1])),))


def enc_anchor(name):
    scores = torch.from_numpy(enc_case(name)[7])[:, None]
    return anchor(("enc", name), run_enc, [enc_module(name)], [scores])


def fuse_anchor(name, kind):
    _, _, _, _, _, _, seg, clf = fuse_case(name)
    return anchor(("fuse", name, kind), run_fuse, [fuse_module(name, kind)], [torch.from_numpy(seg), torch.from_numpy(clf)])


def chain_modules(kind, device="cpu"):
    _, sd_enc, sds, _, _ = chain_case()
    dims = synth.RTS_CHAIN_CASE["dims"]
    return new_encoder(dims, False, sd_enc, device), new_fusion(kind, dims[3], sds[kind], device)


def chain_anchor(kind):
    _, _, _, scores, seg = chain_case()
    return anchor((CHAIN, kind), run_chain, list(chain_modules(kind)), [torch.from_numpy(scores), torch.from_numpy(seg)])
