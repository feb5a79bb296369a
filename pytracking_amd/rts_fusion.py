"""RTS instance-score encoder and learners fusion (ltr/models/rts/label_encoder.py:57-103, ltr/models/rts/rts_net.py:219-236,
ltr/models/rts/learners_fusion.py) on gfx950 (rts_fusion.hip): what RTS.track() runs between the classifier and the decoder.

  encode(module, scores, feature=None)                          ResidualDS16SW_Clf.forward of a reference object      -> pt_score_enc_f32
  segment_target(net, target_filter, test_feat_tm, test_feat, encoded_clf_scores)
                                                                 RTSNet.segment_target: resize + LearnersFusion        -> pt_learners_fuse_f32

The encoder is the stride-1 sibling of the mask label encoder: stem (conv 1 -> C0, ReLU, 3/1/1 max-pool) in one launch with the
convolution output kept on chip, the two BasicBlocks and both heads on the fp32 MFMA: six launches.  `want_sample_w=False` skips the
sample-weight half of the heads (the tracker discards it).  `segment_target` restates the reference method: `net.target_model
.apply_target_model` and `net.decoder` are called as they are (so whatever install() bound there is used) and the bilinear resize of the
encoded scores plus the fusion ('add', or 'concat' + Conv2d(2F, F, 3, padding=1)) run in ONE launch in between.  `encoder_covered` /
`segment_covered` say whether a call runs here; install(rts_fusion=True) hands every other call to the reference.  The weights are packed
once per module state and cached outside the module exactly as the label encoder's are (key: every parameter's and buffer's (data_ptr,
_version, shape) plus the BatchNorm eps values); after a write through `.data` call `refresh(module)`.
"""
import weakref

import torch

from . import _lib
from .filter import _ptr, _stream, device_guarded
from .filter import workspace
from .label_encoder import _aligned, _bn_ok, _channels, _conv_block, _conv_ok, _folded, _one, _state_key, _tensors

_PACKS = weakref.WeakKeyDictionary()
FUSION_TYPES = {"add": _lib.PT_FUSE_ADD, "concat": _lib.PT_FUSE_CONCAT}


def _basic_block(blk):
    """[(Conv2d, BatchNorm2d or None)] x 3 -- conv1, downsample, conv2 -- of a BasicBlock(stride 1, downsample = biased 3x3 stride-1 conv)
    (ltr/models/backbone/resnet.py:15-53), else None."""
    need = ("conv1", "conv2", "downsample", "relu", "use_bn")
    if blk is None or type(blk).__name__ != "BasicBlock" or not all(hasattr(blk, a) for a in need):
        return None
    if not (_conv_ok(blk.conv1, 1, False) and _conv_ok(blk.conv2, 1, False) and _conv_ok(blk.downsample, 1, True)):
        return None
    if not isinstance(blk.relu, torch.nn.ReLU):
        return None
    c = blk.conv1.out_channels
    if (blk.conv2.in_channels, blk.conv2.out_channels, blk.downsample.in_channels, blk.downsample.out_channels) != (c, c, blk.conv1.in_channels, c):
        return None
    bn1, bn2 = (getattr(blk, "bn1", None), getattr(blk, "bn2", None)) if blk.use_bn else (None, None)
    if blk.use_bn and not (_bn_ok(bn1, c) and _bn_ok(bn2, c)):
        return None
    return [(blk.conv1, bn1), (blk.downsample, None), (blk.conv2, bn2)]


def _layers(module):
    """[(Conv2d, BatchNorm2d or None)] in pack order -- stem, res1.conv1, res1.downsample, res1.conv2, res2.conv1, res2.downsample,
    res2.conv2, label_pred, samp_w_pred -- if `module` has exactly the structure of ResidualDS16SW_Clf, else None."""
    if type(module).__name__ != "ResidualDS16SW_Clf" or not all(hasattr(module, a) for a in ("conv_block", "pool", "res1", "res2",
                                                                                             "label_pred", "samp_w_pred")):
        return None
    pool = module.pool
    if type(pool) is not torch.nn.MaxPool2d or (_one(pool.kernel_size), _one(pool.stride), _one(pool.padding), _one(pool.dilation)) != (3, 1, 1, 1):
        return None
    if pool.ceil_mode or pool.return_indices:
        return None
    stem, head = _conv_block(module.conv_block, 1, True), _conv_block(module.label_pred, 1, True)
    b1, b2 = _basic_block(module.res1), _basic_block(module.res2)
    if stem is None or head is None or b1 is None or b2 is None or not _conv_ok(module.samp_w_pred, 1, True):
        return None
    out = [stem] + b1 + b2 + [head, (module.samp_w_pred, None)]
    c0, c1, c2, f = _channels(out)
    chain = (stem[0].in_channels == 1 and b1[0][0].in_channels == c0 and b2[0][0].in_channels == c1 and head[0].in_channels == c2
             and module.samp_w_pred.in_channels == c2 and module.samp_w_pred.out_channels == f)
    return out if chain else None


def pack_weights(module):
    """The pt_score_enc_f32 pack of a ResidualDS16SW_Clf (float32, on its device; include/pt_hot.h): the label encoder's layout."""
    layers = _layers(module)
    n = _lib.lib().pt_score_enc_pack_floats(*_channels(layers)) if layers is not None else 0
    if n == 0:
        raise NotImplementedError("score encoder: the structure of ResidualDS16SW_Clf with layer dims that are multiples of 16 up to 64")
    parts = []
    for group in ([0], [1, 2], [3], [4, 5], [6], [7, 8]):              # a block's conv1 | downsample and the two heads are one layer each
        w, s, b = zip(*[_folded(*layers[k]) for k in group])
        parts += [torch.cat(w).reshape(-1), torch.cat(s), torch.cat(b)]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def _fusion_conv(fusion):
    """The Conv2d of a 'concat' LearnersFusion if it is Conv2d(2F, F, 3, padding=1, bias), else None."""
    conv = getattr(fusion, "fusion_conv1", None)
    if conv is None or not _conv_ok(conv, 1, True) or conv.in_channels != 2 * conv.out_channels:
        return None
    return conv


def _fusion_kind(fusion):
    """'add' / 'concat' for a LearnersFusion of a structure the kernels serve, else None."""
    if type(fusion).__name__ != "LearnersFusion":
        return None
    kind = getattr(fusion, "fusion_type", None)
    if kind == "add":
        return kind
    return kind if kind == "concat" and _fusion_conv(fusion) is not None else None


def pack_fusion(fusion):
    """The pt_learners_fuse_f32 pack of a 'concat' LearnersFusion: tap-major weight (F, 3, 3, 2F), then the bias (include/pt_hot.h)."""
    conv = _fusion_conv(fusion) if _fusion_kind(fusion) == "concat" else None
    n = _lib.lib().pt_learners_fuse_pack_floats(conv.out_channels) if conv is not None else 0
    if n == 0:
        raise NotImplementedError("learners fusion: a 'concat' LearnersFusion with Conv2d(2F, F, 3, padding=1), F a multiple of 16 up to 64")
    pack = torch.cat([conv.weight.detach().permute(0, 2, 3, 1).reshape(-1).float(), conv.bias.detach().float()]).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.pop(module, None)


def _cached(module, layers, make):
    key = _state_key(layers)
    hit = _PACKS.get(module)
    if hit is not None and hit[0] == key:
        return hit[1]
    pack = make(module)
    _PACKS[module] = (key, pack)
    return pack


def packed_weights(module, layers=None):
    layers = _layers(module) if layers is None else layers
    if layers is None:
        return pack_weights(module)                            # raises
    return _cached(module, layers, pack_weights)


def packed_fusion(fusion):
    conv = _fusion_conv(fusion) if _fusion_kind(fusion) == "concat" else None
    if conv is None:
        return pack_fusion(fusion)                             # raises
    return _cached(fusion, [(conv, None)], pack_fusion)


def _quiet(module, tensors, like):
    """Eval mode, everything fp32 on the device of `like`, nothing that asks for a gradient."""
    if module.training or any(m.training for m in module.modules()):
        return False
    if any(t.device != like.device or t.dtype != torch.float32 for t in tensors):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def encoder_covered(module, scores, feature=None) -> bool:
    layers = _layers(module)
    if layers is None or not isinstance(scores, torch.Tensor) or scores.dim() != 4:
        return False
    if not (scores.is_cuda and scores.dtype == torch.float32) or scores.numel() == 0:
        return False
    if not _quiet(module, _tensors(layers) + [scores], scores):
        return False
    n = scores.shape[0] * scores.shape[1]
    return _lib.lib().pt_score_enc_ws_bytes(n, scores.shape[2], scores.shape[3], *_channels(layers)) > 0


@device_guarded
def encode(module, scores, feature=None, checked=False, want_sample_w=True):
    """reference: ResidualDS16SW_Clf.forward -> (label_enc, sample_w), each (frames, seq, F, H, W); sample_w is None when it is not
    wanted."""
    if isinstance(scores, torch.Tensor) and not scores.is_cuda:
        raise RuntimeError("pytracking_amd ops run on the MI355X only (got a CPU tensor)")
    if not checked and not encoder_covered(module, scores, feature):
        raise NotImplementedError("score encoder: eval mode, device fp32 4-D score maps, no grad, the structure of ResidualDS16SW_Clf, "
                                  "layer dims multiples of 16 up to 64")
    layers = _layers(module)
    ch = _channels(layers)
    pack = packed_weights(module, layers)
    frames, seq, H, W = scores.shape
    n = frames * seq
    s = _aligned(scores)
    enc = torch.empty((frames, seq, ch[3], H, W), dtype=torch.float32, device=s.device)
    sw = torch.empty_like(enc) if want_sample_w else None
    L = _lib.lib()
    ws = workspace(L.pt_score_enc_ws_bytes(n, H, W, *ch), s.device)
    rc = L.pt_score_enc_f32(_ptr(s), _ptr(pack), _ptr(enc), _ptr(sw) if want_sample_w else None, n, H, W, *ch, _ptr(ws), ws.numel(),
                            _stream())
    _lib.check(rc, "pt_score_enc_f32")
    return enc, sw


def _fuse_ok(fusion, tensors, lead, f, target, source):
    """The shape-level part of `fuse_covered`: `lead` leading dimensions, F channels, (Ht, Wt) and (Hs, Ws)."""
    kind = _fusion_kind(fusion)
    if kind is None or not _quiet(fusion, list(fusion.parameters()) + tensors, tensors[0]):
        return False
    if kind == "concat" and (_fusion_conv(fusion).out_channels != f or _lib.lib().pt_learners_fuse_pack_floats(f) == 0):
        return False
    n = 1
    for d in lead:
        n *= d
    return 1 <= f <= 64 and 1 <= n <= 1024 and min(*target, *source) >= 1 and max(*target, *source) <= 1024


def fuse_covered(fusion, seg_enc, clf_enc) -> bool:
    """seg_enc (..., F, Ht, Wt) and clf_enc (..., F, Hs, Ws) with the same leading dimensions."""
    if not all(isinstance(t, torch.Tensor) and t.dim() >= 4 for t in (seg_enc, clf_enc)):
        return False
    if seg_enc.shape[:-2] != clf_enc.shape[:-2] or not seg_enc.is_cuda:
        return False
    return _fuse_ok(fusion, [seg_enc, clf_enc], seg_enc.shape[:-3], seg_enc.shape[-3], seg_enc.shape[-2:], clf_enc.shape[-2:])


@device_guarded
def fuse(fusion, seg_enc, clf_enc, checked=False):
    """fusion(seg_enc, bilinear resize of clf_enc to seg_enc's size), shaped as seg_enc; one launch."""
    if isinstance(seg_enc, torch.Tensor) and not seg_enc.is_cuda:
        raise RuntimeError("pytracking_amd ops run on the MI355X only (got a CPU tensor)")
    if not checked and not fuse_covered(fusion, seg_enc, clf_enc):
        raise NotImplementedError("learners fusion: eval mode, device fp32 maps with equal leading dimensions, no grad, a LearnersFusion "
                                  "of type 'add' or 'concat' (Conv2d(2F, F, 3, padding=1)), F up to 64")
    kind = _fusion_kind(fusion)
    pack = packed_fusion(fusion) if kind == "concat" else None
    seg, clf = _aligned(seg_enc), _aligned(clf_enc)
    f, (Ht, Wt), (Hs, Ws) = seg.shape[-3], seg.shape[-2:], clf.shape[-2:]
    out = torch.empty_like(seg)
    rc = _lib.lib().pt_learners_fuse_f32(_ptr(seg), _ptr(clf), _ptr(pack) if pack is not None else None, _ptr(out),
                                         seg.numel() // (f * Ht * Wt), f, Hs, Ws, Ht, Wt, FUSION_TYPES[kind], _stream())
    _lib.check(rc, "pt_learners_fuse_f32")
    return out


def segment_covered(net, target_filter, test_feat_tm, test_feat, encoded_clf_scores=None) -> bool:
    """True when `segment_target` serves this call of RTSNet.segment_target: encoded classifier scores (1 frame, 1 sequence, F, h, w)
    given, a LearnersFusion of type 'add' or 'concat', one sequence, eval mode, no grad, device fp32 tensors."""
    if encoded_clf_scores is None or not all(isinstance(t, torch.Tensor) for t in (target_filter, test_feat_tm, encoded_clf_scores)):
        return False
    if not all(hasattr(net, a) for a in ("target_model", "decoder", "fusion_module")) or net.training:
        return False
    if target_filter.dim() != 5 or test_feat_tm.dim() < 3 or encoded_clf_scores.dim() != 5:
        return False
    if target_filter.shape[0] != 1 or encoded_clf_scores.shape[1] != 1 or encoded_clf_scores.shape[2] != target_filter.shape[1]:
        return False                                           # more than one sequence, or not one encoding per target-model filter
    tens = [target_filter, test_feat_tm, encoded_clf_scores]
    if not all(t.is_cuda and t.dtype == torch.float32 for t in tens):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in tens):
        return False
    return _fuse_ok(net.fusion_module, tens, (1, 1), target_filter.shape[1], test_feat_tm.shape[-2:], encoded_clf_scores.shape[-2:])


def segment_target(net, target_filter, test_feat_tm, test_feat, encoded_clf_scores=None, checked=False):
    """reference: RTSNet.segment_target (rts_net.py:219-236) -> (mask_pred, mask_encoding_pred)."""
    if not checked and not segment_covered(net, target_filter, test_feat_tm, test_feat, encoded_clf_scores):
        raise NotImplementedError("RTSNet.segment_target: encoded classifier scores of one sequence, a LearnersFusion of type 'add' or "
                                  "'concat', eval mode, device fp32 tensors, no grad")
    assert target_filter.dim() == 5                            # seq, filters, ch, h, w
    test_feat_tm = test_feat_tm.view(1, 1, *test_feat_tm.shape[-3:])
    mask_encoding_pred = net.target_model.apply_target_model(target_filter, test_feat_tm)
    decoder_input = fuse(net.fusion_module, mask_encoding_pred, encoded_clf_scores[:1].reshape(1, 1, *encoded_clf_scores.shape[-3:]))
    mask_pred, _ = net.decoder(decoder_input, test_feat, (test_feat_tm.shape[-2] * 16, test_feat_tm.shape[-1] * 16))
    return mask_pred, mask_encoding_pred
