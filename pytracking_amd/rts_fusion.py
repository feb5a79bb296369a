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
once per module state by the recogniser and packer the label encoder uses, and cached outside the module (_packs.py: the key, and when
`refresh(module)` is needed).
"""
import torch

from . import _lib
from ._packs import CPU_TENSOR, PackCache, aligned as _aligned, conv_ok, dev_f32 as _dev_f32, ds16_channels as _channels, ds16_layers, ds16_pack, layers_key, quiet as _quiet, tap_major, tensors as _tensors
from .filter import _ptr, _stream, device_guarded
from .filter import workspace

_PACKS = PackCache()
FUSION_TYPES = {"add": _lib.PT_FUSE_ADD, "concat": _lib.PT_FUSE_CONCAT}


def _layers(module):
    """[(Conv2d, BatchNorm2d or None)] in pack order if `module` has exactly the structure of ResidualDS16SW_Clf, else None."""
    return ds16_layers(module, "ResidualDS16SW_Clf", 1)


def pack_weights(module):
    """The pt_score_enc_f32 pack of a ResidualDS16SW_Clf (float32, on its device; include/pt_hot.h): the label encoder's layout."""
    return ds16_pack(_layers(module), "pt_score_enc_pack_floats", "score encoder: the structure of ResidualDS16SW_Clf")


def _fusion_conv(fusion):
    """The Conv2d of a 'concat' LearnersFusion if it is Conv2d(2F, F, 3, padding=1, bias), else None."""
    conv = getattr(fusion, "fusion_conv1", None)
    if conv is None or not conv_ok(conv, 3, 1, True) or conv.in_channels != 2 * conv.out_channels:
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
    pack = torch.cat([tap_major(conv).reshape(-1), conv.bias.detach().float()]).contiguous()
    assert pack.numel() == n, (pack.numel(), n)
    return pack


def refresh(module):
    """Drop the packed weights of `module` (needed only after a write through `.data`, which bumps no version counter)."""
    _PACKS.drop(module)


def packed_weights(module, layers=None):
    layers = _layers(module) if layers is None else layers
    if layers is None:
        return pack_weights(module)                            # raises
    return _PACKS.get(module, layers_key(layers), pack_weights)


def packed_fusion(fusion):
    conv = _fusion_conv(fusion) if _fusion_kind(fusion) == "concat" else None
    if conv is None:
        return pack_fusion(fusion)                             # raises
    return _PACKS.get(fusion, layers_key([(conv, None)]), pack_fusion)


def encoder_covered(module, scores, feature=None) -> bool:
    layers = _layers(module)
    if layers is None or not isinstance(scores, torch.Tensor) or scores.dim() != 4:
        return False
    if not _dev_f32(scores) or scores.numel() == 0:
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
        raise RuntimeError(CPU_TENSOR)
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
        raise RuntimeError(CPU_TENSOR)
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
    if not all(_dev_f32(t) for t in tens):
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
