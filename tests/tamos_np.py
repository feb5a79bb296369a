"""Dtype-generic numpy restatement of the TaMOs multi-object filter predictor -- GOTFilterPredictor.predict_filter /
_predict_cls_bbreg_filters_parallel (ltr/models/transformer/filter_predictor.py:180-233,245-315) with label_enc 'gaussian' and box_enc
'ltrb_token', Transformer.forward with T object queries (ltr/models/transformer/transformer.py:90-96) -- and of the multi-filter
LinearFilterClassifier (ltr/models/transformer/heads.py:93-98, ltr/models/layers/filter.py:26-27).  Built on the pieces of
oracle/tomp_oracle.py that are generic in the number of queries (mha, encoder_layer, layer_norm, posenc, box_mlp).  It computes in the
dtype of its arguments: float64 is the anchor of tests/tamos_f64.py, fp32 gives ref_err.  `defect` seeds one of the faults the CPU test
proves the bound against.  Parameters are keyed as tests/tamos_cases.py keys them ('fp.' + the reference's state_dict key, 'cls.' ...).
Reads nothing outside the repository.  Test infrastructure only."""
import numpy as np

from oracle import tomp_oracle as TO

DEFECTS = ("rotated_embeddings", "self_only", "mask_one_late", "gth_plus_one", "ln_eps")


def tokens(p, train_feat, test_feat, train_label, train_ltrb, feature_sz, defect=None):
    """feat (L, ns, D), pos (L, ns, D): filter_predictor.py:191-223"""
    nf, ns, D, H, W = train_feat.shape
    E = p["fp.query_embed_fg.weight"]
    T = E.shape[0]
    Et = np.roll(E, 1, axis=0) if defect == "rotated_embeddings" else E
    tr = train_feat.transpose(0, 3, 4, 1, 2).reshape(nf * H * W, ns, D)
    te = test_feat.transpose(0, 3, 4, 1, 2).reshape(-1, ns, D)
    lab = train_label.transpose(0, 3, 4, 1, 2).reshape(nf * H * W, ns, T)
    tr = tr + lab @ Et                                                        # sum_o label[o] E[o]
    box = train_ltrb.transpose(0, 4, 5, 1, 2, 3).reshape(nf * H * W * ns * T, 4)
    enc = TO.box_mlp(p, "fp.box_encoding.", box).reshape(nf * H * W, ns, T, D)
    tr = tr + (enc * Et[None, None]).sum(axis=2)                              # sum_o E[o] (.) MLP(ltrb[o])
    feat = np.concatenate((tr, te), axis=0)
    pe = TO.posenc(H, W, D, feature_sz, feat.dtype)
    pos = np.concatenate([pe] * (nf + 1), axis=0)[:, None, :]
    return feat, np.repeat(pos, ns, axis=1)


def decoder_layer(p, pre, tgt, memory, pos, query_pos, nhead, mask, eps, defect=None):
    """TransformerDecoderLayer.forward_post (transformer.py:224-238) for (T, B, D) queries."""
    ln = lambda x, n: TO.layer_norm(x, p[pre + n + ".weight"], p[pre + n + ".bias"], eps)
    q = tgt + query_pos
    if defect == "self_only":
        sa = np.concatenate([TO.mha(p, pre + "self_attn.", q[t:t + 1], q[t:t + 1], tgt[t:t + 1], nhead) for t in range(tgt.shape[0])], axis=0)
    else:
        sa = TO.mha(p, pre + "self_attn.", q, q, tgt, nhead)
    tgt = ln(tgt + sa, "norm1")
    tgt = ln(tgt + TO.mha(p, pre + "multihead_attn.", tgt + query_pos, memory + pos, memory, nhead, mask), "norm2")
    h = np.maximum(tgt @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"], 0.0)
    return ln(tgt + h @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"], "norm3")


def encoder_layer(p, pre, src, pos, nhead, mask, eps):
    """TransformerEncoderLayer.forward_post (transformer.py:172-180)."""
    ln = lambda x, n: TO.layer_norm(x, p[pre + n + ".weight"], p[pre + n + ".bias"], eps)
    qk = src + pos
    src = ln(src + TO.mha(p, pre + "self_attn.", qk, qk, src, nhead, mask), "norm1")
    h = np.maximum(src @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"], 0.0)
    return ln(src + h @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"], "norm2")


def transformer(p, feat, mask, pos, nhead, n_enc, n_dec, defect=None):
    """-> decoder output (T, B, D), memory (L, B, D)"""
    eps = 2e-5 if defect == "ln_eps" else 1e-5
    pre = "fp.transformer."
    E = p["fp.query_embed_fg.weight"]
    qe = np.repeat(E[:, None, :], feat.shape[1], axis=1)
    mem = feat
    for i in range(n_enc):
        mem = encoder_layer(p, f"{pre}encoder.layers.{i}.", mem, pos, nhead, mask, eps)
    tgt = np.zeros_like(qe)
    for i in range(n_dec):
        tgt = decoder_layer(p, f"{pre}decoder.layers.{i}.", tgt, mem, pos, qe, nhead, mask, eps, defect)
    return TO.layer_norm(tgt, p[pre + "decoder.norm.weight"], p[pre + "decoder.norm.bias"], eps), mem


def predict_filter(p, train_feat, test_feat, train_label, train_ltrb, nhead, n_enc, n_dec, feature_sz, defect=None):
    """-> dec (ns, T, D), enc (1, ns, D, h, w)"""
    h, w = test_feat.shape[-2:]
    feat, pos = tokens(p, train_feat, test_feat, train_label, train_ltrb, feature_sz, defect)
    dec, mem = transformer(p, feat, None, pos, nhead, n_enc, n_dec, defect)
    enc = mem[-h * w:].transpose(1, 2, 0).reshape(test_feat.shape[1], -1, h, w)[None]
    return dec.transpose(1, 0, 2), enc


def predict_cls_bbreg_filters_parallel(p, train_feat, test_feat, train_label, num_gth_frames, train_ltrb, nhead, n_enc, n_dec,
                                       feature_sz, defect=None):
    """-> cls dec (T, D), bbreg dec (T, D), cls enc (1, 1, D, h, w), bbreg enc (1, 1, D, h, w)"""
    assert train_feat.shape[1] == 1
    H, W = train_feat.shape[-2:]
    h, w = test_feat.shape[-2:]
    st = lambda a: np.concatenate((a, a), axis=1)
    feat, pos = tokens(p, st(train_feat), st(test_feat), st(train_label), st(train_ltrb), feature_sz, defect)
    L = feat.shape[0]
    g = num_gth_frames + (1 if defect == "gth_plus_one" else 0)
    mask = np.zeros((2, L), dtype=bool)
    mask[1, g * H * W + (1 if defect == "mask_one_late" else 0):L - h * w] = True
    dec, mem = transformer(p, feat, mask, pos, nhead, n_enc, n_dec, defect)
    enc = mem[-h * w:].transpose(1, 2, 0).reshape(2, -1, h, w)
    return dec[:, 0], dec[:, 1], enc[0][None, None], enc[1][None, None]


def classifier_scores(p, feat, filt):
    """LinearFilterClassifier with T filters per sequence: feat (n, ns, D, h, w), filt (ns, T, D) -> scores (n, ns, T, h, w)"""
    fproj = filt @ p["cls.linear.weight"].T + p["cls.linear.bias"]
    return np.einsum("nschw,stc->nsthw", feat, fproj)
