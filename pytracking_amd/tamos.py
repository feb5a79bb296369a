"""Host-side mirror of the TaMOs multi-object filter predictor: `GOTFilterPredictor` of
`ltr/models/transformer/filter_predictor.py:153-315`, as `ltr/models/tracking/tamosnet.py` builds it and
`pytracking/tracker/tamos/tamos.py:289-306` calls it every frame.

    GOTFilterPredictor(transformer, feature_sz, num_tokens, label_enc='gaussian', box_enc='ltrb')
        .predict_filter(train_feat, test_feat, train_label, train_ltrb_target)
        .predict_cls_bbreg_filters_parallel(train_feat, test_feat, train_label, num_gth_frames, train_ltrb_target)

Same attribute names and state_dict keys as the reference, so a reference checkpoint loads with `strict=True`.  `transformer` is the
gfx950 parameter container (`pytracking_amd.transformer.Transformer`); the torch submodules hold parameters only.  Covered:
`label_enc == 'gaussian'`, `box_enc == 'ltrb_token'` (both of `ltr/train_settings/tamos/*.py`), 1 <= num_tokens <= 16, inference.
Anything else raises NotImplementedError -- there is no stock-PyTorch fallback -- and `install(tamos=True)` never chooses this class
for it.

The mirror never writes to its inputs.  The reference does: its `train_feat_seq += ...` (filter_predictor.py:208,220) lands on a view of
the caller's `train_feat` when there is one memory frame (the permute + flatten is then a view).  The tracker never reads that tensor
again (tamos.py:296-306), so nothing depends on it.

The classifier's scores come from `pytracking_amd.transformer.LinearFilterClassifier` with T filters per sequence.

What `pytracking/tracker/tamos/tamos.py:308-317` runs behind the predictor is here as well (`ltr/models/transformer/heads.py`):

    FPN(high_res_layer='layer2', output_dim=256, input_dims=(512, 256)).forward(test_feat_enc, test_feat_backbone)   heads.py:144-162
    DenseBoxRegressor(num_channels, project_filter).forward(feat, filter) with T filters per sequence               heads.py:119-141

both on the direct 3x3 token convolution of `pytracking_amd/csrc/tomp.hip` (pt_fpn2_f32, pt_tamos_bbreg_f32).  Not here: training; the
`box_enc` / `label_enc` variants refused above; `classify_target` computing a classification FPN map it never reads when
`cls_feature_type == 'trafo'`.  What `TaMOs.track` does per object with these outputs is `pytracking_amd/tamos_readout.py`.
"""
import ctypes
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from .filter import _ptr, _require_device, _stream, device_guarded, workspace
from . import transformer as _tm
from .transformer import MLP, Transformer, _inference_only, _Pack

MAX_TOKENS = 16


def covered(transformer, feature_sz=None, num_tokens=0, label_enc="gaussian", box_enc="ltrb", *args, **kw):
    """The constructor arguments the gfx950 path takes (what `install(tamos=True)` asks before it chooses this class)."""
    return (isinstance(transformer, Transformer) and label_enc == "gaussian" and box_enc == "ltrb_token"
            and isinstance(num_tokens, int) and 1 <= num_tokens <= MAX_TOKENS)


class _SinePositionKeys(nn.Module):
    """Stands where the reference keeps `pos_encoding = PositionEmbeddingSine(...)` (filter_predictor.py:167-168): that module has no
    parameters and no buffers, so it adds no state_dict key; the table itself comes from pt_tomp_posenc_f32."""


class GOTFilterPredictor(nn.Module):
    def __init__(self, transformer, feature_sz, num_tokens, label_enc="gaussian", box_enc="ltrb"):
        super().__init__()
        if not isinstance(transformer, Transformer):
            raise NotImplementedError("GOTFilterPredictor: the transformer is not the gfx950 parameter container")
        if label_enc != "gaussian" or box_enc != "ltrb_token":
            raise NotImplementedError("GOTFilterPredictor: the gfx950 path covers label_enc='gaussian' with box_enc='ltrb_token'")
        if not 1 <= int(num_tokens) <= MAX_TOKENS:
            raise NotImplementedError(f"GOTFilterPredictor: 1 <= num_tokens <= {MAX_TOKENS} on the gfx950 path")
        self.transformer = transformer
        self.feature_sz = feature_sz
        self.num_tokens = int(num_tokens)
        self.label_enc = label_enc
        self.box_enc = box_enc
        d = self.transformer.d_model
        self.box_encoding = MLP([4, d // 4, d, d])
        self.query_embed_fg = nn.Embedding(self.num_tokens, d)
        nn.init.orthogonal_(self.query_embed_fg.weight)
        self.pos_encoding = _SinePositionKeys()
        self._pack = _Pack()
        self._pos = {}
        self._prep_key, self._prepared = None, None

    def forward(self, train_feat, test_feat, train_label, train_ltrb_target, *args, **kwargs):
        return self.predict_filter(train_feat, test_feat, train_label, train_ltrb_target, *args, **kwargs)

    # ---- plumbing (as FilterPredictor) -----------------------------------------------------------------------------
    def pack_list(self):
        be = self.box_encoding
        return self.transformer.pack_list() + [
            be[0].weight, be[0].bias, be[1].weight, be[1].bias, be[1].running_mean, be[1].running_var,
            be[3].weight, be[3].bias, be[4].weight, be[4].bias, be[4].running_mean, be[4].running_var,
            be[6].weight, be[6].bias, self.query_embed_fg.weight]

    def _params(self):
        pack = self._pack.get(self.pack_list())
        if self._prep_key != self._pack.key:                # weights changed: fold the weight-only products again
            L = _lib.lib()
            dims = self._dims(1, 1)
            n = L.pt_tamos_prepared_floats(ctypes.byref(dims), self.num_tokens)
            if n == 0:
                raise NotImplementedError("GOTFilterPredictor: configuration not covered by the gfx950 kernels")
            self._prepared = torch.empty(n, dtype=torch.float32, device=pack.device)
            _lib.check(L.pt_tamos_prepare_f32(ctypes.byref(dims), self.num_tokens, _ptr(pack), _ptr(self._prepared), _stream()),
                       "pt_tamos_prepare_f32")
            self._prep_key = self._pack.key
        return pack, self._prepared

    def _dims(self, H, W):
        t = self.transformer
        fs = self.feature_sz
        fs = max(fs) if isinstance(fs, (list, tuple)) else fs
        return _lib.TompDims(t.d_model, t.nhead, t.dim_feedforward, len(t.encoder.layers), len(t.decoder.layers), H, W, int(fs))

    @device_guarded
    def get_positional_encoding(self, feat):
        """(nframes, nseq, C, h, w) like the reference; the (h*w, C) table is computed once per map size."""
        nframes, nseq, C, h, w = feat.shape
        return self._pos_table(h, w, feat.device).t().reshape(1, 1, C, h, w).expand(nframes, nseq, C, h, w)

    def _pos_table(self, h, w, device):
        key = (h, w, device.index)
        if key not in self._pos:
            d = self._dims(h, w)
            pos = torch.empty(h * w, d.d_model, dtype=torch.float32, device=device)
            _lib.check(_lib.lib().pt_tomp_posenc_f32(_ptr(pos), h, w, d.d_model, d.max_res, _stream()), "pt_tomp_posenc_f32")
            self._pos[key] = pos
        return self._pos[key]

    @device_guarded
    def _run(self, train_feat, test_feat, train_label, train_ltrb_target, parallel, num_gth_frames):
        """-> filters (B, T, D), enc (B, D, H, W); B = n_seq, or 2 (cls, bbreg) when `parallel`.  Every refusal is raised before a launch."""
        _inference_only(self)
        T = self.num_tokens
        if train_feat.dim() == 4:
            train_feat = train_feat.unsqueeze(1)
        if test_feat.dim() == 4:
            test_feat = test_feat.unsqueeze(1)
        if train_ltrb_target.dim() == 5:
            train_ltrb_target = train_ltrb_target.unsqueeze(1)
        if train_label.dim() == 4:
            train_label = train_label.unsqueeze(1)
        _require_device(train_feat, test_feat, train_label, train_ltrb_target)
        nf, ns, D, H, W = train_feat.shape
        if test_feat.shape[0] != 1 or tuple(test_feat.shape[-2:]) != (H, W) or test_feat.shape[1] != ns:
            raise NotImplementedError("one test frame with the memory frames' map size (the tracker's configuration)")
        if D != self.transformer.d_model:
            raise ValueError("feature dimension does not match d_model")
        if tuple(train_label.shape) != (nf, ns, T, H, W) or tuple(train_ltrb_target.shape) != (nf, ns, T, 4, H, W):
            raise ValueError("train_label (n_train, n_seq, T, H, W) and train_ltrb_target (n_train, n_seq, T, 4, H, W) expected")
        if parallel and not 0 <= int(num_gth_frames) <= nf:
            raise ValueError("num_gth_frames outside [0, n_train]")
        train_feat, test_feat = train_feat.contiguous(), test_feat.contiguous()
        train_label, train_ltrb_target = train_label.contiguous(), train_ltrb_target.contiguous()
        L = _lib.lib()
        dims = self._dims(H, W)
        nb = L.pt_tamos_predict_ws_bytes(ctypes.byref(dims), T, nf, ns, int(parallel))
        if nb == 0:
            raise NotImplementedError("GOTFilterPredictor: configuration not covered by the gfx950 kernels")
        dev = train_feat.device
        ws = workspace(nb, dev)
        B = 2 if parallel else ns
        filters = torch.empty(B, T, D, dtype=torch.float32, device=dev)
        enc = torch.empty(B, D, H, W, dtype=torch.float32, device=dev)
        pack, prepared = self._params()
        rc = L.pt_tamos_predict_f32(ctypes.byref(dims), T, _ptr(pack), _ptr(prepared), _ptr(self._pos_table(H, W, dev)),
                                    _ptr(train_feat), _ptr(test_feat), _ptr(train_label), _ptr(train_ltrb_target), nf, ns,
                                    int(parallel), int(num_gth_frames), _ptr(filters), _ptr(enc), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "pt_tamos_predict_f32")
        return filters, enc

    # ---- the reference's entry points --------------------------------------------------------------------------------
    def predict_filter(self, train_feat, test_feat, train_label, train_ltrb_target, *args, **kwargs):
        """-> dec (n_seq, T, D, 1, 1), enc (1, n_seq, D, H, W)  (filter_predictor.py:228-233)"""
        filters, enc = self._run(train_feat, test_feat, train_label, train_ltrb_target, False, 0)
        return filters.reshape(filters.shape[0], filters.shape[1], filters.shape[2], 1, 1), enc.unsqueeze(0)

    def predict_cls_bbreg_filters_parallel(self, train_feat, test_feat, train_label, num_gth_frames, train_ltrb_target,
                                           *args, **kwargs):
        """-> cls dec, bbreg dec (1, T, D, 1, 1), cls enc, bbreg enc (1, 1, D, H, W)  (filter_predictor.py:306-315); with every memory
        frame a ground-truth frame, the predict_filter result four ways (:237-239)."""
        if train_feat.shape[0] == num_gth_frames:
            dec, enc = self.predict_filter(train_feat, test_feat, train_label, train_ltrb_target)
            return dec, dec, enc, enc
        filters, enc = self._run(train_feat, test_feat, train_label, train_ltrb_target, True, num_gth_frames)
        T, D = filters.shape[1:]
        return (filters[0].reshape(1, T, D, 1, 1), filters[1].reshape(1, T, D, 1, 1), enc[0][None, None], enc[1][None, None])


# ------------------------------------------------------------------------------------------------------------------
# heads.py: FPN and the multi-object box regressor
# ------------------------------------------------------------------------------------------------------------------
def _device_only(who, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise NotImplementedError(f"{who}: the gfx950 path takes device tensors only (there is no stock-PyTorch fallback)")


class _PyramidParams(nn.Module):
    """Parameter holder with the state_dict keys of torchvision's `FeaturePyramidNetwork(in_channels_list, out_channels)`:
    `inner_blocks.{i}.0.{weight,bias}` (1x1) and `layer_blocks.{i}.0.{weight,bias}` (3x3, padding 1) -- its blocks are
    `Conv2dNormActivation` with neither norm nor activation, i.e. a Sequential around one Conv2d.  Checkpoints written before that
    wrapper existed carry `inner_blocks.{i}.{weight,bias}`; they are renamed on load, as torchvision itself upgrades them."""

    def __init__(self, in_channels_list, out_channels):
        super().__init__()
        self.inner_blocks = nn.ModuleList(nn.Sequential(nn.Conv2d(c, out_channels, 1)) for c in in_channels_list)
        self.layer_blocks = nn.ModuleList(nn.Sequential(nn.Conv2d(out_channels, out_channels, 3, padding=1)) for _ in in_channels_list)
        for m in self.modules():                            # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for block in ("inner_blocks", "layer_blocks"):
            for i in range(len(self.inner_blocks)):
                for t in ("weight", "bias"):
                    old, new = f"{prefix}{block}.{i}.{t}", f"{prefix}{block}.{i}.0.{t}"
                    if old in state_dict and new not in state_dict:
                        state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class FPN(nn.Module):
    """`heads.FPN` (heads.py:144-162) without torchvision.  torchvision is not installed where this project is built, so both the
    parameter names (`fpn.inner_blocks.{0,1}.0.*`, `fpn.layer_blocks.{0,1}.0.*`, and the older `fpn.inner_blocks.{i}.*` layout) and the
    top-down arithmetic are written from torchvision's documented behaviour, not compared with a run of it:

        lat3 = inner_blocks[1](feat3);  out3 = layer_blocks[1](lat3)
        lat2 = inner_blocks[0](feat2) + F.interpolate(lat3, size=feat2.shape[-2:], mode="nearest");  out2 = layer_blocks[0](lat2)

    Two levels, inference, device tensors; anything else raises NotImplementedError before a launch.  `compute_feat3 = False` skips the
    low-resolution output map, which the tracker never reads (the reference always computes it)."""

    def __init__(self, high_res_layer="layer2", output_dim=256, input_dims=(512, 256)):
        super().__init__()
        if len(tuple(input_dims)) != 2:
            raise NotImplementedError("FPN: the gfx950 path covers the two-level pyramid of heads.FPN")
        self.high_res_layer = high_res_layer
        self.output_dim = int(output_dim)
        self.input_dims = tuple(int(c) for c in input_dims)
        if _lib.lib().pt_fpn2_param_floats(self.input_dims[0], self.input_dims[1], self.output_dim) == 0:
            raise NotImplementedError("FPN: channel counts outside the gfx950 kernels (multiples of 64, output_dim <= 512)")
        self.fpn = _PyramidParams(self.input_dims, self.output_dim)
        self.compute_feat3 = True
        self._pack = _Pack()

    def _params(self):
        f = self.fpn
        return self._pack.get([f.inner_blocks[0][0].weight, f.inner_blocks[0][0].bias, f.inner_blocks[1][0].weight, f.inner_blocks[1][0].bias,
                               f.layer_blocks[0][0].weight.permute(0, 2, 3, 1), f.layer_blocks[0][0].bias,
                               f.layer_blocks[1][0].weight.permute(0, 2, 3, 1), f.layer_blocks[1][0].bias])

    @device_guarded
    def forward(self, test_feat_enc, test_feat_backbone):
        _inference_only(self)
        num_sequences = test_feat_enc.shape[1]
        lo = test_feat_enc.reshape(-1, *test_feat_enc.shape[-3:])
        hi = test_feat_backbone[self.high_res_layer]
        if hi.dim() == 5:
            hi = hi.reshape(-1, *hi.shape[-3:])
        _device_only("FPN", lo, hi)
        _require_device(lo, hi)
        n, c_lo, h3, w3 = lo.shape
        if hi.dim() != 4 or hi.shape[0] != n or (hi.shape[1], c_lo) != self.input_dims:
            raise ValueError("FPN: maps do not match input_dims / each other's batch")
        c_hi, h2, w2 = hi.shape[1:]
        D = self.output_dim
        L = _lib.lib()
        nb = L.pt_fpn2_ws_bytes(n, c_hi, c_lo, D, h2, w2, h3, w3)
        if nb == 0:
            raise NotImplementedError("FPN: configuration not covered by the gfx950 kernels")
        lo, hi = lo.contiguous(), hi.contiguous()
        dev = lo.device
        ws = workspace(nb, dev)
        feat2 = torch.empty(n, D, h2, w2, dtype=torch.float32, device=dev)
        feat3 = torch.empty(n, D, h3, w3, dtype=torch.float32, device=dev) if self.compute_feat3 else None
        rc = L.pt_fpn2_f32(_ptr(self._params()), _ptr(hi), _ptr(lo), _ptr(feat2), _ptr(feat3) if feat3 is not None else None, n, c_hi,
                           c_lo, D, h2, w2, h3, w3, int(feat3 is not None), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "pt_fpn2_f32")
        out = OrderedDict()
        out["feat2"] = feat2.reshape(-1, num_sequences, D, h2, w2)
        if feat3 is not None:
            out["feat3"] = feat3.reshape(-1, num_sequences, D, h3, w3)
        return out


def regressor_covered(num_channels, project_filter=True, *args, **kw):
    """The constructor arguments the gfx950 regressor takes (what `install(tamos=True)` asks before it chooses the class below)."""
    return isinstance(num_channels, int) and num_channels % 64 == 0 and 0 < num_channels <= 512


class DenseBoxRegressor(_tm.DenseBoxRegressor):
    """`heads.DenseBoxRegressor` with one filter per sequence (the parent's path, unchanged) or T filters per sequence
    (heads.py:127-141): feat (nf, ns, C, h, w), filter (ns, T, C, 1, 1) -> ltrb (1, nf*ns, T, 4, h, w).  Same state_dict keys as the
    parent and the reference."""

    @device_guarded
    def forward(self, feat, filter):
        nf, ns, c, h, w = feat.shape
        if filter.numel() == ns * c and filter.dim() != 5:
            return super().forward(feat, filter)
        _inference_only(self)
        _device_only("DenseBoxRegressor", feat, filter)
        _require_device(feat, filter)
        if filter.dim() != 5 or filter.shape[0] != ns or filter.shape[2] != c or filter.shape[-1] * filter.shape[-2] != 1:
            raise ValueError("DenseBoxRegressor: filter (n_seq, T, C, 1, 1) expected")
        T = filter.shape[1]
        if not 1 <= T <= MAX_TOKENS:
            raise NotImplementedError(f"DenseBoxRegressor: 1 <= T <= {MAX_TOKENS} filters per sequence on the gfx950 path")
        L = _lib.lib()
        n_img = nf * ns
        nb = L.pt_tamos_bbreg_ws_bytes(n_img, T, c, h, w)
        if nb == 0:
            raise NotImplementedError("DenseBoxRegressor: configuration not covered by the gfx950 kernels")
        params = self._params()
        fmap = feat.reshape(n_img, c, h, w).contiguous()
        filt = filter.reshape(1, ns, T, c).expand(nf, ns, T, c).contiguous()           # image f * ns + s reads sequence s's filters
        out = torch.empty(n_img, T, 4, h, w, dtype=torch.float32, device=feat.device)
        ws = workspace(nb, feat.device)
        rc = L.pt_tamos_bbreg_f32(_ptr(params), _ptr(fmap), _ptr(filt), _ptr(out), n_img, T, c, h, w, _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "pt_tamos_bbreg_f32")
        return out.reshape(1, n_img, T, 4, h, w)
