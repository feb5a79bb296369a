"""pytracking_amd._packs without a GPU.  The fold: both forms against torch.nn.BatchNorm2d in float64, and the float32 bits of every
module's pack against packs built by the per-module fold code the modules carried before they shared one (kept here verbatim: the
behaviour pin of the fold).  The cache class: the state transitions the six modules rely on."""
import gc

import pytest
import torch
import torch.nn.functional as F

import iou_feat_cases as IC
import kys_modules
import label_enc_cases as LC
import lwl_decoder_cases as DC
import rts_fusion_cases as RC
from oracle import ref_harness
from pytracking_amd import _lib, _packs, synth
from pytracking_amd import candidate_matching as CM, iou_feat as IF, kys as K, label_encoder as LE, lwl_decoder as LD, rts_fusion as RF

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")


@pytest.fixture(scope="module", autouse=True)
def L():
    _lib.build_library()
    return _lib.lib()


# ---- the fold against BatchNorm2d ----------------------------------------------------------------------------------------------------
def test_both_fold_forms_are_eval_batchnorm_in_float64():
    """C = 3, random running statistics.  Every output is a sum of 2 * 9 products, scaled and shifted: under 40 roundings of 2^-53 on
    either side of the comparison (the fold, and BatchNorm2d behind the convolution), each relative to a partial result no larger than
    the same expression evaluated on absolute values (`mag`)."""
    gen = torch.Generator().manual_seed(5)
    conv = torch.nn.Conv2d(2, 3, 3, padding=1).double()
    bn = torch.nn.BatchNorm2d(3).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(3, generator=gen, dtype=torch.float64))
        bn.bias.copy_(torch.randn(3, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(3, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(3, generator=gen, dtype=torch.float64) + 0.1)
        x = torch.randn(2, 2, 5, 7, generator=gen, dtype=torch.float64)
        want = bn(conv(x))
        s, shift = _packs.bn_fold(conv, bn)
        w, b = _packs.bn_fold_weights(conv, bn)
        kept_apart = F.conv2d(x, conv.weight, None, padding=1) * s.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        into_w = F.conv2d(x, w, b, padding=1)
        mag = ((F.conv2d(x.abs(), conv.weight.abs(), None, padding=1) + (conv.bias.abs() + bn.running_mean.abs()).view(1, -1, 1, 1))
               * s.abs().view(1, -1, 1, 1) + bn.bias.abs().view(1, -1, 1, 1))
    assert s.dtype == shift.dtype == w.dtype == b.dtype == torch.float64 and w.shape == conv.weight.shape
    bound = 2 * 40 * 2.0 ** -53 * float(mag.max())
    for name, got in (("scale kept apart", kept_apart), ("scale in W", into_w)):
        err = float((got - want).abs().max())
        print(f"\n{name}: max |fold - BatchNorm2d| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    # without a BatchNorm: scale 1 and the bias (zeros for a bias-free convolution), W and b untouched
    s, shift = _packs.bn_fold(conv)
    assert torch.equal(s, torch.ones(3, dtype=torch.float64)) and torch.equal(shift, conv.bias.detach())
    bare = torch.nn.Conv2d(2, 3, 3, bias=False)
    assert torch.equal(_packs.bn_fold(bare)[1], torch.zeros(3, dtype=torch.float64)) and _packs.bn_fold_weights(bare)[1] is None
    assert torch.equal(_packs.tap_major(bare), bare.weight.detach().permute(0, 2, 3, 1).reshape(3, 18))


# ---- the per-module fold code before _packs.py, verbatim -----------------------------------------------------------------------------
def _enc_folded(conv, bn):
    o = conv.out_channels
    bias = conv.bias.detach().double() if conv.bias is not None else torch.zeros(o, dtype=torch.float64, device=conv.weight.device)
    if bn is None:
        s, shift = torch.ones_like(bias), bias
    else:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shift = (bias - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return conv.weight.detach().permute(0, 2, 3, 1).reshape(o, -1).float(), s.float(), shift.float()


def _enc_pack(layers):
    parts = []
    for group in ([0], [1, 2], [3], [4, 5], [6], [7, 8]):
        w, s, b = zip(*[_enc_folded(*layers[k]) for k in group])
        parts += [torch.cat(w).reshape(-1), torch.cat(s), torch.cat(b)]
    return torch.cat(parts).contiguous()


def _iou_pack(blocks):
    parts = []
    for conv, bn in blocks:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shift = (conv.bias.detach().double() - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
        parts += [conv.weight.detach().permute(0, 2, 3, 1).reshape(-1).float(), s.float(), shift.float()]
    return torch.cat(parts).contiguous()


def _dec_folded(conv, bn):
    o = conv.out_channels
    bias = conv.bias.detach().double() if conv.bias is not None else torch.zeros(o, dtype=torch.float64, device=conv.weight.device)
    if bn is None:
        return torch.ones_like(bias).float(), bias.float()
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s.float(), ((bias - bn.running_mean.detach().double()) * s + bn.bias.detach().double()).float()


def _dec_pack(layers):
    parts = []
    last = layers[-1][0]
    for conv, bn in layers:
        w = conv.weight.detach().float()
        if conv is last:
            parts += [w.permute(0, 2, 3, 1).reshape(-1), conv.bias.detach().float().reshape(-1)]
        elif w.shape[-1] == 1:
            parts += [w.reshape(-1), conv.bias.detach().float().reshape(-1)]
        else:
            parts += [w.permute(0, 2, 3, 1).reshape(-1), *_dec_folded(conv, bn)]
    return torch.cat(parts).contiguous()


def _kys_fold(conv, bn=None):
    w = conv.weight.detach().double()
    b = conv.bias.detach().double() if conv.bias is not None else None
    if bn is not None:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w = w * s[:, None, None, None]
        b = (b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return [w] + ([b] if b is not None else [])


def _kys_pack(pred):
    _fold = _kys_fold
    parts = []
    for stack in (pred.cost_volume_proc1, pred.cost_volume_proc2):
        parts += _fold(stack[0][0], stack[0][1]) + _fold(stack[1][0], stack[1][1])
    parts += _fold(pred.init_hidden_state_predictor[0][0])
    parts += _fold(pred.is_target_predictor[0][0]) + _fold(pred.is_target_predictor[1][0])
    parts += _fold(pred.representation_predictor[0][0]) + _fold(pred.representation_predictor[1][0])
    parts += _fold(pred.response_predictor[0][0])
    g = pred.state_predictor
    parts += _fold(g.conv_reset) + _fold(g.conv_update) + _fold(g.conv_state_new)
    return torch.cat([p.reshape(-1) for p in parts]).float().contiguous()


def _tcm_fold(conv, bn=None):
    w = conv.weight.detach().double().reshape(conv.weight.shape[0], -1)
    b = conv.bias.detach().double()
    if bn is not None:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w = w * s[:, None]
        b = (b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return w, b


def _tcm_pack(sg):
    _fold = _tcm_fold
    parts = []
    enc = sg.kenc.encoder
    convs = [m for m in enc if isinstance(m, torch.nn.Conv1d)]
    bns = [m for m in enc if isinstance(m, torch.nn.BatchNorm1d)]
    for i, conv in enumerate(convs):
        parts += list(_fold(conv, bns[i] if i < 4 else None))
    if not sg.conf["skip_gnn"]:
        for layer in sg.gnn.layers:
            up = layer.update
            qkv = [_fold(p) for p in up.attn.proj]
            parts += [torch.cat([w for w, _ in qkv]), torch.cat([b for _, b in qkv])]
            parts += list(_fold(up.attn.merge))
            parts += list(_fold(up.mlp[0], up.mlp[1]))
            parts += list(_fold(up.mlp[3]))
    parts += list(_fold(sg.final_proj))
    return torch.cat([p.reshape(-1) for p in parts]).float().contiguous()


def _same_bits(got, want):
    assert got.dtype == want.dtype == torch.float32 and got.is_contiguous()
    return torch.equal(got, want) and torch.equal(got.view(torch.int32), want.view(torch.int32))      # -0.0 and NaN payloads included


def test_label_encoder_pack_bits_are_the_earlier_folds():
    net = LC.module("bn_odd")
    assert any(bn is not None for _, bn in LE._layers(net))
    assert _same_bits(LE.pack_weights(net), _enc_pack(LE._layers(net)))


def test_score_encoder_pack_bits_are_the_earlier_folds():
    net = RC.enc_module("bn")
    assert any(bn is not None for _, bn in RF._layers(net))
    assert _same_bits(RF.pack_weights(net), _enc_pack(RF._layers(net)))


def test_iou_feat_pack_bits_are_the_earlier_folds():
    net = IC.module("b")
    assert _same_bits(IF.pack_weights(net), _iou_pack(IF._blocks(net)))


def test_decoder_pack_bits_are_the_earlier_folds():
    net = DC.module("tiny")
    st = LD._structure(net)
    assert st["use_bn"] and _same_bits(LD.pack_weights(net), _dec_pack(st["layers"]))


def test_kys_predictor_pack_bits_are_the_earlier_folds():
    pred = kys_modules.wrapper(31, "max", 4, "cpu").predictor
    assert _same_bits(K.pack_weights(pred), _kys_pack(pred))


@needs_reference
def test_superglue_pack_bits_are_the_earlier_folds():
    ref_harness.install()
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    sg = SuperGlue({'skip_gnn': False, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': 10, 'output_normalization': 'sinkhorn'})
    sg.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.tcm_superglue_state(17).items()})
    sg.eval()
    assert _same_bits(CM.pack_weights(sg), _tcm_pack(sg))


# ---- the cache class -----------------------------------------------------------------------------------------------------------------
def _layers(net):
    return [(net[0], net[1])]


def _make(net):
    return torch.cat([t.detach().reshape(-1) for t in _packs.tensors(_layers(net))])


def _packed(cache, net):
    return cache.get(net, _packs.layers_key(_layers(net)), _make)


def test_pack_cache_follows_the_module_state():
    cache = _packs.PackCache()
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3)).eval()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    assert net not in cache and len(cache) == 0
    p0 = _packed(cache, net)
    assert net in cache and _packed(cache, net) is p0                   # same state: the same object
    with torch.no_grad():
        net[1].running_var.mul_(2.0)                                    # in-place: the version counter moves
    p1 = _packed(cache, net)
    assert p1 is not p0 and not torch.equal(p1, p0)
    net.load_state_dict(state)
    p2 = _packed(cache, net)
    assert p2 is not p1 and torch.equal(p2, p0)
    net[0].bias.data = net[0].bias.data + 1.0                           # through .data: a new tensor, the data_ptr moves
    p3 = _packed(cache, net)
    assert p3 is not p2 and not torch.equal(p3, p0)
    net[1].eps = 1e-3                                                   # an extra of the key
    assert _packed(cache, net) is not p3
    other = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3)).eval()
    _packed(cache, other)
    cache.drop(net)
    assert net not in cache and other in cache and len(cache) == 1
    cache.drop(net)                                                     # dropping what is not there is not an error
    del other
    gc.collect()
    assert len(cache) == 0                                              # the entry goes with the module


def test_state_key_extras_and_caches_are_per_module():
    t = torch.zeros(3)
    assert _packs.state_key([t]) == ((t.data_ptr(), t._version, (3,)),)
    assert _packs.state_key([t], "max") != _packs.state_key([t], "none") and _packs.state_key([t], "max")[-1] == "max"
    caches = [m._PACKS for m in (CM, IF, K, LE, LD, RF)]
    assert all(isinstance(c, _packs.PackCache) for c in caches) and len({id(c) for c in caches}) == 6


def test_structure_checks_ask_for_the_exact_layer_types():
    """conv_ok / bn_ok accept torch.nn.Conv2d / BatchNorm2d themselves, not subclasses (a subclass may override forward): every module
    that recognises a structure through them, the IoU towers included, hands such a block to the reference."""
    class MyConv(torch.nn.Conv2d):
        pass

    class MyNorm(torch.nn.BatchNorm2d):
        pass

    assert _packs.conv_ok(torch.nn.Conv2d(4, 4, 3, padding=1), 3, 1, True) and not _packs.conv_ok(MyConv(4, 4, 3, padding=1), 3, 1, True)
    assert _packs.bn_ok(torch.nn.BatchNorm2d(4), 4) and not _packs.bn_ok(MyNorm(4), 4)
    assert not _packs.conv_ok(torch.nn.Conv2d(4, 4, 3, padding=1, bias=False), 3, 1, True)
    assert not _packs.conv_ok(torch.nn.Conv2d(4, 4, 3, padding=2, dilation=2), 3, 1, True)
    assert _packs.conv_ok(torch.nn.Conv2d(4, 4, 3, stride=2, padding=1), 3, 2, True) and _packs.conv_ok(torch.nn.Conv2d(4, 4, 1), 1, 1, True)
    net = IC.module("b")
    assert IF._blocks(net) is not None
    sub = MyConv(net.conv3_1t[0].in_channels, net.conv3_1t[0].out_channels, 3, padding=1)
    sub.load_state_dict(net.conv3_1t[0].state_dict())
    net.conv3_1t[0] = sub
    assert IF._blocks(net) is None
    net = IC.module("b")
    net.conv4_2t[1] = MyNorm(net.conv4_2t[1].num_features).eval()
    assert IF._blocks(net) is None
    other = LC.ResidualDS16SW(synth.LABEL_ENC_DIMS, False).eval()
    assert LE.pack_weights(other) is not None
    with pytest.raises(NotImplementedError):
        LE.pack_weights(torch.nn.Sequential())                          # refused on the structure alone
