"""The edge cases of tests/fused_edge_cases.py without a GPU: every one is covered by its module (pt_*_ws_bytes > 0 and a structure the
Python mirror packs, so the GPU test cannot be sent down the reference branch), every 3x3 convolution lands on the route the case claims
(pt_mf_corr_tm_plan), and the arithmetic behind each named edge -- the 1x1 kernel switch, the wave shares, the padded widths, the row
limit -- holds for the shapes chosen."""
import pytest

import corr_tm_cases as TC
import fused_edge_cases as EC
import lwl_decoder_cases as DC
from pytracking_amd import _lib, iou_feat as IF, label_encoder as LE, lwl_decoder as LD, synth

ALL = [(kind, name) for kind in EC.CASES for name in EC.CASES[kind]]


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _ws_bytes(L, kind, name):
    if kind == "iou_feat":
        n, t3, t4 = EC.IOU_FEAT[name]
        return L.pt_iou_feat_ws_bytes(n, *t3, *t4)
    if kind == "label_enc":
        n, H, W, dims, _ = EC.LABEL_ENC[name]
        return L.pt_label_enc_ws_bytes(n, H, W, *dims)
    return L.pt_lwl_decoder_ws_bytes(*DC.c_args(EC.DECODER[name]))


@pytest.mark.parametrize("kind,name", ALL)
def test_every_edge_case_is_covered(kind, name, L):
    assert _ws_bytes(L, kind, name) > 0
    net, args = EC.case(kind, name)
    pack = {"iou_feat": IF, "label_enc": LE, "lwl_decoder": LD}[kind].pack_weights(net)      # raises for a structure the mirror refuses
    assert pack.numel() > 0
    assert name not in {"iou_feat": synth.IOU_FEAT_CASES, "label_enc": synth.LABEL_ENC_CASES, "lwl_decoder": synth.LWL_DECODER_CASES}[kind]
    n = EC.samples(kind, name)
    first = {"iou_feat": lambda: args["feats"][0], "label_enc": lambda: args["masks"], "lwl_decoder": lambda: args["scores"]}[kind]()
    assert first.shape[0] == n and all(v.shape[0] == 1 for v in _leaves(EC.sample(kind, args, n - 1)))


def _leaves(args):
    for v in args.values():
        if hasattr(v, "shape"):
            yield v
        elif isinstance(v, dict):
            yield from _leaves(v)
        elif isinstance(v, tuple) and v and hasattr(v[0], "shape"):
            yield from v


@pytest.mark.parametrize("name", EC.CASES["lwl_decoder"])
def test_decoder_routes(name, L):
    plans = EC.plans(L, "lwl_decoder", name)
    assert set(plans) == set(EC.DECODER_ROUTES[name])
    for stage, want in EC.DECODER_ROUTES[name].items():
        got = {EC.GEMM if p == EC.GEMM else EC.BANDED for p in plans[stage]}
        assert got == {want}, (stage, plans[stage])
        assert all(p == EC.GEMM or 1 <= p[0] <= 8 for p in plans[stage])                # dec_conv3_plan takes the banded route for 1..8 splits


@pytest.mark.parametrize("name", EC.CASES["iou_feat"])
def test_iou_routes(name, L):
    plans = EC.plans(L, "iou_feat", name)
    for tower, want in zip(("tower3", "tower4"), EC.IOU_ROUTES[name]):
        assert {EC.GEMM if p == EC.GEMM else EC.BANDED for p in plans[tower]} == {want}, (tower, plans[tower])


def test_iou_row_limit_is_the_banded_routes(L):
    """The widest row pt_mf_corr_tm_plan accepts for the layers of `row_limit` / `row_past`, found by scanning."""
    for name in ("row_limit", "row_past"):
        n, _, t4 = EC.IOU_FEAT[name]
        for cout, cin in ((t4[1], t4[0]), (t4[2], t4[1])):
            widest = max(W for W in range(1, 400) if TC.query(L, n, cout, cin, t4[3], W)[0] == 0)
            assert widest == EC.IOU_ROW_LIMIT, (name, cout, cin, widest)
    assert EC.IOU_FEAT["row_limit"][2][4] == EC.IOU_ROW_LIMIT and EC.IOU_FEAT["row_past"][2][4] == EC.IOU_ROW_LIMIT + 1
    assert EC.IOU_FEAT["row_limit"][1][3:] == (1, 1) and EC.IOU_FEAT["row_past"][1][3:] == (1, 1)
    for n, t3, t4 in EC.IOU_FEAT.values():
        assert t3[1] != t3[2] and t4[1] != t4[2]                                       # Cmid != Cout
    n, t3, t4 = EC.IOU_FEAT["n8_c192"]
    assert n == 8 and t3[0] % 64 == 0 and t3[0] % 128 and t4[0] % 64 == 0 and t4[0] % 128
    assert EC.IOU_FEAT["row_past"][2][1] % 64                                          # the GEMM route pads the second layer's input


def test_decoder_edges_are_where_the_cases_say():
    c = EC.DECODER["mdim64"]
    assert c["mdim"] == 64 and c["n"] == 1 and sorted(fc for _, fc, _, _ in c["levels"]) == [16, 48, 48, 80]
    shares = lambda fc: [len(range(w * 16, fc, 64)) for w in range(4)]                  # noqa: E731   chunks of k_dec_conv1's four waves
    assert shares(48) == [1, 1, 1, 0] and shares(80) == [2, 1, 1, 1]
    c = EC.DECODER["mdim96"]
    assert all((DC.OC[lv] * c["mdim"] + c["ic"]) % 64 for lv, _, _, _ in c["levels"]) and c["mdim"] // 2 == 48
    assert c["levels"][-1][3] > EC.IOU_ROW_LIMIT                                       # layer1: Cpad != Cin on the GEMM route
    c = EC.DECODER["n8_wide1x1"]
    (_, _, h2, w2), (_, _, h1, w1) = c["levels"][2:]
    assert c["n"] == 8 and 1985 <= h1 * w1 <= 2048 and (h1 * w1) % 16
    assert EC.wide_1x1(h1 * w1, DC.OC["layer1"] * c["mdim"], 8) and not EC.wide_1x1(h1 * w1 - 64, DC.OC["layer1"] * c["mdim"], 8)
    assert not EC.wide_1x1(h2 * w2, DC.OC["layer2"] * c["mdim"], 8) and EC.wide_1x1(h2 * w2 + 64, DC.OC["layer2"] * c["mdim"], 8)
    c = EC.DECODER["three_n8"]
    assert c["n"] == 8 and len(c["levels"]) == 3 and not c["use_bn"]


def test_label_encoder_edges_are_where_the_cases_say():
    hw = lambda name: EC.LABEL_ENC[name][1:3]                                           # noqa: E731
    assert [hw(k) for k in ("m1x1", "m1x17", "m17x1")] == [(1, 1), (1, 17), (17, 1)]
    assert [hw(k)[0] for k in ("h15", "h16", "h17")] == [15, 16, 17] and [hw(k)[1] for k in ("w127", "w128", "w129")] == [127, 128, 129]
    assert EC.LABEL_ENC["n33"][0] == 33
    assert EC.LABEL_ENC["c16"][3] == (16,) * 4 and EC.LABEL_ENC["c64"][3] == (64,) * 4 and 48 in EC.LABEL_ENC["c48"][3]


def test_per_sample_cases_and_where_they_are_bit_for_bit(L):
    """The plans of `three_n8` and `n8_c192` are those of one sample alone, so tests/test_gpu_fused_f64.py asserts equal bits there; the
    wide-1x1 case changes its channel splits with n and is held to the bound instead."""
    assert all(EC.samples(kind, name) in (8, 33) for kind, name in EC.PER_SAMPLE)
    got = {(kind, name): EC.routes_coincide(L, kind, name) for kind, name in EC.PER_SAMPLE}
    assert got == {("iou_feat", "n8_c192"): True, ("label_enc", "n33"): True, ("lwl_decoder", "n8_wide1x1"): False,
                   ("lwl_decoder", "three_n8"): True}
