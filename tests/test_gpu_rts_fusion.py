"""RTS instance-score encoder and learners fusion on the MI355X (rts_fusion.hip through pytracking_amd.rts_fusion): every encoder, fusion
and chain case against the golden of the unmodified reference's fp32 CPU run (tools/make_golden_rts_fusion.py) within the project's 1e-4
absolute and bit-identical on a second call; every case against the float64 run of the plain-torch stand-in within f64_bound.bound(ref_err)
(FACTOR x the fp32 CPU stand-in's own distance from float64 on that case, tests/rts_fusion_cases.py) -- the measured ratios are printed
and, when RTS_FUSION_F64_OUT names a file, written there as a table (profiles/rts_fusion_f64.txt is the table of such a run); a null
sample_w, score-map views and (frames, seq) inputs, graph capture of the chain, the weight cache, and install(rts_fusion=True,
decoder=True) on an RTSNet built from the bundle's own parts.

Every test prints its measured figures before it asserts (run with -s)."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import f64_bound
import rts_fusion_cases as RC
from f64_bound import dev, needs_bundle
from oracle import ref_harness
from pytracking_amd import rts_fusion as RF, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = f64_bound.Table("RTS_FUSION_F64_OUT",
                        "RTS instance-score encoder and learners fusion on the MI355X against the float64 run of the plain-torch stand-in\n"
                        "(tests/test_gpu_rts_fusion.py): per output max |out - float64| and its ratio to ref_err, the fp32 CPU stand-in's own\n"
                        f"distance from float64 on that case; bound = {f64_bound.FACTOR} x ref_err.")


def _run_enc(name):
    g, n, H, W, dims, use_bn, sd, scores = RC.enc_case(name)
    net = RC.enc_module(name, DEV)
    with torch.no_grad():
        s = dev(scores)[:, None]                                       # (frames, 1 sequence, H, W)
        assert RF.encoder_covered(net, s)
        enc, sw = RF.encode(net, s)
    return g, net, s, enc, sw


def _run_fuse(name, kind):
    g, n, f, source, target, sds, seg, clf = RC.fuse_case(name)
    net = RC.fuse_module(name, kind, DEV)
    with torch.no_grad():
        seg, clf = dev(seg), dev(clf)
        assert RF.fuse_covered(net, seg, clf)
        out = RF.fuse(net, seg, clf)
    return g, net, seg, clf, out


def _run_chain(kind, want_sample_w=False):
    g, _, _, scores, seg = RC.chain_case()
    enc_net, fusion = RC.chain_modules(kind, DEV)
    scores, seg = dev(scores), dev(seg)

    def chain():
        return RF.fuse(fusion, seg, RF.encode(enc_net, scores, want_sample_w=want_sample_w)[0])

    with torch.no_grad():
        out = chain()
    return g, chain, out


@pytest.mark.parametrize("name", RC.ENC_CASES)
def test_encoder_matches_reference_golden(name):
    g, net, s, enc, sw = _run_enc(name)
    n, H, W, dims, use_bn = synth.SCORE_ENC_CASES[name]
    assert enc.shape == (n, 1, dims[3], H, W) and sw.shape == enc.shape
    err = max(float(np.abs(enc[:, 0].cpu().numpy() - g["label_enc"]).max()), float(np.abs(sw[:, 0].cpu().numpy() - g["sample_w"]).max()))
    print(f"\nrts_fusion_enc_{name}: max |gpu - reference fp32| = {err:.3e} (bound {ATOL:.0e}, ref_fp32_err {float(g['ref_fp32_err']):.3e})")
    assert err <= ATOL
    with torch.no_grad():
        enc2, sw2 = RF.encode(net, s)
    assert torch.equal(enc, enc2) and torch.equal(sw, sw2)              # two calls are bit-identical


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
@pytest.mark.parametrize("name", RC.FUSE_CASES)
def test_fuse_matches_reference_golden(name, kind):
    g, net, seg, clf, out = _run_fuse(name, kind)
    assert out.shape == seg.shape
    err = float(np.abs(out[0].cpu().numpy() - g["out." + kind]).max())
    print(f"\nrts_fusion_fuse_{name} {kind}: max |gpu - reference fp32| = {err:.3e} (bound {ATOL:.0e}, ref_fp32_err "
          f"{float(g['ref_fp32_err.' + kind]):.3e})")
    assert err <= ATOL
    with torch.no_grad():
        assert torch.equal(out, RF.fuse(net, seg, clf))
        if name == "same" and kind == "add":
            assert torch.equal(out, seg + clf)                          # no resize: the plain fusion, bit for bit
        if name == "same" and kind == "concat":                         # no resize: the plain convolution of the concatenation
            plain = torch.nn.functional.conv2d(torch.cat([seg[0], clf[0]], 1).double(), net.fusion_conv1.weight.double(),
                                               net.fusion_conv1.bias.double(), padding=1)
            anchor = RC.fuse_anchor(name, kind)
            assert float((out[0].double() - plain).abs().max()) <= f64_bound.bound(anchor.ref_err)


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
def test_chain_matches_reference_golden(kind):
    g, chain, out = _run_chain(kind)
    err = float(np.abs(out[0].cpu().numpy() - g["out." + kind]).max())
    print(f"\nrts_fusion_{RC.CHAIN} {kind}: max |gpu - reference fp32| = {err:.3e} (bound {ATOL:.0e}, ref_fp32_err "
          f"{float(g['ref_fp32_err.' + kind]):.3e})")
    assert out.shape == (1, 1, 16, 30, 52) and err <= ATOL
    with torch.no_grad():
        assert torch.equal(out, chain())


@pytest.mark.parametrize("name", RC.ENC_CASES)
def test_encoder_within_float64_bound(name):
    g, net, s, enc, sw = _run_enc(name)
    a = RC.enc_anchor(name)
    f64_bound.held(f"enc_{name}", {"label_enc": enc, "sample_w": sw}, a.want, a.ref_err, table=TABLE)


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
@pytest.mark.parametrize("name", RC.FUSE_CASES)
def test_fuse_within_float64_bound(name, kind):
    g, net, seg, clf, out = _run_fuse(name, kind)
    a = RC.fuse_anchor(name, kind)
    f64_bound.held(f"fuse_{name}_{kind}", {"decoder_input": out}, a.want, a.ref_err, table=TABLE)


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
def test_chain_within_float64_bound(kind):
    g, chain, out = _run_chain(kind)
    a = RC.chain_anchor(kind)
    f64_bound.held(f"{RC.CHAIN}_{kind}", {"decoder_input": out}, a.want, a.ref_err, table=TABLE)


@pytest.mark.parametrize("name", ["odd", "deployed", "dims"])
def test_null_sample_w_gives_the_same_label_enc_bits(name):
    g, net, s, enc, sw = _run_enc(name)
    with torch.no_grad():
        enc2, none = RF.encode(net, s, want_sample_w=False)
    assert none is None and torch.equal(enc2, enc)


def test_score_map_views_and_sequences():
    g, net, s, enc, sw = _run_enc("odd")                                # (3, 1, 5, 7)
    n, H, W = s.shape[0], s.shape[2], s.shape[3]
    with torch.no_grad():
        padded = torch.zeros(n, 1, H + 3, W + 5, device=DEV)
        padded[:, :, 1:H + 1, 2:W + 2] = s
        view = padded[:, :, 1:H + 1, 2:W + 2]                           # a non-contiguous view of the same values
        assert not view.is_contiguous() and RF.encoder_covered(net, view)
        e1, s1 = RF.encode(net, view)
        assert torch.equal(e1, enc) and torch.equal(s1, sw)
        four = torch.cat([s, s.flip(0)], 0)[:4].reshape(2, 2, H, W)     # frames = 2, seq = 2
        e2, s2 = RF.encode(net, four)
        flat_e, flat_s = RF.encode(net, four.reshape(4, 1, H, W))       # the contiguous, flattened call
    assert e2.shape == (2, 2, enc.shape[2], H, W) and s2.shape == e2.shape
    assert torch.equal(e2.reshape(4, *enc.shape[2:]), flat_e[:, 0]) and torch.equal(s2.reshape(4, *enc.shape[2:]), flat_s[:, 0])
    assert torch.equal(flat_e[:3], enc) and torch.equal(flat_s[:3], sw)  # (frames, seq) flattens frame-major, as the reference's view


@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
def test_graph_capture_of_the_chain_replays_the_eager_bits(kind):
    g, chain, out = _run_chain(kind)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain()                                                     # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = chain()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, out)


def test_cache_follows_load_state_dict_and_in_place_updates():
    g, n, H, W, dims, use_bn, sd, scores = RC.enc_case("bn")
    net = RC.enc_module("bn", DEV)
    s = dev(scores)[:, None]
    other = synth.label_enc_state(int(g["state_seed"]) + 50, dims, use_bn)
    with torch.no_grad():
        first = RF.encode(net, s)
        net.load_state_dict(RC.state_tensors(other))
        want = RF.encode(RC.new_encoder(dims, use_bn, other, DEV), s)
        got = RF.encode(net, s)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], first[0])
        net.res1.bn2.running_var.mul_(1.7)                              # in place
        net.samp_w_pred.bias.add_(0.3)
        changed = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
        want2 = RF.encode(RC.new_encoder(dims, use_bn, changed, DEV), s)
        got2 = RF.encode(net, s)
        stock = net(s)
    assert torch.equal(got2[0], want2[0]) and torch.equal(got2[1], want2[1]) and not torch.equal(got2[1], got[1])
    err = max(float((got2[0] - stock[0]).abs().max()), float((got2[1] - stock[1]).abs().max()))
    print(f"\nencoder after the in-place change: max |fused - stock on device| = {err:.3e}")
    assert err <= 2 * ATOL                                              # both sides within 1e-4 of the exact value
    gf, fusion, seg, clf, out = _run_fuse("edge", "concat")
    with torch.no_grad():
        fusion.fusion_conv1.weight.mul_(0.5)                            # in place
        got3 = RF.fuse(fusion, seg, clf)
        stock3 = RC.fuse_standin(fusion, seg, clf)
    err = float((got3 - stock3).abs().max())
    print(f"fusion after the in-place change: max |fused - stock on device| = {err:.3e}")
    assert not torch.equal(got3, out) and err <= 2 * ATOL


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(rts_fusion=True, decoder=True)
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
@pytest.mark.parametrize("kind", RC.FUSION_TYPES)
def test_install_dispatches_an_rts_net_built_from_the_bundles_parts(amd, kind):
    """RTSNet(feature_extractor=None, ...) from the bundle's LinearFilter, RTSDecoder, ResidualDS16SW_Clf and LearnersFusion, with stub
    backbone maps of the decoder tests' small case 'tiny' (layer3 = 3 x 4, so the image is 48 x 64) and 512 target-model channels."""
    import ltr.models.rts.linear_filter as target_clf
    from ltr.models.rts.decoder import RTSDecoder
    from ltr.models.rts.label_encoder import ResidualDS16SW_Clf
    from ltr.models.rts.learners_fusion import LearnersFusion
    from ltr.models.rts.rts_net import RTSNet
    c = synth.LWL_DECODER_CASES["tiny"]
    f, C = c["ic"], 512
    torch.manual_seed(5100)
    net = RTSNet(feature_extractor=None, target_model=target_clf.LinearFilter(filter_size=3, filter_initializer=None),
                 decoder=RTSDecoder(f, c["mdim"], OrderedDict((L, fc) for L, fc, _, _ in c["levels"]), use_bn=True),
                 target_model_input_layer="layer3", decoder_input_layers=tuple(L for L, _, _, _ in c["levels"]),
                 clf_encoder=ResidualDS16SW_Clf(layer_dims=synth.LABEL_ENC_DIMS, use_bn=False), clf_enc_input="sc",
                 fusion_module=LearnersFusion(kind)).to(DEV).eval()
    rng = np.random.default_rng(5101)
    feats = {L: dev(np.maximum(rng.standard_normal((1, fc, H, W), dtype=np.float32), 0)) for L, fc, H, W in c["levels"]}
    h, w = c["levels"][1][2:]
    feat_tm = dev(rng.standard_normal((1, C, h, w), dtype=np.float32) * np.float32(0.05))
    filt = dev(rng.standard_normal((1, f, C, 3, 3), dtype=np.float32) * np.float32(0.3))
    scores = dev(synth.score_maps(5102, 1, 2, 3))[None]                # (1 frame, 1 sequence, 2, 3): resized to 3 x 4 by the fuse
    enc_key, seg_key = "ResidualDS16SW_Clf.forward", "RTSNet.segment_target"
    amd.stats.clear()
    with torch.no_grad():
        enc, sw = net.clf_encoder(scores)
        mask, mask_enc = net.segment_target(filt, feat_tm, feats, enc)
        want_enc, want_sw = amd.original(ResidualDS16SW_Clf, "forward")(net.clf_encoder, scores)
        want_mask, want_mask_enc = amd.original(RTSNet, "segment_target")(net, filt, feat_tm, feats, want_enc)
    assert amd.stats[enc_key + ".fast"] == 1 and amd.stats[enc_key + ".reference"] == 0, dict(amd.stats)
    assert amd.stats[seg_key + ".fast"] == 1 and amd.stats[seg_key + ".reference"] == 0, dict(amd.stats)
    assert enc.shape == want_enc.shape and sw.shape == want_sw.shape and mask.shape == want_mask.shape
    errs = [float((a - b).abs().max()) for a, b in ((enc, want_enc), (sw, want_sw), (mask, want_mask), (mask_enc, want_mask_enc))]
    print(f"\ninstall(rts_fusion=True, decoder=True), {kind}: max |fused - stock on device| encoder {max(errs[:2]):.3e}, mask {errs[2]:.3e}, "
          f"mask encoding {errs[3]:.3e} (bound 2e-4)")
    assert max(errs) <= 2e-4
    with torch.no_grad():
        net.segment_target(filt, feat_tm, feats, None)                  # no encoded scores: the reference branch
    assert amd.stats[seg_key + ".fast"] == 1 and amd.stats[seg_key + ".reference"] == 1
    net.train()
    net.decoder.eval()                                                  # (its BatchNorm would see one value per channel)
    with torch.no_grad():
        net.clf_encoder(scores)                                         # training mode: the reference branch
        net.segment_target(filt, feat_tm, feats, enc)
    assert amd.stats[enc_key + ".fast"] == 1 and amd.stats[enc_key + ".reference"] == 1
    assert amd.stats[seg_key + ".fast"] == 1 and amd.stats[seg_key + ".reference"] == 2
