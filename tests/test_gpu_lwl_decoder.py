"""Segmentation decoder on the MI355X (lwl_decoder.hip through pytracking_amd.lwl_decoder): every case of synth.LWL_DECODER_CASES -- the
mask AND every '{L}_dec' level -- against the golden of the unmodified reference's fp32 CPU run (tools/make_golden_lwl_decoder.py) within
the project's 1e-4 absolute (the reference's own distance from float64 is recorded in each golden, at most 1.4e-6), bit-identical repeats,
the mask with and without level outputs, n = 4, the deployed size in full against the same module in stock PyTorch on the device, graph
capture, tensor views, the weight cache, install(decoder=True) on the bundle's LWL net and on the RTS class, and one segment_target call
downstream of the fused learner.

Every test prints its measured maximum error before it asserts (run with -s)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import lwl_decoder_cases as DC
from f64_bound import needs_bundle
from oracle import ref_harness
from pytracking_amd import lwl_decoder as LD, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
_RUNS = {}


def _run(name):
    """(golden, case, module on the device, scores, features, mask, level outputs) of one fused call, computed once per session."""
    if name not in _RUNS:
        g, c, _, _, _ = DC.case(name)
        net = DC.module(name, DEV)
        s, feats = DC.inputs(name, DEV)
        with torch.no_grad():
            assert LD.covered(net, s, feats, c["image"], DC.level_names(c))
            mask, outs = LD.forward(net, s, feats, c["image"], DC.level_names(c))
            torch.cuda.synchronize()
        _RUNS[name] = (g, c, net, s, feats, mask, outs)
    return _RUNS[name]


@pytest.mark.parametrize("name", DC.CASES)
def test_matches_reference_golden(name):
    g, c, net, s, feats, mask, outs = _run(name)
    assert mask.shape == (c["n"], 1) + tuple(c["image"]) and list(outs) == DC.level_names(c)
    errs = OrderedDict()
    for q in DC.level_names(c):
        L = q[:-4]
        fc, H, W = [(f, h, w) for l, f, h, w in c["levels"] if l == L][0]
        assert outs[q].shape == (c["n"], DC.OC[L] * c["mdim"], H, W)
        if q in g:
            errs[q] = float(np.abs(outs[q].cpu().numpy() - g[q]).max())
    errs["mask"] = float(np.abs(DC.golden_view(name, "mask", mask).cpu().numpy() - g["mask"]).max())
    print(f"\nlwl_decoder_{name}: max |gpu - reference fp32| " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items())
          + f"  (bound {ATOL:.0e}, ref_fp32_err {float(g['ref_fp32_err']):.3e})")
    assert all(v <= ATOL for v in errs.values()), errs
    with torch.no_grad():
        mask2, outs2 = LD.forward(net, s, feats, c["image"], DC.level_names(c))
        mask3, outs3 = LD.forward(net, s, feats, c["image"])
    assert torch.equal(mask, mask2) and all(torch.equal(outs[q], outs2[q]) for q in outs)           # two calls are bit-identical
    assert torch.equal(mask, mask3) and len(outs3) == 0                                            # and so is the mask without level outputs


def test_four_samples_reproduce_the_golden_per_copy():
    g, c, net, s, feats, mask, outs = _run("bands")
    with torch.no_grad():
        m4, o4 = LD.forward(net, s.repeat(2, 1, 1, 1, 1), {L: v.repeat(2, 1, 1, 1) for L, v in feats.items()}, c["image"], DC.level_names(c))
    assert m4.shape[0] == 4
    worst = 0.0
    for k in range(2):
        worst = max(worst, float(np.abs(m4[2 * k:2 * k + 2].cpu().numpy() - g["mask"]).max()))
        for q in o4:
            worst = max(worst, float(np.abs(o4[q][2 * k:2 * k + 2].cpu().numpy() - g[q]).max()))
    print(f"\nlwl_decoder_bands, n = 4: max |gpu - reference fp32| = {worst:.3e} (bound {ATOL:.0e})")
    assert worst <= ATOL


def test_deployed_in_full_against_stock_pytorch_on_the_device():
    g, c, net, s, feats, mask, outs = _run("deployed")
    with torch.no_grad():
        want_mask, want = net(s, feats, c["image"], DC.level_names(c))
    errs = {q: float((outs[q] - want[q]).abs().max()) for q in outs}
    errs["mask"] = float((mask - want_mask).abs().max())
    print("\nlwl_decoder_deployed: max |fused - stock on device| " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()) + "  (bound 2e-4)")
    assert all(v <= 2e-4 for v in errs.values()), errs


@pytest.mark.parametrize("name", ["tiny", "deployed"])
def test_graph_capture_replays_the_eager_bits(name):
    g, c, net, s, feats, mask, outs = _run(name)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            LD.forward(net, s, feats, c["image"], DC.level_names(c))      # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            k_mask, k_outs = LD.forward(net, s, feats, c["image"], DC.level_names(c))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(k_mask, mask) and all(torch.equal(k_outs[q], outs[q]) for q in outs)


def test_views_give_equal_bits():
    g, c, net, s, feats, mask, outs = _run("tiny")
    with torch.no_grad():
        sp = torch.zeros(s.shape[:3] + (s.shape[3] + 2, s.shape[4] + 3), device=DEV)
        sp[..., 1:-1, 2:-1] = s
        sv = sp[..., 1:-1, 2:-1]
        fv = {}
        for L, v in feats.items():
            wide = torch.zeros(v.shape[0], v.shape[1] * 2, v.shape[2], v.shape[3] + 1, device=DEV)
            wide[:, ::2, :, :-1] = v
            fv[L] = wide[:, ::2, :, :-1]
        assert not sv.is_contiguous() and not any(v.is_contiguous() for v in fv.values()) and LD.covered(net, sv, fv, c["image"])
        m2, o2 = LD.forward(net, sv, fv, c["image"], DC.level_names(c))
    assert torch.equal(m2, mask) and all(torch.equal(o2[q], outs[q]) for q in outs)


def test_cache_follows_load_state_dict_in_place_updates_and_refresh():
    g, c, sd, _, _ = DC.case("tiny")
    net = DC.module("tiny", DEV)
    s, feats = DC.inputs("tiny", DEV)
    other = synth.lwl_decoder_state(int(g["state_seed"]) + 50, c["mdim"], c["ic"], c["use_bn"], c["levels"])

    def fresh(state):
        m = DC.Decoder(c["ic"], c["mdim"], OrderedDict((L, fc) for L, fc, _, _ in c["levels"]), c["use_bn"])
        m.load_state_dict(state)
        return m.to(DEV).eval()

    with torch.no_grad():
        first = LD.forward(net, s, feats, c["image"])[0]
        net.load_state_dict(DC.state_tensors(other))
        got = LD.forward(net, s, feats, c["image"])[0]
        assert torch.equal(got, LD.forward(fresh(DC.state_tensors(other)), s, feats, c["image"])[0]) and not torch.equal(got, first)
        net.RRB1["layer2"].bblock[1].running_var.mul_(1.7)                # in place
        net.project.conv2.bias.add_(0.3)
        got2 = LD.forward(net, s, feats, c["image"])[0]
        changed = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        assert torch.equal(got2, LD.forward(fresh(changed), s, feats, c["image"])[0]) and not torch.equal(got2, got)
        net.CAB["layer4"].convreluconv[2].bias.data.mul_(-3.0)            # through .data, in place: no version bump, the same pointer
        stale = LD.forward(net, s, feats, c["image"])[0]
        LD.refresh(net)
        got3 = LD.forward(net, s, feats, c["image"])[0]
        stock = net(s, feats, c["image"])[0]
    assert torch.equal(stale, got2) and not torch.equal(got3, got2)
    err = float((got3 - stock).abs().max())
    print(f"\nafter refresh(): max |fused - stock on device| = {err:.3e}")
    assert err <= 2 * ATOL                                                # both sides within 1e-4 of the exact value


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(decoder=True)
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
def test_install_dispatches_the_bundles_lwl_net_and_the_rts_class(amd):
    from oracle import tracker_harness as TH
    from ltr.models.rts.decoder import RTSDecoder
    c = synth.LWL_DECODER_CASES["deployed"]
    s, feats = DC.inputs("deployed", DEV)
    lwl = TH.build_lwl(4900).to(DEV).decoder
    torch.manual_seed(4901)
    rts = RTSDecoder(c["ic"], c["mdim"], OrderedDict((L, fc) for L, fc, _, _ in c["levels"]), use_bn=True).to(DEV).eval()
    for dec in (lwl, rts):
        key = type(dec).__name__ + ".forward"
        amd.stats.clear()
        with torch.no_grad():
            mask, outs = dec(s, feats, c["image"], ("layer4_dec", "layer1_dec"))
            want_mask, want = amd.original(type(dec), "forward")(dec, s, feats, c["image"], ("layer4_dec", "layer1_dec"))
        assert amd.stats[key + ".fast"] == 1 and amd.stats[key + ".reference"] == 0
        assert list(outs) == list(want) == ["layer4_dec", "layer1_dec"] and mask.shape == want_mask.shape
        err = max([float((mask - want_mask).abs().max())] + [float((outs[q] - want[q]).abs().max()) for q in outs])
        print(f"\ninstall(decoder=True), {type(dec).__name__}: max |fused - stock on device| = {err:.3e} (bound 2e-4)")
        assert err <= 2e-4
        with torch.no_grad():
            dec(s[None], feats, c["image"], (), 1)                        # num_objects: the reference branch
        assert amd.stats[key + ".fast"] == 1 and amd.stats[key + ".reference"] == 1
    amd.uninstall()
    assert not hasattr(type(lwl).forward, "__wrapped__") and not hasattr(RTSDecoder.forward, "__wrapped__")


def _segment_scores(amd, decoder):
    from oracle import tracker_harness as TH
    import tracker_replay as TR
    amd.uninstall()
    amd.install(decoder=decoder)
    amd.stats.clear()
    _, rec, _ = TH.run_lwl(seed=TH.LWL_RUN["seed"], n_frames=1, dims=TH.LWL_TEST, device="cuda")
    events = TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    return [np.asarray(e["scores"], dtype=np.float64) for e in events if e["kind"] == "lwl_segment"], dict(amd.stats)


@needs_bundle
def test_segment_target_downstream_of_the_fused_learner(amd):
    """initialize() + one track() of the reference LWL tracker: `segment_target` (lwl_net.py) applies the filter of the fused few-shot learner
    and decodes the mask encoding.  With the fused decoder the raw scores stay within 2e-4 of the same run with the stock decoder."""
    fused, stats = _segment_scores(amd, True)
    stock, _ = _segment_scores(amd, False)
    assert stats.get("LWTLDecoder.forward.fast", 0) >= 1 and stats.get("LWTLDecoder.forward.reference", 0) == 0, stats
    assert stats.get("GNSteepestDescent.fast", 0) >= 1, stats
    assert len(fused) == len(stock) >= 1
    err = max(float(np.abs(a - b).max()) for a, b in zip(fused, stock))
    print(f"\nsegment_target: max |scores with fused decoder - with stock decoder| = {err:.3e} (bound 2e-4), max |s| {max(np.abs(b).max() for b in stock):.3f}")
    assert err <= 2e-4
