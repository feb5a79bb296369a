"""Mask label encoder on the MI355X (label_enc.hip through pytracking_amd.label_encoder): every case of synth.LABEL_ENC_CASES against the
golden of the unmodified reference's fp32 CPU run (tools/make_golden_label_enc.py) within the project's 1e-4 absolute -- the reference's
own distance from float64 is recorded in each golden and is at most 3.8e-6 -- the deployed size at 8 and 32 masks (the tile shapes the
n = 2 golden does not reach), bit-identical repeats, graph capture, mask views, the weight cache, install(label_encoder=True) on the
bundle's LWL net, and one LWL model update downstream of the fused encoder.

Every test prints its measured maximum error before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import label_enc_cases as LC
from f64_bound import dev, needs_bundle
from oracle import ref_harness
from pytracking_amd import label_encoder as LE, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4


def _run(name):
    g, n, H, W, dims, use_bn, sd, masks = LC.case(name)
    net = LC.module(name, DEV)
    with torch.no_grad():
        m = dev(masks)[:, None]                                        # (frames, 1 sequence, H, W)
        assert LE.covered(net, m)
        enc, sw = LE.forward(net, m)
    return g, net, m, enc, sw


@pytest.mark.parametrize("name", LC.CASES)
def test_matches_reference_golden(name):
    g, net, m, enc, sw = _run(name)
    n, H, W, dims, use_bn = synth.LABEL_ENC_CASES[name]
    h, w = LC.out_hw(H, W)
    assert enc.shape == (n, 1, dims[3], h, w) and sw.shape == enc.shape
    err = LC.against_golden(g, enc.cpu().numpy(), sw.cpu().numpy())
    print(f"\nlabel_enc_{name}: max |gpu - reference fp32| = {err:.3e} (bound {ATOL:.0e}, ref_fp32_err {float(g['ref_fp32_err']):.3e})")
    assert err <= ATOL
    with torch.no_grad():
        enc2, sw2 = LE.forward(net, m)
    assert torch.equal(enc, enc2) and torch.equal(sw, sw2)              # two calls are bit-identical


@pytest.mark.parametrize("copies", [4, 16])
def test_deployed_size_with_many_masks(copies):
    """8 and 32 masks of 480 x 832 (the golden's two, repeated): the larger workgroup tiles the convolutions choose once the grid is big
    enough.  Every copy must reproduce the golden."""
    g, net, m, enc, sw = _run("deployed")
    with torch.no_grad():
        big = m.repeat(copies, 1, 1, 1)
        enc_b, sw_b = LE.forward(net, big)
        torch.cuda.synchronize()
    assert enc_b.shape == (2 * copies, 1, *enc.shape[2:])
    worst = 0.0
    for k in range(copies):
        worst = max(worst, LC.against_golden(g, enc_b[2 * k:2 * k + 2].cpu().numpy(), sw_b[2 * k:2 * k + 2].cpu().numpy()))
    print(f"\nlabel_enc_deployed x {copies}: max |gpu - reference fp32| = {worst:.3e} (bound {ATOL:.0e})")
    assert worst <= ATOL
    assert torch.equal(enc_b[:2], enc_b[-2:]) and torch.equal(sw_b[:2], sw_b[-2:])


@pytest.mark.parametrize("name", ["bands", "deployed"])
def test_graph_capture_replays_the_eager_bits(name):
    g, net, m, enc, sw = _run(name)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            LE.forward(net, m)                                          # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            k_enc, k_sw = LE.forward(net, m)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(k_enc, enc) and torch.equal(k_sw, sw)


def test_mask_views_and_sequences():
    g, net, m, enc, sw = _run("odd")                                    # (3, 1, 33, 50)
    n, H, W = m.shape[0], m.shape[2], m.shape[3]
    with torch.no_grad():
        padded = torch.zeros(n, 1, H + 3, W + 5, device=DEV)
        padded[:, :, 1:H + 1, 2:W + 2] = m
        view = padded[:, :, 1:H + 1, 2:W + 2]                           # a non-contiguous view of the same values
        assert not view.is_contiguous() and LE.covered(net, view)
        e1, s1 = LE.forward(net, view)
        assert torch.equal(e1, enc) and torch.equal(s1, sw)
        four = torch.cat([m, m.flip(0)], 0)[:4].reshape(2, 2, H, W)     # frames = 2, seq = 2
        e2, s2 = LE.forward(net, four)
        want_e, want_s = net(four)                                      # the same module in stock PyTorch on the device
    assert e2.shape == (2, 2, enc.shape[2], enc.shape[3], enc.shape[4]) and e2.shape == want_e.shape
    assert torch.equal(e2.reshape(4, *enc.shape[2:])[:3], enc[:, 0])    # (frames, seq) flattens frame-major, as the reference's view
    err = max(float((e2 - want_e).abs().max()), float((s2 - want_s).abs().max()))
    print(f"\nseq = 2: max |fused - stock on device| = {err:.3e}")
    assert err <= 2 * ATOL


def test_cache_follows_load_state_dict_and_in_place_updates():
    g, n, H, W, dims, use_bn, sd, masks = LC.case("bn_odd")
    net = LC.module("bn_odd", DEV)
    m = dev(masks)[:, None]
    other = synth.label_enc_state(int(g["state_seed"]) + 50, dims, use_bn)
    with torch.no_grad():
        first = LE.forward(net, m)
        net.load_state_dict(LC.state_tensors(other))
        fresh = LC.ResidualDS16SW(dims, use_bn)
        fresh.load_state_dict(LC.state_tensors(other))
        want = LE.forward(fresh.to(DEV).eval(), m)
        got = LE.forward(net, m)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], first[0])
        net.res1.bn2.running_var.mul_(1.7)                              # in place
        net.samp_w_pred.bias.add_(0.3)
        changed = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        fresh2 = LC.ResidualDS16SW(dims, use_bn)
        fresh2.load_state_dict(changed)
        want2 = LE.forward(fresh2.to(DEV).eval(), m)
        got2 = LE.forward(net, m)
        stock = net(m)
    assert torch.equal(got2[0], want2[0]) and torch.equal(got2[1], want2[1]) and not torch.equal(got2[1], got[1])
    err = max(float((got2[0] - stock[0]).abs().max()), float((got2[1] - stock[1]).abs().max()))
    print(f"\nafter the in-place change: max |fused - stock on device| = {err:.3e}")
    assert err <= 2 * ATOL                                              # both sides within 1e-4 of the exact value


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(label_encoder=True)
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
def test_install_dispatches_the_bundles_lwl_net(amd):
    from oracle import tracker_harness as TH
    net = TH.build_lwl(4900).to(DEV)
    masks = dev(synth.label_enc_masks(5, 3, 480, 832))[:, None]
    amd.stats.clear()
    with torch.no_grad():
        enc, sw = net.label_encoder(masks)
        stock_enc, stock_sw = amd.original(type(net.label_encoder), "forward")(net.label_encoder, masks)
    assert amd.stats["ResidualDS16SW.forward.fast"] == 1 and amd.stats["ResidualDS16SW.forward.reference"] == 0
    assert enc.shape == stock_enc.shape and sw.shape == stock_sw.shape
    err = max(float((enc - stock_enc).abs().max()), float((sw - stock_sw).abs().max()))
    print(f"\ninstall(label_encoder=True), LWL net: max |fused - stock on device| = {err:.3e} (bound 2e-4)")
    assert err <= 2e-4
    net.label_encoder.train()
    with torch.no_grad():
        net.label_encoder(masks[:1, :, :32, :32])                       # training mode: the reference branch
    assert amd.stats["ResidualDS16SW.forward.fast"] == 1 and amd.stats["ResidualDS16SW.forward.reference"] == 1


def _lwl_filters(amd, label_encoder):
    """The filters of the first-frame model and of one per-frame update of the reference LWL tracker on the device."""
    from oracle import tracker_harness as TH
    import tracker_replay as TR
    amd.uninstall()
    amd.install(label_encoder=label_encoder)
    amd.stats.clear()
    _, rec, _ = TH.run_lwl(seed=TH.LWL_RUN["seed"], n_frames=2, dims=TH.LWL_TEST, device="cuda")
    events = TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    return {e["kind"]: np.asarray(e["filter"], dtype=np.float64) for e in events if e["kind"] in ("lwl_init", "lwl_update")}, dict(amd.stats)


@needs_bundle
def test_lwl_update_downstream_of_the_fused_encoder(amd):
    """One initialize() + two track() calls of the reference LWL tracker (the second one updates the model): `update_target_model`
    (lwl.py:560-578) encodes the stored masks and runs the fused few-shot learner on them.  With the fused encoder the filters stay within the 1e-4 tests/test_trackers_on_device.py
    holds LWL filters to, measured against the same run with the stock encoder."""
    fused, stats = _lwl_filters(amd, True)
    stock, _ = _lwl_filters(amd, False)
    assert stats.get("ResidualDS16SW.forward.fast", 0) >= 2 and stats.get("ResidualDS16SW.forward.reference", 0) == 0, stats
    assert stats.get("GNSteepestDescent.fast", 0) >= 2, stats
    assert set(fused) == {"lwl_init", "lwl_update"} == set(stock)
    for kind in ("lwl_init", "lwl_update"):
        err = float(np.abs(fused[kind] - stock[kind]).max())
        print(f"\n{kind}: max |filter with fused encoder - with stock encoder| = {err:.3e} (bound {ATOL:.0e}), max |w| {np.abs(stock[kind]).max():.3f}")
        assert err <= ATOL
