"""The LWL / RTS feature heads on the MI355X (pt_feat_head_f32 through pytracking_amd.features): the six small cases of
synth.FEAT_HEAD_CASES at stride 2 and the deployed 1024 x 30 x 52 -> 512 head at both strides against the float64 stand-in of
tests/feat_head_cases.py, within FACTOR x the fp32 CPU stand-in's own distance from float64 on the same case; the committed goldens of
the unmodified reference within the project's 1e-4; stride 1 bit-equal to pt_clf_head_f32; an exact-sum case (integer operands: every
convolution sum is exact in fp32 in any order, so only the norm factor rounds) to rtol 1e-6; leading dimensions, bit-identical repeats,
graph capture, the weight cache; install(feature_heads=True) on the bundle's LWL net and one LWL model update downstream of the fused
head.

Measured on the MI355X (max |out - float64| / ref_err; profiles/feat_head_f64.txt), bound 4x:
  stride 2  one 1.23x  two_three 0.41x  cout36 0.70x  odd_h 1.06x  straddle 1.14x  map 0.83x  deployed 1.29x  deployed, n = 2 1.44x
  stride 1  deployed 1.33x

Every test prints its measured figures before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import f64_bound
import feat_head_cases as FC
from f64_bound import needs_bundle
from oracle import ref_harness
from pytracking_amd import _lib, features as FM, synth
from pytracking_amd.filter import _ptr, _stream, workspace

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4


def _head(w, stride, scale=FC.SCALE, basic=False):
    """The fused head with the weight `w` (Cout, Cin, 3, 3) on the device."""
    Cout, Cin = w.shape[:2]
    if basic:
        head = FM.residual_basic_block(feature_dim=Cin, num_blocks=0, l2norm=True, final_conv=True, norm_scale=scale, out_dim=Cout)
    else:
        head = FM.residual_bottleneck(feature_dim=Cout, num_blocks=0, l2norm=True, final_conv=True, norm_scale=scale, out_dim=Cout,
                                      input_dim=Cin, final_stride=stride)
    head.load_state_dict({"0.weight": w.clone()}, strict=True)
    return head.to(DEV).eval()


def _abi(x, w, stride):
    """One call of the C ABI on device tensors: pt_feat_head_f32 at `stride`, pt_clf_head_f32 for stride None."""
    L = _lib.lib()
    n, Cin, H, W = x.shape
    Cout = w.shape[0]
    wt = w.permute(0, 2, 3, 1).contiguous()
    ho, wo = FC.out_hw(H, W, stride or 1)
    out = torch.empty(n, Cout, ho, wo, device=x.device)
    if stride is None:
        ws = workspace(L.pt_clf_head_ws_bytes(n, Cin, Cout, H, W), x.device)
        rc = L.pt_clf_head_f32(_ptr(x), _ptr(wt), _ptr(out), n, Cin, Cout, H, W, FC.SCALE, FC.EPS, _ptr(ws), ws.numel(), _stream())
    else:
        ws = workspace(L.pt_feat_head_ws_bytes(n, Cin, Cout, H, W, stride), x.device)
        rc = L.pt_feat_head_f32(_ptr(x), _ptr(wt), _ptr(out), n, Cin, Cout, H, W, stride, FC.SCALE, FC.EPS, _ptr(ws), ws.numel(),
                                _stream())
    _lib.check(rc, "head")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", FC.CASES)
def test_stride_2_within_the_float64_bound_and_the_golden(name):
    x, w, a = FC.small(name)
    n, Cin, Cout, H, W = synth.FEAT_HEAD_CASES[name]
    head = _head(w, 2)
    with torch.no_grad():
        out = head(x.to(DEV))
        again = head(x.to(DEV))
    assert out.shape == (n, Cout, *FC.out_hw(H, W, 2))
    err = f64_bound.errors(a.want, out)[""]
    g = FC.golden(name)
    gerr = float(np.abs(out.cpu().numpy() - g["out"]).max())
    print(f64_bound.report(f"feat_head_{name} stride 2", {"": err}, a.ref_err) + f"  max |gpu - reference fp32 golden| {gerr:.3e} (bound {ATOL:.0e})")
    assert err <= f64_bound.bound(a.ref_err)
    assert gerr <= ATOL
    assert torch.equal(out, again)                                      # two calls are bit-identical


@pytest.mark.parametrize("name", FC.CASES)
def test_stride_1_is_the_classification_head_bit_for_bit(name):
    x, w, a = FC.small(name, stride=1)
    xd, wd = x.to(DEV), w.to(DEV)
    new, old = _abi(xd, wd, 1), _abi(xd, wd, None)
    err = f64_bound.errors(a.want, new)[""]
    print(f64_bound.report(f"feat_head_{name} stride 1", {"": err}, a.ref_err))
    assert torch.equal(new, old)
    with torch.no_grad():
        assert torch.equal(_head(w, 1, basic=True)(xd), old)            # the host module at stride 1 stays on pt_clf_head_f32
    assert err <= ATOL


def test_exact_sums():
    """Integer operands from -2 ... 2: every product and every partial sum is an integer below 2^24, exact in fp32 in any order, so the
    device and float64 agree on y to the bit and differ by a handful of roundings in the norm factor.  Any indexing error is O(1)."""
    n, Cin, Cout, H, W = 2, 64, 16, 5, 8
    x, w = (torch.from_numpy(t) for t in synth.feat_head_problem(77, n, Cin, Cout, H, W, integers=True))
    want = FC.standin(x.double(), w.double(), 2).numpy()
    with torch.no_grad():
        got = _head(w, 2)(x.to(DEV)).cpu().numpy()
    rel = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30) * (want != 0)))
    print(f"\nexact sums {(n, Cin, Cout, H, W)}: max relative error {rel:.3e} (rtol 1e-6), zeros {int((want == 0).sum())}")
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("n,stride,basic", [(1, 2, False), (1, 1, True), (2, 2, False)])
def test_deployed_shapes(n, stride, basic):
    """1024 x 30 x 52 -> 512: the RTS classifier head (stride 2), the LWL / RTS target-model head (stride 1, through
    features.residual_basic_block), and two images at stride 2."""
    x, w, a = FC.deployed(n, stride, 2400 + 10 * n + stride)
    with torch.no_grad():
        out = _head(w, stride, basic=basic)(x.to(DEV))
    assert out.shape == (n, 512, *FC.out_hw(30, 52, stride))
    f64_bound.held(f"feat_head deployed n = {n} stride {stride}", out, a.want, a.ref_err)


def test_leading_dimensions_are_preserved():
    x, w, a = FC.small("odd_h")                                         # (2, 128, 5, 8)
    head = _head(w, 2)
    with torch.no_grad():
        flat = head(x.to(DEV))
        five = head(x.to(DEV).reshape(2, 1, 128, 5, 8))
        three = head(x.to(DEV)[0])
    assert five.shape == (2, 1, 32, 3, 4) and torch.equal(five.reshape(flat.shape), flat)
    assert three.shape == (32, 3, 4) and torch.equal(three, flat[0])


@pytest.mark.parametrize("name", ["straddle", "deployed"])
def test_graph_capture_replays_the_eager_bits(name):
    x, w, _ = FC.deployed(1, 2, 2412) if name == "deployed" else FC.small(name)
    head, xd = _head(w, 2), x.to(DEV)
    with torch.no_grad():
        eager = head(xd)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            head(xd)                                                    # warm-up: workspace allocated outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = head(xd)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_cache_follows_load_state_dict_and_in_place_updates():
    x, w, _ = FC.small("cout36")
    other = torch.from_numpy(synth.feat_head_problem(FC.SEED + 50, *synth.FEAT_HEAD_CASES["cout36"])[1])
    head, xd = _head(w, 2), x.to(DEV)
    with torch.no_grad():
        first = head(xd)
        head.load_state_dict({"0.weight": other})
        got = head(xd)
        assert torch.equal(got, _head(other, 2)(xd)) and not torch.equal(got, first)
        head[0].weight[:, :, 0, 0].mul_(-1.5)                           # in place
        changed = head[0].weight.detach().cpu().clone()
        got2 = head(xd)
        assert torch.equal(got2, _head(changed, 2)(xd)) and not torch.equal(got2, got)
        f = FC.standin(xd, head[0].weight.detach(), 2)                  # stock PyTorch on the device
    err = float((got2 - f).abs().max())
    print(f"\nafter the in-place change: max |fused - stock on device| = {err:.3e}")
    assert err <= 2 * ATOL


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    amd.install(feature_heads=True)
    try:
        yield amd
    finally:
        amd.uninstall()


@needs_bundle
def test_install_dispatches_the_bundles_lwl_net(amd):
    from oracle import tracker_harness as TH
    net = TH.build_lwl(4900).to(DEV)
    fe = net.target_model.feature_extractor
    assert isinstance(fe, FM.ClfHead) and (fe[0].in_channels, fe[0].out_channels, fe[0].stride) == (1024, 512, (1, 1))
    x = torch.from_numpy(synth.feat_head_problem(2450, 1, 1024, 512, 30, 52)[0]).to(DEV)
    amd.stats.clear()
    with torch.no_grad():
        out = net.target_model.extract_target_model_features(x)
        stock = torch.nn.Sequential.forward(fe, x)
    assert amd.stats["residual_basic_block.fast"] == 1 and amd.stats["residual_basic_block.reference"] == 0
    err = float((out - stock).abs().max())
    print(f"\ninstall(feature_heads=True), LWL net: max |fused - stock on device| = {err:.3e} (bound 2e-4), max |v| {float(stock.abs().max()):.3f}")
    assert out.shape == stock.shape == (1, 512, 30, 52) and err <= 2e-4
    fe.train()
    with torch.no_grad():
        fe(x[:, :, :4, :4])                                             # training mode: the reference branch
    assert amd.stats["residual_basic_block.fast"] == 1 and amd.stats["residual_basic_block.reference"] == 1


def _lwl_filters(amd, feature_heads):
    """The filters of the first-frame model and of one per-frame update of the reference LWL tracker on the device."""
    from oracle import tracker_harness as TH
    import tracker_replay as TR
    amd.uninstall()
    amd.install(feature_heads=feature_heads)
    amd.stats.clear()
    _, rec, _ = TH.run_lwl(seed=TH.LWL_RUN["seed"], n_frames=2, dims=TH.LWL_TEST, device="cuda")
    events = TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    return {e["kind"]: np.asarray(e["filter"], dtype=np.float64) for e in events if e["kind"] in ("lwl_init", "lwl_update")}, dict(amd.stats)


@needs_bundle
def test_lwl_update_downstream_of_the_fused_head(amd):
    """One initialize() + two track() calls of the reference LWL tracker: every frame's backbone features go through the target-model head
    (lwl.py: extract_target_model_features) before the learner and the segmentation.  With the fused head the filters stay within the 1e-4
    tests/test_trackers_on_device.py holds LWL filters to, measured against the same run with the stock head."""
    fused, stats = _lwl_filters(amd, True)
    stock, stock_stats = _lwl_filters(amd, False)
    assert stats.get("residual_basic_block.fast", 0) >= 3 and stats.get("residual_basic_block.reference", 0) == 0, stats   # init + 2 frames
    assert not any(k.startswith("residual_basic_block") for k in stock_stats), stock_stats
    assert set(fused) == {"lwl_init", "lwl_update"} == set(stock)
    for kind in ("lwl_init", "lwl_update"):
        err = float(np.abs(fused[kind] - stock[kind]).max())
        print(f"\n{kind}: max |filter with fused head - with stock head| = {err:.3e} (bound {ATOL:.0e}), max |w| {np.abs(stock[kind]).max():.3f}")
        assert err <= ATOL
