"""Box label encoders on the MI355X (box_enc.hip through pytracking_amd.box_encoder): every case of synth.BOX_ENC_CASES and
synth.BOX_CAT_ENC_CASES, every output, within FACTOR x max(ref_err, one fp32 ulp of the output's range) of the float64 stand-in
(tests/box_enc_cases.py; ref_err = the fp32 CPU stand-in's own distance from float64 on that case, 8 threads; FACTOR is the project's,
tests/f64_bound.py) and within the golden's distance (the CPU bound of tests/test_box_enc_cpu.py plus the float64 bound); bit-identical
repeats, graph capture, feature views, box dtypes, the weight cache, and install(box_encoder=True) on the reference's four classes.
tests/test_box_enc_cpu.py shows that the float64 bound rejects a doubled BatchNorm eps, 10-bit weights and a box moved by a pixel.

Every test prints its measured error before it asserts (run with -s); the worst multiple of ref_err per case is in
profiles/box_enc_f64.txt.  Reads nothing of the reference tree except where marked."""
import numpy as np
import pytest
import torch

import box_enc_cases as BC
import f64_bound
from f64_bound import needs_bundle
from oracle import ref_harness
from pytracking_amd import box_encoder as BE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_RUNS = {}


def _bound(a):
    return f64_bound.bound(a.ref_err, floor=f64_bound.spacing_of_max(a.want))


def _layers_crossed(kind, c):
    return 8 if kind == BC.BOX else 2 * (len(c["dims"]) - 1) + 1


def _run(kind, name):
    """(module on the device, device arguments, {output: (n, F, h, w) device tensor}) of a case, once per session."""
    if (kind, name) not in _RUNS:
        _, c, _, boxes, feat = BC.case(kind, name)
        net = BC.module(kind, name, DEV)
        args = BC.call_args(kind, c, boxes, feat, DEV)
        with torch.no_grad():
            assert BE.covered(net, *args)
            out = BE.forward(net, *args)
        _RUNS[(kind, name)] = (net, args, out)
    return _RUNS[(kind, name)]


def _named(kind, c, out):
    out = out if kind == BC.BOX else (out,)
    return {q: out[k].reshape(-1, *out[k].shape[-3:]) for k, q in enumerate(BC.outputs(kind, c))}


@pytest.mark.parametrize("kind,name", BC.ALL)
def test_matches_float64_and_golden(kind, name):
    g, c, _, boxes, feat = BC.case(kind, name)
    net, args, out = _run(kind, name)
    n, (h, w), F = c["n"], c["feat"], c["dims"][-1]
    if kind == BC.BOX:
        assert out[0].shape == (n, 1, F, h, w) and (out[1] is None) == (not c["use_sample_w"])
        assert out[1] is None or out[1].shape == out[0].shape
    else:
        assert out.shape == (n, 1, F, h, w)
    got = {q: t.cpu().numpy() for q, t in _named(kind, c, out).items()}
    a = BC.anchor(kind, name)
    bound = _bound(a)
    f64_bound.held(f"{kind}_{name}", got, a.want, a.ref_err, floor=f64_bound.spacing_of_max(a.want))
    gerr = max(float(np.abs(got[q] - g[q]).max()) for q in got)
    gbound = float(g["ref_fp32_err"]) + _layers_crossed(kind, c) * float(g["max_abs"]) * 2.0 ** -24 + 1e-12 + bound
    print(f"{kind}_{name}: max |gpu - reference fp32 golden| = {gerr:.3e} (bound {gbound:.3e})")
    assert gerr <= gbound
    with torch.no_grad():
        again = BE.forward(net, *args)
    for q, t in _named(kind, c, again).items():
        assert torch.equal(t, _named(kind, c, out)[q]), q                # two calls are bit-identical


@pytest.mark.parametrize("kind,name", [(BC.BOX, "odd"), (BC.BOX, "deployed"), (BC.CAT, "blocks3"), (BC.CAT, "deployed")])
def test_graph_capture_replays_the_eager_bits(kind, name):
    _, c, _, _, _ = BC.case(kind, name)
    net, args, out = _run(kind, name)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            BE.forward(net, *args)                                      # warm-up: pack and workspace exist before the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = BE.forward(net, *args)
        graph.replay()
        torch.cuda.synchronize()
    for q, t in _named(kind, c, captured).items():
        assert torch.equal(t, _named(kind, c, out)[q]), q


@pytest.mark.parametrize("kind", BC.KINDS)
def test_feature_views_and_box_dtypes(kind):
    _, c, _, boxes, feat = BC.case(kind, "odd")
    net, (bb, ft, sz), out = _run(kind, "odd")
    want = _named(kind, c, out)
    n, C, h, w = ft.shape
    with torch.no_grad():
        padded = torch.zeros(n, C + 3, h + 2, w + 5, device=DEV)
        padded[:, 1:C + 1, 1:h + 1, 2:w + 2] = ft
        view = padded[:, 1:C + 1, 1:h + 1, 2:w + 2]                     # nothing dense about it
        assert not view.is_contiguous() and BE.covered(net, bb, view, sz)
        planes = torch.zeros(n, C + 2, h, w, device=DEV)
        planes[:, :C] = ft
        strided = planes[:, :C]                                         # dense planes, a larger image stride: passed as it is
        flat = torch.zeros(ft.numel() + 1, device=DEV)
        flat[1:] = ft.reshape(-1)
        offset = flat[1:].view(n, C, h, w)                              # 4 bytes off the allocation's alignment
        assert offset.data_ptr() % 16 == 4
        five = ft.view(n, 1, C, h, w) if kind == BC.BOX else ft
        for tag, f in (("view", view), ("strided", strided), ("offset", offset), ("5-D", five)):
            got = _named(kind, c, BE.forward(net, bb, f, sz))
            assert all(torch.equal(got[q], want[q]) for q in want), tag
        ints = torch.tensor([[int(v) for v in b] for b in boxes.tolist()], device=DEV).reshape(bb.shape)
        for tag, b in (("float64", bb.double()), ("int64", ints), ("int32", ints.int()), ("half", bb.half())):
            assert BE.covered(net, b, ft, sz), tag
            got = _named(kind, c, BE.forward(net, b, ft, sz))
            assert all(torch.equal(got[q], want[q]) for q in want), tag
        assert not BE.covered(net, bb[0] if kind == BC.BOX else bb[:, None], ft, sz)             # the wrong rank
        assert not BE.covered(net, bb, ft.double(), sz) and not BE.covered(net, bb, ft.half(), sz)
        with pytest.raises(NotImplementedError, match="box label encoder"):
            BE.forward(net, bb, ft.double(), sz)
        net.train()
        assert not BE.covered(net, bb, ft, sz)
        net.eval()
    ft_grad = ft.clone().requires_grad_(True)
    assert not BE.covered(net, bb, ft_grad, sz)
    with torch.no_grad():
        assert BE.covered(net, bb, ft_grad, sz)


@pytest.mark.parametrize("kind,name", [(BC.BOX, "bn"), (BC.CAT, "blocks1")])
def test_cache_follows_the_state_and_refresh(kind, name):
    _, c, _, boxes, feat = BC.case(kind, name)
    net = BC.module(kind, name, DEV)
    args = BC.call_args(kind, c, boxes, feat, DEV)
    bn = net.label_pred[1] if kind == BC.BOX else net.res[0].bn1
    with torch.no_grad():
        first = _named(kind, c, BE.forward(net, *args))
        bn.running_var.mul_(1.7)                                        # in place: the version counter moves
        second = _named(kind, c, BE.forward(net, *args))
        stock = BC.run(kind, net, args, c)
        assert not torch.equal(second["label_enc"], first["label_enc"])
        err = float((second["label_enc"] - stock["label_enc"]).abs().max())
        print(f"\n{kind}_{name} after the in-place change: max |fused - stock on device| = {err:.3e}")
        assert err <= 2 * _bound(BC.anchor(kind, name)) + 1e-6
        conv = net.label_pred[0]
        conv.bias.data[:] = conv.bias.data + 0.5                        # through .data, same storage: nothing the key sees
        stale = _named(kind, c, BE.forward(net, *args))
        assert torch.equal(stale["label_enc"], second["label_enc"])     # the cached pack
        BE.refresh(net)
        fresh = _named(kind, c, BE.forward(net, *args))
        assert not torch.equal(fresh["label_enc"], second["label_enc"])
        stock = BC.run(kind, net, args, c)
        assert float((fresh["label_enc"] - stock["label_enc"]).abs().max()) <= 2 * _bound(BC.anchor(kind, name)) + 1e-6


@pytest.fixture()
def amd():
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


def _reference_net(pkg, kind, c, sd):
    import importlib
    M = importlib.import_module(f"ltr.models.{pkg}.label_encoder")
    kw = dict(layer_dims=c["dims"], feat_dim=c["feat_dim"], use_final_relu=c["final_relu"], use_gauss=False, use_bn=c["use_bn"])
    net = (M.ResidualDS16FeatSWBox(use_sample_w=c["use_sample_w"], **kw) if kind == BC.BOX
           else M.ResidualDS16FeatSWBoxCatMultiBlock(final_bn=c["final_bn"], **kw))
    net.load_state_dict(BC.state_tensors(sd))
    return net.to(DEV).eval()


@needs_bundle
@pytest.mark.parametrize("pkg", ["lwl", "rts"])
@pytest.mark.parametrize("kind,name", [(BC.BOX, "deployed"), (BC.CAT, "deployed")])
def test_install_dispatches_the_references_classes(amd, pkg, kind, name):
    """Reads the reference's classes through the bundle (oracle/_ref)."""
    _, c, sd, boxes, feat = BC.case(kind, name)
    args = BC.call_args(kind, c, boxes, feat, DEV)
    net = _reference_net(pkg, kind, c, sd)
    cname = type(net).__name__
    ref_forward = type(net).__dict__["forward"]
    stock = BC.run(kind, net, args, c)                                  # switch off: the reference's own code
    amd.install()
    assert type(net).__dict__["forward"] is ref_forward                 # the default install leaves the classes alone
    amd.uninstall()
    amd.install(box_encoder=True)
    amd.stats.clear()
    got = BC.run(kind, net, args, c)
    assert amd.stats[cname + ".forward.fast"] == 1 and amd.stats[cname + ".forward.reference"] == 0
    a = BC.anchor(kind, name)
    err = max(float((got[q] - stock[q]).abs().max()) for q in got)
    print(f"\ninstall(box_encoder=True), {pkg} {cname}: max |fused - stock on device| = {err:.3e} (bound 2 x {_bound(a):.3e})")
    assert err <= 2 * _bound(a)                                         # both sides within the bound of float64
    assert max(f64_bound.errors(a.want, {q: t.cpu().numpy() for q, t in got.items()}).values()) <= _bound(a)
    net.train()
    with torch.no_grad():
        net(*args)
    assert amd.stats[cname + ".forward.fast"] == 1 and amd.stats[cname + ".forward.reference"] == 1
