"""The ResNet backbone forward on the MI355X (csrc_bbn/backbone.hip through the C ABI of include/pt_bbn.h and through
pytracking_amd.backbone) against the float64 run of the unmodified reference classes (tests/golden/backbone_*.npz) on the whole case table
(tests/backbone_cases.py).

Bound.  Every output layer lies within FACTOR x max(ref_err, 2^-23 max|want|) of float64: the bound of tests/f64_bound.py with its
ulp_of_max floor, ref_err being the reference's own fp32 distance from its float64 run of that case on the CPU (the golden's <o>_ref_err,
over the whole map).  Maps of more than 65 536 elements are compared at the golden's fixed positions.  The workspace and the outputs are
NaN prefilled and sit between NaN guard regions.  Figures are printed before they are asserted and, when BACKBONE_F64_OUT names a file,
written there as a table (profiles/backbone_f64.txt is the table of such a run)."""
import ctypes

import numpy as np
import pytest
import torch

import backbone_cases as C
import backbone_np as RN
import f64_bound
from pytracking_amd import _lib_bbn as K
from pytracking_amd import backbone as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# worst ratio of a device output to max(ref_err, ulp of max) measured on the MI355X (profiles/backbone_f64.txt)
WORST_MEASURED = 1.83
F_MAX = 32                                         # tests/test_backbone_cpu.py: every seeded defect misses this many units
FACTOR = f64_bound.raised_factor(WORST_MEASURED, F_MAX)
TABLE = f64_bound.Table("BACKBONE_F64_OUT",
                        "ResNet backbone forward on the MI355X against float64 (tests/test_gpu_backbone.py):\n"
                        "per case and output layer max |out - float64| and its ratio to max(ref_err, 2^-23 max|want|) -- the unmodified reference's\n"
                        f"own fp32 distance from its float64 run of that case on the CPU, floored at one fp32 ulp of the map's range; bound = {FACTOR} x that.")
GUARD = 64                                         # floats of NaN in front of and behind every buffer: 256 bytes, keeps the alignment


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_MODULES = {}


def module(name):
    """the stand-in of the case on the device, its input and its pack"""
    if name not in _MODULES:
        c = C.CASES[name]
        m = RN.standin(c["spec"], C.params(name), c["outputs"], DEV)
        _MODULES[name] = (m, f64_bound.dev(C.image(name), DEV), B.packed_weights(m))
    return _MODULES[name]


class Call:
    """One pt_bbn_forward_f32 call of a case: workspace and outputs in ONE NaN-prefilled device tensor, each between two guards."""

    def __init__(self, name, outputs=None):
        self.m, self.x, self.pack = module(name)
        self.outputs = [o for o in C.ALL if o in (outputs or C.CASES[name]["outputs"])]
        self.mask = sum(1 << C.ALL.index(o) for o in self.outputs)
        self.net = B.describe(self.m)
        n, _, H, W = self.x.shape
        L, d = K.lib(), ctypes.byref(self.net.desc)
        rows = (K.BbnLaunch * K.PT_BBN_MAX_LAUNCHES)()
        count = L.pt_bbn_plan(d, n, H, W, self.mask, rows)
        assert count > 0
        self.rows = list(rows[:count])
        self.shapes = {C.ALL[r.out]: (n, r.N, r.Hout, r.Wout) for r in self.rows if r.out >= 0}
        assert list(self.shapes) == self.outputs
        self.ws_bytes = L.pt_bbn_ws_bytes(d, n, H, W, self.mask)
        assert self.ws_bytes > 0 and self.ws_bytes % 256 == 0
        sizes = [self.ws_bytes // 4] + [(int(np.prod(s)) + 63) // 64 * 64 for s in self.shapes.values()]
        self.at = np.cumsum([GUARD] + [s + GUARD for s in sizes])[:-1]
        self.sizes = sizes
        self.t = torch.full((int(self.at[-1] + sizes[-1] + GUARD),), float("nan"), device=DEV)
        assert self.t.data_ptr() % 256 == 0

    def ptr(self, i):
        return self.t.data_ptr() + 4 * int(self.at[i])

    def run(self):
        outs = (ctypes.c_void_p * K.PT_BBN_OUT_COUNT)()
        for i, o in enumerate(self.outputs):
            outs[C.ALL.index(o)] = self.ptr(1 + i)
        n, _, H, W = self.x.shape
        rc = K.lib().pt_bbn_forward_f32(ctypes.byref(self.net.desc), self.pack.data_ptr(), self.x.data_ptr(), n, H, W, self.mask, outs, self.ptr(0),
                                        self.ws_bytes, stream())
        assert rc == 0, K.lib().pt_bbn_strerror(rc)

    def result(self):
        """{output: device tensor (a copy)} after checking that every guard and every pad behind an output still holds its NaN"""
        torch.cuda.synchronize()
        kept = torch.ones_like(self.t, dtype=torch.bool)
        kept[int(self.at[0]):int(self.at[0]) + self.sizes[0]] = False                    # the workspace
        out = {}
        for i, (o, s) in enumerate(self.shapes.items()):
            a, count = int(self.at[1 + i]), int(np.prod(s))
            kept[a:a + count] = False
            out[o] = self.t[a:a + count].reshape(s).clone()
        assert bool(torch.isnan(self.t[kept]).all()), "a guard region was written"
        assert not any(bool(torch.isnan(v).any()) for v in out.values()), "NaN in an output"
        return out


_FIRST = {}


def first_run(name):
    if name not in _FIRST:
        call = Call(name)
        call.run()
        _FIRST[name] = (call, call.result())
    return _FIRST[name]


def check(tag, name, outs, star=False):
    g = C.golden(name)
    for o, v in outs.items():
        assert tuple(v.shape) == tuple(g[o + "_shape"])
        full = v.double().cpu().numpy()
        f64_bound.held(f"{tag} {o}", C.at_subset(name, o, full), g[o + "_f64"], float(g[o + "_ref_err"]), factor=FACTOR,
                       floor=f64_bound.ULP * float(g[o + "_max"]), table=TABLE, star=star)
        # what the stored positions do not see: the whole map's sum, within the bound per element
        unit = f64_bound.bound(float(g[o + "_ref_err"]), FACTOR, f64_bound.ULP * float(g[o + "_max"]))
        assert abs(full.sum() - float(g[o + "_sum"])) <= unit * full.size and abs(np.abs(full).sum() - float(g[o + "_abssum"])) <= unit * full.size


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_through_the_c_abi(name):
    check(name, name, first_run(name)[1])


@pytest.mark.parametrize("name", list(C.CASES))
def test_golden_fp32_runs_are_within_the_bound_of_their_float64(name):
    g = C.golden(name)
    for o in C.CASES[name]["outputs"]:
        f64_bound.held(f"{name} {o} reference fp32", g[o + "_f32"].astype(np.float64), g[o + "_f64"], float(g[o + "_ref_err"]), factor=FACTOR,
                       floor=f64_bound.ULP * float(g[o + "_max"]))


@pytest.mark.parametrize("name", C.SMALL + ["r50_288"])
def test_repeat_and_two_graph_replays_are_bit_equal(name):
    call, want = first_run(name)
    call.run()
    again = call.result()
    assert all(torch.equal(again[o], want[o]) for o in want)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.run()                                                        # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call.run()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for i in range(len(call.shapes)):
            a = int(call.at[1 + i])
            call.t[a:a + call.sizes[1 + i]] = float("nan")
        graph.replay()
        replayed = call.result()
        assert all(torch.equal(replayed[o], want[o]) for o in want)


@pytest.mark.parametrize("name", [n for n in C.SMALL if len(C.CASES[n]["outputs"]) > 1] + ["r50_288"])
def test_a_strict_subset_of_the_outputs_equals_the_full_run(name):
    _, want = first_run(name)
    outputs = C.CASES[name]["outputs"]
    for sub in ([outputs[0]], [outputs[-1]], outputs[1:-1]):
        if not sub:
            continue
        call = Call(name, sub)
        deepest = max(C.ALL.index(o) for o in sub)
        assert max(r.layer for r in call.rows) == deepest or (deepest == 0 and max(r.layer for r in call.rows) == 0)
        call.run()
        got = call.result()
        assert list(got) == sub and all(torch.equal(got[o], want[o]) for o in sub), (name, sub)


@pytest.mark.parametrize("name", ["bott_odd_n2", "basic_tiny", "mrcnn_tiny", "conv1_only_mrcnn"])
def test_python_path_equals_the_abi_and_caches_the_pack(name):
    m, x, pack = module(name)
    _, want = first_run(name)
    with torch.no_grad():
        assert B.covered(m, x)
        got = B.forward(m, x)
        assert list(got) == list(want) and all(torch.equal(got[o], want[o]) for o in want)
        assert B.packed_weights(m) is pack                                     # the second call hits the cache
        sub = B.forward(m, x, [C.CASES[name]["outputs"][-1]])
        assert list(sub) == [C.CASES[name]["outputs"][-1]] and torch.equal(sub[list(sub)[0]], want[list(sub)[0]])
        kept = m.bn1.running_mean.clone()                                      # (x + 0.25) - 0.25 is not x in fp32: the statistic is put back from a copy
        try:
            m.bn1.running_mean.add_(0.25)                                      # a changed BatchNorm statistic invalidates the pack
            changed = B.forward(m, x)
            assert B.packed_weights(m) is not pack and not torch.equal(changed[list(want)[0]], want[list(want)[0]])
        finally:
            m.bn1.running_mean.copy_(kept)
        assert all(torch.equal(v, want[o]) for o, v in B.forward(m, x).items())
        # outside: the reasons, in the dispatcher's order
        assert B.why_not(m, x.cpu()) == "CPU input" and B.why_not(m, x.double()) == "input that is not contiguous fp32"
        assert B.why_not(m, x.permute(0, 1, 3, 2)) == "input that is not contiguous fp32" and B.why_not(m, x, ["fc"]) == "outputs outside conv1 / layer1..4"
    assert B.why_not(m, x) == "gradients enabled"
    with pytest.raises(NotImplementedError):
        B.forward(m, x)


def _installed_features(make, shape):
    """(fast, stock fp32, stock float64) backbone features of the unmodified network `make()` builds, and the stats of the fast call"""
    from pytracking_amd import install as amd
    amd.uninstall()
    torch.manual_seed(3)
    im = torch.rand(shape, device=DEV) * 2 - 1
    try:
        amd.install(backbone=True)
        net = make().to(DEV).eval()
        amd.stats.clear()
        with torch.no_grad():
            fast = net.extract_backbone_features(im)
        stats = dict(amd.stats)
    finally:
        amd.uninstall()
    with torch.no_grad():
        stock = net.extract_backbone_features(im)
        net.feature_extractor.double()
        want = net.feature_extractor(im.double(), net.output_layers)
    return fast, stock, want, stats


@f64_bound.needs_bundle
@pytest.mark.parametrize("which", ["dimpnet50", "lwl_resnet50"])
def test_the_unmodified_networks_take_the_fast_backbone(which):
    from oracle import ref_harness
    ref_harness.install()
    if which == "dimpnet50":
        from ltr.models.tracking import dimpnet
        make, shape = (lambda: dimpnet.dimpnet50(backbone_pretrained=False)), (1, 3, 288, 288)
    else:
        from ltr.models.lwl import lwl_net
        make, shape = (lambda: lwl_net.steepest_descent_resnet50(          # ltr/train_settings/lwl/lwl_stage2.py:94-102
            filter_size=3, num_filters=16, optim_iter=5, backbone_pretrained=False, out_feature_dim=512, label_encoder_dims=(16, 32, 64),
            use_bn_in_label_enc=False, clf_feat_blocks=0, final_conv=True, backbone_type="mrcnn")), (1, 3, 240, 416)
    fast, stock, want, stats = _installed_features(make, shape)
    assert stats.get("ResNet.forward.fast") == 1 and not stats.get("ResNet.forward.reference"), stats
    assert list(fast) == list(stock) == list(want)
    for o in want:
        ref_err = float((stock[o].double() - want[o]).abs().max())
        f64_bound.held(f"{which} {o}", fast[o], f64_bound.host(want[o]), ref_err, factor=FACTOR, floor=f64_bound.ulp_of_max, table=TABLE, star=True)
