"""The ResNet backbone forward (include/pt_bbn.h, pytracking_amd/backbone.py) without a GPU: header and bindings, refusals, the plan's routes
against the case table, the float64 restatement against the reference's goldens, and the seeded defects of the restatement."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import backbone_cases as C
import backbone_np as RN
import f64_bound
from pytracking_amd import _abi, _lib, _lib_bbn, _lib_loc, _lib_mem, _lib_mot
from pytracking_amd import backbone as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# raised_factor's cap for the GPU tests: far below the weakest seeded defect (BatchNorm eps dropped: 125 x on bott_c8 / layer3)
F_MAX = 32


@pytest.fixture(scope="module")
def L():
    _lib_bbn.build_library()
    return _lib_bbn.lib()


def desc(kind="Bottleneck", inplanes=16, blocks=(1, 1, 1, 1), stride=(1, 2, 2, 2), stride_conv=None, after_pool=0, block=None):
    d = _lib_bbn.BbnDesc()
    d.block = block if block is not None else _lib_bbn.PT_BBN_BOTTLENECK if kind == "Bottleneck" else _lib_bbn.PT_BBN_BASIC
    d.inplanes, d.blocks[:], d.stride[:] = inplanes, list(blocks), list(stride)
    d.stride_conv = (2 if kind == "Bottleneck" else 1) if stride_conv is None else stride_conv
    d.conv1_after_pool = after_pool
    return d


def units(g, o):
    """the bound's unit of output `o` of a golden: max(the reference's own fp32 error, one fp32 ulp of the map's range)"""
    return max(float(g[o + "_ref_err"]), f64_bound.ULP * float(g[o + "_max"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_restatement_equals_the_reference_golden(name):
    c, g = C.CASES[name], C.golden(name)
    out = RN.restate(c["spec"], C.params(name), C.image(name), c["outputs"])
    assert list(out) == [o for o in C.ALL if o in c["outputs"]]
    for o, v in out.items():
        v = v.numpy()
        assert v.dtype == np.float64 and tuple(v.shape) == tuple(g[o + "_shape"])
        assert np.abs(C.at_subset(name, o, v) - g[o + "_f64"]).max() <= 1e-12 * float(g[o + "_max"]), (name, o)
        assert abs(v.sum() - float(g[o + "_sum"])) <= 1e-12 * float(g[o + "_abssum"]) and abs(np.abs(v).sum() - float(g[o + "_abssum"])) <= 1e-12 * float(g[o + "_abssum"])
        assert 1e-2 <= float(g[o + "_max"]) <= 1e2


@pytest.mark.parametrize("defect", RN.DEFECTS)
def test_seeded_defects_miss_the_bound(defect):
    """each defect of the restatement is further than F_MAX x the unit from the golden on at least one output of one small case (a map of
    another shape misses it outright)"""
    worst = 0.0
    for name in C.SMALL[:11]:
        c, g = C.CASES[name], C.golden(name)
        for o, v in RN.restate(c["spec"], C.params(name), C.image(name), c["outputs"], defect=defect).items():
            if tuple(v.shape) != tuple(g[o + "_shape"]):
                return
            worst = max(worst, float(np.abs(C.at_subset(name, o, v.numpy()) - g[o + "_f64"]).max()) / units(g, o))
    print(f"\n{defect}: {worst:.1f} x the unit")
    assert worst > F_MAX, (defect, worst)


def test_f_max_is_a_legal_cap():
    assert f64_bound.raised_factor(0.0, F_MAX) == f64_bound.FACTOR and f64_bound.raised_factor(F_MAX / 2, F_MAX) == F_MAX


@f64_bound.needs_bundle
def test_standin_and_key_list_equal_the_reference_classes():
    from oracle import ref_harness
    ref_harness.install()
    from ltr.models.backbone import resnet, resnet_mrcnn
    for name in ("bott_odd_n2", "basic_tiny", "mrcnn_tiny", "r50_288", "r18_288"):
        c = C.CASES[name]
        spec = c["spec"]
        mod = resnet_mrcnn if spec["mrcnn"] else resnet
        ref = mod.ResNet(getattr(mod, spec["kind"]), spec["blocks"], c["outputs"], inplanes=spec["inplanes"]).state_dict()
        want = [(k, tuple(v.shape)) for k, v in ref.items()]
        assert [(k, tuple(s)) for k, s, _ in RN.keys(spec)] == want, name
        assert [(k, tuple(v.shape)) for k, v in RN.ResNet(spec, c["outputs"]).state_dict().items()] == want, name
        assert list(C.params(name)) == [k for k, _ in want]
        # what describe() reads off the reference object is what it reads off the stand-in
        a, b = B.describe(mod.ResNet(getattr(mod, spec["kind"]), spec["blocks"], c["outputs"], inplanes=spec["inplanes"])), B.describe(RN.ResNet(spec, c["outputs"]))
        assert a is not None and bytes(a.desc) == bytes(b.desc) and len(a.layers) == len(b.layers)
        assert a.desc.conv1_after_pool == int(spec["mrcnn"]) and a.desc.stride_conv == (1 if spec["mrcnn"] or spec["kind"] == "BasicBlock" else 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# plan
# ---------------------------------------------------------------------------------------------------------------------------------
def routes_of(L, d, n, H, W, mask, rows):
    count = L.pt_bbn_plan(ctypes.byref(d), n, H, W, mask, rows)
    assert count > 0, (n, H, W, mask, count)
    return {r.route for r in rows[:count]}


def test_every_route_of_the_plan_is_reached_by_a_case(L):
    rows = (_lib_bbn.BbnLaunch * _lib_bbn.PT_BBN_MAX_LAUNCHES)()
    table = {}
    for name, c in C.CASES.items():
        for r in B.plan(RN.ResNet(c["spec"], c["outputs"]).eval(), c["shape"]):
            table.setdefault(r.route, name)
    swept = set()
    for kind, blocks in (("Bottleneck", (3, 4, 6, 3)), ("BasicBlock", (2, 2, 2, 2))):
        for inplanes in (8, 16, 24, 64):
            d = desc(kind, inplanes, blocks)
            for n in range(1, 33):
                for size in list(range(16, 833, 24)) + [832]:
                    if L.pt_bbn_ws_bytes(ctypes.byref(d), n, size, size, 0b11111) == 0:
                        continue                                       # beyond the addressing limit: refused, no route
                    swept |= routes_of(L, d, n, size, size, 0b11111, rows)
            swept |= routes_of(L, d, 1, 480, 832, 0b01111, rows) | routes_of(L, d, 1, 384, 576, 0b01111, rows)
    assert swept == set(range(_lib_bbn.PT_BBN_R_COUNT)), sorted(swept)
    assert swept <= set(table), [_lib_bbn.ROUTES[r] for r in sorted(swept - set(table))]
    print("\n" + "  ".join(f"{_lib_bbn.ROUTES[r]}: {table[r]}" for r in sorted(table)))


def test_plan_rows_of_the_table(L):
    """launch order, early return and map sizes as the case table states them"""
    rows = {name: B.plan(RN.ResNet(c["spec"], c["outputs"]).eval(), c["shape"]) for name, c in C.CASES.items()}
    K = _lib_bbn
    assert [(r.kernel, r.out) for r in rows["conv1_only"]] == [(K.PT_BBN_K_STEM, K.PT_BBN_OUT_CONV1)]
    assert [(r.kernel, r.out) for r in rows["conv1_only_mrcnn"]] == [(K.PT_BBN_K_STEM, -1), (K.PT_BBN_K_POOL, K.PT_BBN_OUT_CONV1)]
    assert max(r.layer for r in rows["bott_c64_l23"]) == 3 and sorted(r.out for r in rows["bott_c64_l23"] if r.out >= 0) == [2, 3]
    last = {r.layer: (r.Hout, r.Wout) for r in rows["bott_odd_n2"]}
    assert last == {0: (9, 12), 1: (9, 12), 2: (5, 6), 3: (3, 3), 4: (2, 2)} and (rows["bott_odd_n2"][0].Hout, rows["bott_odd_n2"][0].Wout) == (17, 24)
    assert {(r.Hin, r.Hout, r.Wout, r.ksize) for r in rows["bott_n5_to_1x1"] if (r.layer, r.block, r.conv) == (4, 1, 2)} == {(1, 1, 1, 3)}
    # resnet.py puts the stride on the 3x3, resnet_mrcnn.py on the first 1x1
    first = lambda name, cv: next(r for r in rows[name] if (r.layer, r.block, r.conv) == (2, 0, cv) and r.kernel == K.PT_BBN_K_CONV)
    assert (first("bott_odd_n2", 1).stride, first("bott_odd_n2", 2).stride) == (1, 2) and (first("mrcnn_tiny", 1).stride, first("mrcnn_tiny", 2).stride) == (2, 1)
    for name, rs in rows.items():
        for i, r in enumerate(rs):
            assert r.grid_x >= 1 and r.grid_y >= 1 and r.grid_z == (1 if r.kernel == K.PT_BBN_K_REDUCE else max(r.split, 1)), (name, i)
            if r.kernel in (K.PT_BBN_K_CONV, K.PT_BBN_K_STEM):
                assert r.grid_x == -(-r.M // r.bm) and r.grid_y == -(-r.N // 64) and r.ksteps * r.split >= -(-r.K // 32), (name, i)
                if r.split > 1:                                        # its reduction follows, and owns the epilogue and the output
                    q = rs[i + 1]
                    assert q.kernel == K.PT_BBN_K_REDUCE and (q.M, q.N, q.split) == (r.M, r.N, r.split) and (r.relu, r.residual, r.out) == (0, 0, -1)
                    assert r.ksteps >= K.PT_BBN_MIN_KSTEPS and r.grid_x * r.grid_y * r.split <= K.PT_BBN_FILL_WGS
    # the deployed single frame: what DESIGN.md states of the plan at 72x72, 36x36 and 18x18
    r50 = {(r.layer, r.block, r.conv): (K.ROUTES[r.route], r.grid_x * r.grid_y * r.grid_z) for r in rows["r50_288"] if r.kernel == K.PT_BBN_K_CONV}
    assert r50[(1, 1, 1)] == ("T32", 162) and r50[(1, 1, 2)] == ("T32", 162) and r50[(1, 1, 3)] == ("T64", 324)
    assert r50[(2, 1, 1)] == ("T32_S2", 164) and r50[(2, 1, 2)] == ("T32_S2", 164) and r50[(2, 1, 3)] == ("T32", 328)
    assert r50[(3, 1, 1)] == ("T32_S4", 176) and r50[(3, 1, 2)] == ("T32_S4", 176) and r50[(3, 1, 3)] == ("T32", 176)


# ---------------------------------------------------------------------------------------------------------------------------------
# header, bindings, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_do_not_launch(L):
    K, n, p = _lib_bbn, None, ctypes.c_void_p(1 << 20)
    ok = desc()
    outs = (ctypes.c_void_p * 5)(*[1 << 24] * 5)
    ws_bytes = L.pt_bbn_ws_bytes(ctypes.byref(ok), 1, 32, 32, 31)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    fwd = lambda d=ok, pack=p, x=p, nn=1, H=32, W=32, mask=31, o=outs, ws=p, wb=ws_bytes: L.pt_bbn_forward_f32(
        ctypes.byref(d) if d is not None else None, pack, x, nn, H, W, mask, o, ws, wb, n)
    assert fwd(d=None) == fwd(pack=n) == fwd(x=n) == fwd(o=n) == fwd(ws=n) == K.PT_BBN_ERR_NULL
    assert fwd(o=(ctypes.c_void_p * 5)(1 << 24, None, 1 << 24, 1 << 24, 1 << 24)) == K.PT_BBN_ERR_NULL
    assert fwd(nn=0) == fwd(H=0) == fwd(W=-1) == fwd(mask=0) == fwd(mask=32) == K.PT_BBN_ERR_SHAPE
    assert fwd(wb=ws_bytes - 1) == fwd(ws=ctypes.c_void_p((1 << 20) + 128)) == fwd(pack=ctypes.c_void_p((1 << 20) + 4)) == K.PT_BBN_ERR_WORKSPACE
    rows = (K.BbnLaunch * K.PT_BBN_MAX_LAUNCHES)()
    for what, bad in C_REFUSALS:
        d = desc(**bad)
        assert fwd(d=d) == K.PT_BBN_ERR_UNSUPPORTED, what
        assert L.pt_bbn_pack_floats(ctypes.byref(d)) == 0 and L.pt_bbn_ws_bytes(ctypes.byref(d), 1, 32, 32, 31) == 0, what
        assert L.pt_bbn_plan(ctypes.byref(d), 1, 32, 32, 31, rows) == K.PT_BBN_ERR_UNSUPPORTED, what
    # views beyond the 32-bit byte offsets of the kernels: the input, an activation
    assert fwd(nn=64, H=2048, W=2048) == K.PT_BBN_ERR_UNSUPPORTED and L.pt_bbn_ws_bytes(ctypes.byref(ok), 64, 2048, 2048, 31) == 0
    big = desc(inplanes=256)
    assert L.pt_bbn_ws_bytes(ctypes.byref(big), 1, 832, 832, 31) > 0 and L.pt_bbn_ws_bytes(ctypes.byref(big), 16, 832, 832, 31) == 0
    assert L.pt_bbn_plan(n, 1, 32, 32, 31, rows) == K.PT_BBN_ERR_NULL and L.pt_bbn_pack_floats(n) == 0 and L.pt_bbn_ws_bytes(n, 1, 32, 32, 31) == 0
    assert L.pt_bbn_plan(ctypes.byref(ok), 1, 32, 32, 31, n) == 23                # rows may be NULL: the count alone
    assert b"NULL" in L.pt_bbn_strerror(K.PT_BBN_ERR_NULL) and b"limits" in L.pt_bbn_strerror(K.PT_BBN_ERR_UNSUPPORTED) and L.pt_bbn_abi_version() == 1


C_REFUSALS = (("inplanes not a multiple of 8", dict(inplanes=12)), ("inplanes 0", dict(inplanes=0)), ("inplanes above the limit", dict(inplanes=264)),
              ("a layer without blocks", dict(blocks=(1, 0, 1, 1))), ("too many blocks", dict(blocks=(1, 1, 49, 1))), ("stride 3", dict(stride=(1, 2, 3, 2))),
              ("stride 0", dict(stride=(0, 2, 2, 2))), ("unknown block kind", dict(block=2)), ("the stride on a third convolution", dict(stride_conv=3)),
              ("basic block with the stride on conv2", dict(kind="BasicBlock", stride_conv=2)), ("conv1 tap flag", dict(after_pool=2)))


def test_pack_floats_is_the_parameter_count_plus_the_stem_padding(L):
    for name in ("bott_odd_n2", "basic_tiny", "mrcnn_tiny", "r50_288"):
        spec = C.CASES[name]["spec"]
        convs = [(k, s) for k, s, role in RN.keys(spec) if isinstance(role, tuple)]
        want = sum(int(np.prod(s)) + 2 * s[0] for _, s in convs) + spec["inplanes"] * (_lib_bbn.PT_BBN_STEM_K - 147)
        m = RN.ResNet(spec, ["layer3"]).eval()
        assert L.pt_bbn_pack_floats(ctypes.byref(B.describe(m).desc)) == want
        pack = B.pack_weights(m)
        assert pack.numel() == want and pack.dtype == torch.float32
        # the first convolution behind the stem: tap-major weights, then the float64 fold rounded once
        c0, blk = spec["inplanes"], m.layer1[0]
        at = c0 * _lib_bbn.PT_BBN_STEM_K + 2 * c0
        w = blk.conv1.weight.detach()
        assert torch.equal(pack[at:at + w.numel()], w.permute(0, 2, 3, 1).reshape(-1))
        s = (blk.bn1.weight.detach().double() / torch.sqrt(blk.bn1.running_var.double() + blk.bn1.eps)).float()
        assert torch.equal(pack[at + w.numel():at + w.numel() + s.numel()], s)


def test_module_side_refusals_and_the_request():
    spec = C.CASES["bott_tiny"]["spec"]
    x = torch.zeros(1, 3, 32, 32)
    good = RN.standin(spec, C.params("bott_tiny"), ["layer2", "layer3"])
    with torch.no_grad():
        assert B.why_not(good, x) == "CPU input" and not B.covered(good, x)
        assert B.why_not(good, x, ["fc"]) == B.why_not(good, x, ["default"]) == B.why_not(good, x, ["layer5"]) == B.why_not(good, x, []) == "outputs outside conv1 / layer1..4"
        assert B.why_not(good, x.double()) == "CPU input" and B.why_not(good, torch.zeros(1, 1, 32, 32)) == "input that is not (n, 3, H, W)"
        assert B._mask(good, None) == 0b01100 and B._mask(good, ["conv1", "layer4"]) == 0b10001
        good.train()
        assert B.why_not(good, x) == "training mode"
        good.eval()
    assert B.why_not(good, x) == "gradients enabled"
    with pytest.raises(RuntimeError, match="MI355X only"):
        B.forward(good, x)
    structure = "structure outside ltr's ResNet at dilation 1 with BatchNorm everywhere"

    def broken(change):
        m = RN.standin(spec, C.params("bott_tiny"), ["layer3"])
        change(m)
        with torch.no_grad():
            return B.why_not(m, x)
    dilated = torch.nn.Conv2d(64, 64, 3, stride=1, padding=2, dilation=2, bias=False)
    assert broken(lambda m: setattr(m.layer3[0], "conv2", dilated)) == structure                      # dilation_factor != 1
    assert broken(lambda m: setattr(m.layer2[0], "bn2", torch.nn.Identity())) == structure
    assert broken(lambda m: setattr(m.layer2[0], "downsample", None)) == structure
    assert broken(lambda m: setattr(m, "maxpool", torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True))) == structure
    assert broken(lambda m: setattr(m, "conv1", torch.nn.Conv2d(3, 16, 7, stride=2, padding=3, bias=True))) == structure
    with torch.no_grad():
        assert B.why_not(RN.standin(C.CASES["basic_tiny"]["spec"], C.params("basic_tiny"), ["layer3"]), x) == "CPU input"

    def without_bn(m):                                                                                # BasicBlock(use_bn=False)
        m.layer1[1].use_bn = False
        del m.layer1[1].bn1, m.layer1[1].bn2
    basic = RN.ResNet(C.CASES["basic_tiny"]["spec"], ["layer3"]).eval()
    without_bn(basic)
    with torch.no_grad():
        assert B.why_not(basic, x) == structure
        # the structure is remembered per module tree: a replaced submodule is seen, an attribute rewritten in place needs refresh()
        seen = RN.standin(spec, C.params("bott_tiny"), ["layer3"])
        assert B.why_not(seen, x) == "CPU input"
        seen.layer3[0].conv2 = dilated
        assert B.why_not(seen, x) == structure


def _defined(path):
    llvm = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "llvm", "bin")
    nm = os.path.join(llvm, "llvm-nm")
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    else:                                                                     # llvm-readelf's --dyn-syms table says the same (Ndx UND = undefined)
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        defined = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    return {s for s in defined if s.startswith("pt_")}


def test_header_symbols_exported(L):
    """the dynamic symbol table of libpt_bbn.so holds exactly the functions include/pt_bbn.h declares; the other four libraries' sets are what
    their headers declare, and none of them is a pt_bbn_ name"""
    defined = _defined(_lib_bbn.LIB_PATH)
    assert defined == set(_lib_bbn.EXPORTS) and all(s.startswith("pt_bbn_") for s in defined)
    assert _lib_bbn.EXPORTS == ["pt_bbn_strerror", "pt_bbn_abi_version", "pt_bbn_pack_floats", "pt_bbn_ws_bytes", "pt_bbn_plan", "pt_bbn_forward_f32"]
    for lib, prefix, count in ((_lib_loc, "pt_loc_", 6), (_lib_mot, "pt_mot_", 6), (_lib_mem, "pt_mem_", 6)):
        lib.build_library()
        got = _defined(lib.LIB_PATH)
        assert got == set(lib.EXPORTS) and len(got) == count and all(s.startswith(prefix) for s in got)
    _lib.build_library()
    hot = _defined(_lib.LIB_PATH)
    assert hot == set(_lib.EXPORTS) and not any(s.startswith(("pt_loc_", "pt_mot_", "pt_mem_", "pt_bbn_")) for s in hot)


def test_derived_bindings_match_the_host_compiler(tmp_path):
    """sizeof / offsetof of the structs and the value of every constant of include/pt_bbn.h, printed by a C program generated from the parsed
    header, equal the ctypes classes and attributes of _lib_bbn (the check tests/test_mem_update_cpu.py makes for include/pt_mem.h)."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    with open(os.path.join(ROOT, "include", "pt_bbn.h")) as fh:
        abi = _abi.parse(fh.read())
    assert list(abi.structs) == ["pt_bbn_desc", "pt_bbn_launch"] and list(abi.functions) == _lib_bbn.EXPORTS
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "pt_bbn.h"', "int main(void) {"]
    src += [f'    printf("{k} %lld\\n", (long long){k});' for k in abi.constants]
    for cname, cls in abi.structs.items():
        src.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        src += [f'    printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(src + ["    return 0;", "}"]) + "\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, text=True)
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                                                   text=True).stdout.splitlines()}
    want = {k: [getattr(_lib_bbn, k)] for k in abi.constants}
    for cname in abi.structs:
        cls = getattr(_lib_bbn, _abi.class_name(cname))
        want[cname] = [ctypes.sizeof(cls)]
        for f, t in cls._fields_:
            want[f"{cname}.{f}"] = [getattr(cls, f).offset, ctypes.sizeof(t)]
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    c = ctypes
    restype, args = abi.functions["pt_bbn_forward_f32"]
    assert restype is c.c_int and [t.__name__ for t in args] == ["LP_BbnDesc", "c_void_p", "c_void_p", "c_int", "c_int", "c_int", "c_int", "c_void_p",
                                                                 "c_void_p", c.c_size_t.__name__, "c_void_p"]
    assert abi.functions["pt_bbn_pack_floats"][0] is c.c_size_t and abi.functions["pt_bbn_strerror"] == (c.c_char_p, [c.c_int])
    assert _lib_bbn.OUTPUTS == RN.OUTPUTS and len(_lib_bbn.ROUTES) == _lib_bbn.PT_BBN_R_COUNT and len(_lib_bbn.KERNELS) == 4


def test_the_other_headers_declare_what_they_declared():
    """the function sets of the four pinned headers, by count and prefix: libpt_bbn adds to none of them"""
    for lib, header, count in ((_lib_loc, "pt_loc.h", 6), (_lib_mot, "pt_mot.h", 6), (_lib_mem, "pt_mem.h", 6)):
        with open(os.path.join(ROOT, "include", header)) as fh:
            assert list(_abi.parse(fh.read()).functions) == lib.EXPORTS and len(lib.EXPORTS) == count
    assert not any("bbn" in name for name in _lib.EXPORTS)


def test_install_switch_is_off_by_default_and_the_module_never_imports_the_oracle():
    from pytracking_amd import install
    assert inspect.signature(install.install).parameters["backbone"].default is False
    src = open(os.path.join(ROOT, "pytracking_amd", "backbone.py")).read()
    assert "import oracle" not in src and "from oracle" not in src


@f64_bound.needs_bundle
def test_install_round_trip_and_the_dispatcher_on_the_cpu():
    from oracle import ref_harness
    ref_harness.install()
    from ltr.models.backbone import resnet, resnet_mrcnn
    from pytracking_amd import install as amd
    amd.uninstall()
    classes = [resnet.ResNet, resnet_mrcnn.ResNet]
    refs = [vars(c)["forward"] for c in classes]
    c = C.CASES["bott_tiny"]
    net = resnet.ResNet(resnet.Bottleneck, c["spec"]["blocks"], ["layer2", "layer3"], inplanes=16)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in C.params("bott_tiny").items()}, strict=True)
    net.eval()
    x, g = torch.from_numpy(C.image("bott_tiny")), C.golden("bott_tiny")
    try:
        amd.install()
        assert [vars(k)["forward"] for k in classes] == refs                      # a default install() leaves both alone
        default_ledger = [(o, n) for o, n, _, _ in amd._state["ledger"]]
        amd.uninstall()
        amd.install(backbone=True)
        extra = [(o, n) for o, n, _, _ in amd._state["ledger"]]
        assert extra[:len(default_ledger)] == default_ledger and extra[len(default_ledger):] == [(k, "forward") for k in classes]
        for k, ref in zip(classes, refs):
            assert vars(k)["forward"].__wrapped__ is ref and amd.original(k, "forward") is ref
        amd.stats.clear()
        with torch.no_grad():
            out = net(x)                                                          # a CPU input goes to the reference method, counted
        assert amd.stats["ResNet.forward.reference"] == 1 and amd.stats["ResNet.forward.fast"] == 0
        assert list(out) == ["layer2", "layer3"]
        f64_bound.held("reference method on the CPU", out["layer3"].reshape(-1), g["layer3_f64"], float(g["layer3_ref_err"]), floor=f64_bound.ulp_of_max)
        amd.uninstall()
        amd.install(strict=True, backbone=True)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="outside the gfx950 backbone"):
            net(x)
    finally:
        amd.uninstall()
    assert [vars(k)["forward"] for k in classes] == refs
