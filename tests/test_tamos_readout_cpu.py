"""CPU side of the TaMOs per-frame multi-object read-out (no GPU here): the numpy restatement of tests/tamos_readout_np.py against the
goldens of the unmodified reference (tools/make_golden_tamos_readout.py), the coverage and the decision margins of the case table, the
seeded defects, the argument checks of libpt_mot (nothing is launched) and the derived ctypes bindings against the host C compiler.

Bounds.  The restatement's fp32 run is held to the golden -- another fp32 evaluation of the same lines -- within FACTOR x max(ref_err,
2^-23 max|want|) on each side of float64, i.e. twice the bound of tests/f64_bound.py, ref_err being the restatement's own fp32 distance from
float64.  Flags and cells are compared exactly.  MARGIN is what every discrete decision of every case keeps clear in float64: the fp32
rounding of the sigmoid and of the bicubic sum (16 taps, weights of magnitude <= 1.3, map values within [-3, 3]: below 3e-6) cannot cross
it, which is why the device test excludes nothing."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import f64_bound
import tamos_readout_cases as C
import tamos_readout_np as RN
from pytracking_amd import _abi, _lib_mot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-3
_RUNS = {}


def anchor(name):
    return f64_bound.anchor(("tamos_readout", name), lambda dt: _floats(C.run(C.CASES[name], dt)))


def _floats(out):
    return f64_bound.OrderedDict((k, out[k]) for k in RN.FLOAT_OUTPUTS)


def run64(name):
    if name not in _RUNS:
        _RUNS[name] = C.run(C.CASES[name])
    return _RUNS[name]


@pytest.fixture(scope="module")
def L():
    _lib_mot.build_library()
    return _lib_mot.lib()


@pytest.mark.parametrize("name", C.CASES)
def test_restatement_equals_the_reference_golden(name):
    g, a, w = C.golden(name), anchor(name), run64(name)
    f32 = C.run(C.CASES[name], np.float32)
    assert np.array_equal(g["flag"], w["flag"]) and np.array_equal(g["cell"], w["cell"])
    assert np.array_equal(f32["flag"], w["flag"]) and np.array_equal(f32["cell"], w["cell"])
    for k in ("map", "max1", "raw_box", "box"):
        unit = max(a.ref_errs[k], f64_bound.ulp_of_max(a.want[k]))
        err = float(np.abs(g[k].astype(np.float64) - f32[k].astype(np.float64)).max())
        print(f"{name} {k}: max |fp32 restatement - golden| = {err:.3e} ({err / unit:.2f} x max(ref_err {a.ref_errs[k]:.3e}, ulp of max))")
        assert err <= 2 * f64_bound.FACTOR * unit, (name, k, err, unit)
    if not C.CASES[name]["frame"]["normalize_scores"] and C.CASES[name]["scores"].shape[-2:] == (C.CASES[name]["H"], C.CASES[name]["W"]):
        assert np.array_equal(g["map"], f32["map"])                           # used as it is: the raw map, bit for bit


def test_targets_restatement_equals_the_reference_golden():
    g = C.golden("targets")
    for nf in (1, 2):
        b = C.target_boxes(nf)
        w64, w32 = RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE), RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE, np.float32)
        assert w32.shape == g[f"ltrb_nf{nf}"].shape == (nf, b.shape[1], 4, 12, 18)
        assert np.array_equal(w32, g[f"ltrb_nf{nf}"])                         # a difference, a sum and a quotient of fp32 numbers: bit for bit
        assert (w64[:, 1] == 0).all() and (w64[-1, -1] == 0).all() and (w64[:, 0] != 0).any()      # the empty boxes
    lab = C.LABEL
    w64 = RN.label(C.LABEL_CENTRES, lab["feature_sz"], lab["sigma"], lab["end_pad"])
    w32 = RN.label(C.LABEL_CENTRES, lab["feature_sz"], lab["sigma"], lab["end_pad"], np.float32)
    unit = max(float(np.abs(w32 - w64).max()), f64_bound.ulp_of_max(w64))
    err = float(np.abs(g["label"].astype(np.float64) - w32).max())
    print(f"label: max |fp32 restatement - golden| = {err:.3e} ({err / unit:.2f} x unit)")
    assert g["label"].shape == w64.shape == (4, 12, 18) and err <= 2 * f64_bound.FACTOR * unit
    assert w64[3].max() < 1e-30                                               # the centre far off the map
    # get_label_function from a position: the centre in the reference's fp32 order, then the same label
    fr = C.CASES["up6x9_wide"]["frame"]
    centre = RN.label_centre(g["pos"], fr, lab["feature_sz"])
    got = RN.label(centre[None], lab["feature_sz"], lab["sigma"], lab["end_pad"], np.float32)[0]
    assert np.abs(got - g["label_from_pos"]).max() <= 2 * f64_bound.FACTOR * f64_bound.ULP


def test_table_reaches_every_statement_peak_and_clip():
    reached = set()
    for name in C.CASES:
        w = run64(name)
        assert w["statement"].tolist() == C.STATEMENTS[name], (name, w["statement"].tolist())
        reached |= set(w["statement"].tolist())
    assert reached == set(range(1, 10))                                       # the nine return statements of tamos.py:386-429
    assert {len(c["active"]) for c in C.CASES.values()} >= {1, 2, 4, 9} and max(c["T"] for c in C.CASES.values()) == 16
    wide = C.CASES["up6x9_wide"]
    assert wide["active"] != list(range(len(wide["active"]))) and 15 in wide["active"]          # gaps in the active ids
    assert C.CASES["up6x9_wide"]["frame"]["scale_factor"] == 144 / 400 and C.CASES["up6x9_tall"]["frame"]["scale_factor"] == 96 / 192   # both aspect branches
    # peaks: a corner, the four borders, a tie that row-major order would decide the other way
    a5, clipc = run64("asis5x7"), run64("asis12x18_clip")
    assert a5["peak1"][0].tolist() == [0, 0]
    s = C.CASES["asis5x7"]["scores"][1]
    assert s[2, 5] == s[4, 1] == s.max() and a5["peak1"][1].tolist() == [4, 1] and a5["peak2"][1].tolist() == [2, 5]
    assert clipc["peak1"][:3].tolist() == [[0, 8], [6, 0], [4, 17]] and run64("up6x9_tall")["peak1"][0].tolist() == [11, 9]
    # a neighbourhood bound exactly on .5, decided by round-half-to-even
    tall = C.CASES["up6x9_tall"]
    cst = RN.constants(tall["frame"], tall["objects"][0], 12, 18)
    assert cst["neigh"].tolist() == [3.0, 3.0] and run64("up6x9_tall")["mask"][0].tolist() == [10, 12, 8, 12]
    assert clipc["mask"][2].tolist()[:2] == [2, 6]                             # round(2.5) = 2, round(6.5) = 6
    # clipping: left and top, right and bottom, the minimum size
    raw, box = clipc["raw_box"], clipc["box"]
    fr = C.CASES["asis12x18_clip"]["frame"]
    assert raw[0, 0] < 0 and raw[0, 1] < 0 and box[0, :2].tolist() == [0, 0]
    assert raw[1, 0] + raw[1, 2] > fr["image_w"] and raw[1, 1] + raw[1, 3] > fr["image_h"]
    assert box[1, 0] + box[1, 2] == fr["image_w"] and box[1, 1] + box[1, 3] == fr["image_h"]
    assert box[3].tolist() == [fr["image_w"] - 10, fr["image_h"] - 10, 10, 10]


@pytest.mark.parametrize("name", C.CASES)
def test_every_discrete_decision_keeps_its_margin(name):
    w = run64(name)
    for t, m in zip(C.CASES[name]["active"], w["margins"]):
        worst = min(m, key=m.get)
        print(f"{name} object {t}: smallest margin {m[worst]:.3e} ({worst})")
        assert m[worst] >= MARGIN, (name, t, worst, m[worst])
    assert float(np.abs(C.CASES[name]["scores"]).max()) <= 3.1               # the range the fp32 rounding above is worked out for


def _defect_ratio(defect):
    """the largest miss of a seeded defect over the table: inf for a discrete output that changes, else the largest ratio of a float
    output's error to max(ref_err, ulp of max) -- the unit the device is held to"""
    worst = 0.0
    for name in C.CASES:
        a, w, x = anchor(name), run64(name), C.run(C.CASES[name], defect=defect)
        if any(not np.array_equal(w[k], x[k]) for k in RN.DISCRETE_OUTPUTS):
            return float("inf")
        for k in RN.FLOAT_OUTPUTS:
            unit = max(a.ref_errs[k], f64_bound.ulp_of_max(a.want[k]))
            worst = max(worst, float(np.abs(x[k] - w[k]).max()) / unit)
    return worst


F_MAX = C.F_MAX


@pytest.mark.parametrize("defect", RN.DEFECTS)
def test_seeded_defects_miss_the_bound(defect):
    r = _defect_ratio(defect)
    print(f"defect {defect}: {r:.3g} x max(ref_err, ulp of max)")
    assert r > F_MAX >= f64_bound.FACTOR


def test_seeded_defects_of_the_targets_miss_the_bound():
    b = C.target_boxes(2)
    w, x = RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE), RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE, defect="no_half_stride")
    ref = float(np.abs(RN.encode_bbox(b, C.IMAGE_SAMPLE_SIZE, C.STRIDE, np.float32) - w).max())
    assert float(np.abs(x - w).max()) > F_MAX * max(ref, f64_bound.ulp_of_max(w))


@pytest.mark.parametrize("name", C.CASES)
def test_host_constants_equal_the_restatement_bit_for_bit(L, name):
    case = C.CASES[name]
    f = C.frame_block(case["frame"])
    for t in case["active"]:
        q = _lib_mot.MotConsts()
        assert L.pt_mot_constants_f32(ctypes.byref(f), ctypes.byref(C.object_block(case["objects"][t])), case["H"], case["W"], ctypes.byref(q)) == 0
        want = RN.constants(case["frame"], case["objects"][t], case["H"], case["W"])
        got = dict(center=list(q.center), neigh=list(q.neigh), prev=list(q.prev))
        for k, v in got.items():
            assert np.array_equal(np.asarray(v, np.float32), want[k]), (name, t, k, v, want[k])
        assert np.float32(q.disp_threshold) == want["disp_threshold"]


def test_argument_checks_do_not_launch(L):
    n, one = None, ctypes.c_void_p(256)
    M = _lib_mot
    case = C.CASES["up6x9_wide"]
    f = C.frame_block(case["frame"])
    act = (ctypes.c_int * 2)(0, 2)
    objs = (M.MotObject * 2)(C.object_block(case["objects"][0]), C.object_block(case["objects"][2]))
    ok = lambda **kw: dict(dict(scores=one, Hs=6, Ws=9, ltrb=one, H=12, W=18, T=16, active=act, n=2, objs=objs, fr=ctypes.byref(f), map_out=n, rec=one, seq=1.0), **kw)
    call = lambda a: L.pt_mot_readout_f32(a["scores"], a["Hs"], a["Ws"], a["ltrb"], a["H"], a["W"], a["T"], a["active"], a["n"], a["objs"], a["fr"],
                                          a["map_out"], a["rec"], a["seq"], n)
    for key in ("scores", "ltrb", "active", "objs", "fr", "rec"):
        assert call(ok(**{key: n})) == M.PT_MOT_ERR_NULL, key
    assert call(ok(Hs=0)) == M.PT_MOT_ERR_SHAPE and call(ok(W=-1)) == M.PT_MOT_ERR_SHAPE
    assert call(ok(Hs=12)) == M.PT_MOT_ERR_SHAPE                               # one size equal, one different
    assert call(ok(H=24, W=36, Hs=12, Ws=18)) == M.PT_MOT_ERR_SHAPE            # not the location grid of the stride
    assert call(ok(active=(ctypes.c_int * 2)(0, 16))) == M.PT_MOT_ERR_SHAPE and call(ok(active=(ctypes.c_int * 2)(3, 3))) == M.PT_MOT_ERR_SHAPE
    assert call(ok(n=0)) == M.PT_MOT_ERR_UNSUPPORTED and call(ok(T=1)) == M.PT_MOT_ERR_UNSUPPORTED        # more active objects than objects
    # every refusal of the table
    for what, over, T, (Hs, Ws, H, W) in C.REFUSALS:
        fr = dict(case["frame"], **over)
        fr.update(img_sample_sz=(float(H * 8), float(W * 8)))
        fb = C.frame_block(fr)
        assert call(ok(fr=ctypes.byref(fb), T=T, n=1, Hs=Hs, Ws=Ws, H=H, W=W)) == M.PT_MOT_ERR_UNSUPPORTED, what
    q = M.MotConsts()
    even = C.frame_block(dict(case["frame"], kernel_size=(2.0, 1.0)))
    assert L.pt_mot_constants_f32(ctypes.byref(even), ctypes.byref(objs[0]), 12, 18, ctypes.byref(q)) == M.PT_MOT_ERR_UNSUPPORTED
    assert L.pt_mot_constants_f32(n, ctypes.byref(objs[0]), 12, 18, ctypes.byref(q)) == M.PT_MOT_ERR_NULL
    assert L.pt_mot_constants_f32(ctypes.byref(f), ctypes.byref(objs[0]), 0, 18, ctypes.byref(q)) == M.PT_MOT_ERR_SHAPE
    # the wait and the targets
    assert L.pt_mot_wait_f32(n, act, 2, 1.0, n) == M.PT_MOT_ERR_NULL and L.pt_mot_wait_f32(one, act, 0, 1.0, n) == M.PT_MOT_ERR_SHAPE
    lab = M.MotLabel()
    lab.sz[:], lab.sigma[:], lab.end_pad[:] = (12.0, 18.0), (0.9, 0.9), (0.0, 0.0)
    c2 = (ctypes.c_float * 2)(0.0, 0.0)
    tg = L.pt_mot_targets_f32
    assert tg(n, 0, 96, 144, 8, n, n, n, 0, n, n) == M.PT_MOT_ERR_SHAPE        # neither part
    assert tg(n, 3, 96, 144, 8, one, n, n, 0, n, n) == M.PT_MOT_ERR_NULL and tg(one, 3, 96, 144, 8, n, n, n, 0, n, n) == M.PT_MOT_ERR_NULL
    assert tg(one, 3, 96, 144, 0, one, n, n, 0, n, n) == M.PT_MOT_ERR_SHAPE and tg(one, 3, 100, 144, 8, one, n, n, 0, n, n) == M.PT_MOT_ERR_UNSUPPORTED
    assert tg(n, 0, 0, 0, 0, n, ctypes.byref(lab), c2, 1, n, n) == M.PT_MOT_ERR_NULL and tg(n, 0, 0, 0, 0, n, n, c2, 1, one, n) == M.PT_MOT_ERR_NULL
    assert tg(n, 0, 0, 0, 0, n, ctypes.byref(lab), c2, M.PT_MOT_MAX_CENTRES + 1, one, n) == M.PT_MOT_ERR_UNSUPPORTED
    lab.sigma[0] = 0.0
    assert tg(n, 0, 0, 0, 0, n, ctypes.byref(lab), c2, 1, one, n) == M.PT_MOT_ERR_SHAPE
    assert b"NULL" in L.pt_mot_strerror(M.PT_MOT_ERR_NULL) and b"not covered" in L.pt_mot_strerror(M.PT_MOT_ERR_UNSUPPORTED)
    assert L.pt_mot_abi_version() == 1


def test_header_symbols_exported(L):
    """the dynamic symbol table of libpt_mot.so holds exactly the functions include/pt_mot.h declares, and libpt_hot's set is untouched"""
    llvm = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "llvm", "bin")
    nm = os.path.join(llvm, "llvm-nm")
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib_mot.LIB_PATH], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    else:                                                                     # llvm-readelf's --dyn-syms table says the same (Ndx UND = undefined)
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--dyn-syms", "-W", _lib_mot.LIB_PATH], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        defined = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    defined = {s for s in defined if s.startswith("pt_")}
    assert defined == set(_lib_mot.EXPORTS) and len(defined) == 6 and all(s.startswith("pt_mot_") for s in defined)


def test_derived_bindings_match_the_host_compiler(tmp_path):
    """sizeof / offsetof of the structs and the value of every constant of include/pt_mot.h, printed by a C program generated from the parsed
    header, equal the ctypes classes and attributes of _lib_mot (the check tests/test_abi_cpu.py makes for include/pt_hot.h)."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    with open(os.path.join(ROOT, "include", "pt_mot.h")) as fh:
        abi = _abi.parse(fh.read())
    assert list(abi.structs) == ["pt_mot_frame", "pt_mot_object", "pt_mot_consts", "pt_mot_label"] and list(abi.functions) == _lib_mot.EXPORTS
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "pt_mot.h"', "int main(void) {"]
    src += [f'    printf("{k} %lld\\n", (long long){k});' for k in abi.constants]
    for cname, cls in abi.structs.items():
        src.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        src += [f'    printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(src + ["    return 0;", "}"]) + "\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, text=True)
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                                                   text=True).stdout.splitlines()}
    want = {k: [getattr(_lib_mot, k)] for k in abi.constants}
    for cname in abi.structs:
        cls = getattr(_lib_mot, _abi.class_name(cname))
        want[cname] = [ctypes.sizeof(cls)]
        for f, t in cls._fields_:
            want[f"{cname}.{f}"] = [getattr(cls, f).offset, ctypes.sizeof(t)]
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    # prototypes: restype and argument count / kinds of the entry points
    c = ctypes
    restype, args = abi.functions["pt_mot_readout_f32"]
    assert restype is c.c_int and [t.__name__ for t in args] == ["c_void_p", "c_int", "c_int", "c_void_p", "c_int", "c_int", "c_int", "c_void_p", "c_int",
                                                                 "LP_MotObject", "LP_MotFrame", "c_void_p", "c_void_p", "c_float", "c_void_p"]
    assert abi.functions["pt_mot_strerror"] == (c.c_char_p, [c.c_int]) and abi.functions["pt_mot_abi_version"] == (c.c_int, [])
    L = _lib_mot.lib() if os.path.exists(_lib_mot.LIB_PATH) else None
    if L is not None:                                                     # what the loaded functions carry
        assert L.pt_mot_readout_f32.restype is c.c_int and len(L.pt_mot_readout_f32.argtypes) == 15


def test_install_switch_is_off_by_default_and_the_module_never_imports_the_oracle():
    import inspect
    from pytracking_amd import install
    assert inspect.signature(install.install).parameters["tamos_readout"].default is False
    src = open(os.path.join(ROOT, "pytracking_amd", "tamos_readout.py")).read()
    assert "import oracle" not in src and "from oracle" not in src
