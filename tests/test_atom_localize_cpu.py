"""CPU side of ATOM's per-frame score localisation (no GPU here): the float64 numpy restatement of tests/atom_localize_np.py against the
goldens of the unmodified reference (tools/make_golden_atom_localize.py), the coverage and the decision margins of the case table, the
seeded defects, the argument checks of libpt_loc (nothing is launched), the symbol tables of the three libraries, the derived ctypes bindings
against the host C compiler and the install switch.

Bounds.  The restatement's float64 run is held to the reference's float64 run within FACTOR x max(ref_fp32_err, 2^-23 max|want|): the
reference's "float64" run still forms its phase factors in float32 (fourier.py:67-68 asks for float32 frequency coordinates), so it sits at
the scale of the fp32 run's own error from the restatement, not at float64 resolution.  Where the golden keeps only the fp32 map (the
deployed case) the fp32 run is held with twice that bound.  Flags, scales and cells are compared exactly."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import atom_localize_cases as C
import atom_localize_np as RN
import f64_bound
from pytracking_amd import _abi, _lib, _lib_loc, _lib_mot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_FACTOR = 16


@pytest.fixture(scope="module")
def L():
    _lib_loc.build_library()
    return _lib_loc.lib()


def unit(name, k, want):
    return max(C.ref_errs(name)[k], f64_bound.ulp_of_max(want))


@pytest.mark.parametrize("name", C.CASES)
def test_restatement_equals_the_reference_golden(name):
    g, w = C.golden(name), C.run(name)
    si = w["scale_ind"]
    assert int(g["flag"]) == w["flag"] and int(g["scale_ind"]) == si and w["branch"] == C.BRANCHES[name]
    assert tuple(g["map_shape"]) == (len(C.CASES[name]["scores"]), 1) + C.CASES[name]["G"]
    m = w["map"][si]
    rows = [("tv", g["tv64"], w["tv"], 1), ("max1", g["max164"], m.max(), 1)]
    if "map64" in g:
        rows.append(("map", g["map64"], m, 1))
    elif "map" in g:
        rows.append(("map", g["map"].astype(np.float64), m, 2))              # the fp32 run: its own error on top
    for k, ref, got, slack in rows:
        u = unit(name, k, w[k] if k != "max1" else m.max())
        err = float(np.abs(np.asarray(ref, np.float64) - np.asarray(got, np.float64)).max())
        print(f"{name} {k}: max |restatement - reference| = {err:.3e} ({err / u if u else 0.0:.2f} x max(ref_fp32_err, ulp of max))")
        assert err <= slack * f64_bound.FACTOR * u, (name, k, err, u)
    # the fp32 run's translation vector: formed from integers in the same float32 operations
    assert np.abs(g["tv"].astype(np.float64) - w["tv"]).max() <= f64_bound.FACTOR * unit(name, "tv", w["tv"])


def test_table_reaches_every_outcome_shape_and_border():
    runs = {n: C.run(n) for n in C.CASES}
    assert {w["branch"] for w in runs.values()} == {"plain", "not_found", "normal", "hn_weak", "hn_first", "hn_second", "uncertain_far", "uncertain_near"}
    assert {len(c["scores"]) for c in C.CASES.values()} == {1, 2, 3, 8}
    shapes = {(c["N"], c["G"], c["kernel"]) for c in C.CASES.values()}
    assert {((4, 4), (9, 9), (4, 4)), ((6, 7), (24, 28), (4, 4)), ((5, 6), (40, 24), (3, 3)), ((8, 8), (32, 48), (4, 3)), ((18, 18), (288, 288), (4, 4)),
            ((18, 18), (576, 576), (4, 4))} == shapes
    modes = {(c["window"] is not None, c["hn_without_windowing"], c["advanced"]) for c in C.CASES.values()}
    assert {(False, False, True), (True, False, True), (True, True, True), (False, False, False), (True, False, False)} <= modes
    # the chosen scale is not always the first, and the second peak of a hard negative can be the answer
    assert {w["scale_ind"] for w in runs.values()} >= {0, 1, 2, 3, 5}
    # the neighbourhood clipped at each border
    br, tl = runs["b_hn_second_clip_br"], runs["b_uncertain_far_clip_tl"]
    assert br["mask"][1] == 32 and br["mask"][3] == 48 and br["peak1"][0] + C.RN.constants(C.CASES["b_hn_second_clip_br"])["neigh"][0] / 2 + 1 > 32
    assert tl["mask"][0] == 0 and tl["mask"][2] == 0 and tl["peak1"][0] - C.RN.constants(C.CASES["b_uncertain_far_clip_tl"])["neigh"][0] / 2 < 0
    # a bound on a half-integer that half-to-even and half-away rounding decide differently
    he, case = runs["b_half_even"], C.CASES["b_half_even"]
    nr = float(RN.constants(case)["neigh"][0])
    assert nr == 7.0 and he["peak1"][0] % 2 == 0 and he["mask"][:2] == (he["peak1"][0] - 4, he["peak1"][0] + 4)
    assert RN.localize(case, "half_away")["mask"][:2] == (he["peak1"][0] - 3, he["peak1"][0] + 5)
    # ATOM's mask is zero: on a map that is negative outside the neighbourhood the second peak is the mask's first zero
    mz = runs["b_mask_zero"]
    assert mz["max2"] == 0.0 and tuple(mz["peak2"]) == (mz["mask"][0], mz["mask"][2])
    # the one-hot quirk: 18 x 18, 4 x 4 kernel, 288 x 288 grid: (19 / 18)^2 at cell 16 (n + 9) mod 288
    hot = np.zeros((1, 1, 18, 18), np.float32)
    hot[0, 0, 5, 11] = 1
    up = RN.upsample(dict(C.CASES["deployed"], scores=hot))[0]
    assert np.unravel_index(up.argmax(), up.shape) == (16 * 14, (16 * 20) % 288) and abs(up.max() - (19 / 18) ** 2) < 1e-12


@pytest.mark.parametrize("name", C.CASES)
def test_every_discrete_decision_keeps_its_margin(name):
    w = C.run(name)
    need = MARGIN_FACTOR * max(f64_bound.bound(C.ref_errs(name)[k], f64_bound.FACTOR, f64_bound.ulp_of_max(w["map"])) for k in ("map", "max1", "max2"))
    m = w["margins"]
    worst = min(m, key=m.get)
    print(f"{name}: smallest margin {m[worst]:.3e} ({worst}), needed {need:.3e}; all {dict((k, float(f'{v:.3g}')) for k, v in m.items())}")
    assert m[worst] >= need, (name, worst, m[worst], need)
    on_half = C.CASES[name]["on_half"]
    assert all("round_" + k not in m for k in on_half) and (not on_half or name == "b_half_even")


def _defect_ratio(defect):
    """the largest miss of a seeded defect over the table: inf for a discrete output that changes, else the largest ratio of a float
    output's error to max(ref_err, ulp of max) -- the unit the device is held to"""
    worst = 0.0
    for name in C.CASES:
        w, x = C.run(name), C.run(name, defect)
        if any(not np.array_equal(np.asarray(w[k]), np.asarray(x[k])) for k in RN.DISCRETE_OUTPUTS):
            return float("inf")
        for k in RN.FLOAT_OUTPUTS:
            err, u = float(np.abs(np.asarray(x[k]) - np.asarray(w[k])).max()), unit(name, k, w[k])
            worst = max(worst, err / u if u else (float("inf") if err else 0.0))
    return worst


@pytest.mark.parametrize("defect", RN.DEFECTS)
def test_seeded_defects_miss_the_bound(defect):
    r = _defect_ratio(defect)
    print(f"defect {defect}: {r:.3g} x max(ref_err, ulp of max)")
    assert r > C.F_MAX >= f64_bound.FACTOR


@pytest.mark.parametrize("name", C.CASES)
def test_host_constants_equal_the_restatement_bit_for_bit(L, name):
    case = C.CASES[name]
    q = _lib_loc.LocAtomParams()
    assert L.pt_loc_atom_constants_f32(ctypes.byref(C.state_block(case)), ctypes.byref(q)) == 0
    want = RN.constants(case)
    for k in ("ratio", "center", "half", "neigh"):
        assert np.array_equal(np.asarray(list(getattr(q, k)), np.float32), want[k]), (name, k, list(getattr(q, k)), want[k])
    assert np.float32(q.disp_threshold) == want["disp_threshold"] and np.float32(q.target_scale) == want["target_scale"]
    S = len(case["scores"])
    assert np.array_equal(np.asarray(list(q.scale_factors), np.float32)[:S], want["scale_factors"])
    assert list(q.parity) == [k % 2 for k in case["kernel"]] and q.advanced == int(case["advanced"])
    assert q.windowed == int(case["window"] is not None) and q.hn == int(case["window"] is not None and case["hn_without_windowing"])


def test_argument_checks_do_not_launch(L):
    n, one = None, ctypes.c_void_p(256)
    A = _lib_loc
    case = C.CASES["n5x6_k3_g40x24_hn"]
    q = A.LocAtomParams()
    assert L.pt_loc_atom_constants_f32(ctypes.byref(C.state_block(case)), ctypes.byref(q)) == 0
    ok = lambda **kw: dict(dict(scores=one, S=3, Nh=5, Nw=6, Gh=40, Gw=24, window=one, prm=ctypes.byref(q), map_out=one, map_hn=one, rec=one, ws=one,
                                ws_bytes=4096), **kw)
    call = lambda a: L.pt_loc_atom_f32(a["scores"], a["S"], a["Nh"], a["Nw"], a["Gh"], a["Gw"], a["window"], a["prm"], a["map_out"], a["map_hn"], a["rec"],
                                       1.0, a["ws"], a["ws_bytes"], n)
    for key in ("scores", "prm", "map_out", "rec", "ws", "window", "map_hn"):
        assert call(ok(**{key: n})) == A.PT_AL_ERR_NULL, key
    assert call(ok(Nh=0)) == A.PT_AL_ERR_SHAPE and call(ok(Gw=-1)) == A.PT_AL_ERR_SHAPE
    assert call(ok(ws_bytes=16)) == A.PT_AL_ERR_WORKSPACE and call(ok(ws=ctypes.c_void_p(264))) == A.PT_AL_ERR_WORKSPACE
    for what, Nh, Nw, Gh, Gw, S in C.REFUSALS:                                # every refusal of the table
        assert call(ok(S=S, Nh=Nh, Nw=Nw, Gh=Gh, Gw=Gw)) == A.PT_AL_ERR_UNSUPPORTED, what
        assert L.pt_loc_atom_ws_bytes(S, Nh, Nw, Gh, Gw) == 0, what
    for name, c in C.CASES.items():
        S, (Nh, Nw), (Gh, Gw) = len(c["scores"]), c["N"], c["G"]
        assert L.pt_loc_atom_ws_bytes(S, Nh, Nw, Gh, Gw) == (S * -(-Gh // A.PT_AL_BAND_ROWS) * 16 + 255) // 256 * 256, name
    plain = A.LocAtomParams()
    st = C.state_block(C.CASES["n4_g9"])
    assert L.pt_loc_atom_constants_f32(n, ctypes.byref(plain)) == A.PT_AL_ERR_NULL and L.pt_loc_atom_constants_f32(ctypes.byref(st), n) == A.PT_AL_ERR_NULL
    st.output_sz[0] = 0.0
    assert L.pt_loc_atom_constants_f32(ctypes.byref(st), ctypes.byref(plain)) == A.PT_AL_ERR_SHAPE
    assert L.pt_loc_atom_wait_f32(n, 1.0, n) == A.PT_AL_ERR_NULL
    assert b"NULL" in L.pt_loc_strerror(A.PT_AL_ERR_NULL) and b"unsupported" in L.pt_loc_strerror(A.PT_AL_ERR_UNSUPPORTED)
    assert L.pt_loc_abi_version() == 1


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
    """the dynamic symbol table of libpt_loc.so holds exactly the functions include/pt_loc.h declares; libpt_hot's and libpt_mot's sets are
    what their headers declare, and none of them is a pt_loc_ name"""
    defined = _defined(_lib_loc.LIB_PATH)
    assert defined == set(_lib_loc.EXPORTS) and len(defined) == 6 and all(s.startswith("pt_loc_") for s in defined)
    assert _lib_loc.EXPORTS == ["pt_loc_strerror", "pt_loc_abi_version", "pt_loc_atom_constants_f32", "pt_loc_atom_ws_bytes", "pt_loc_atom_f32",
                                "pt_loc_atom_wait_f32"]
    _lib_mot.build_library()
    mot = _defined(_lib_mot.LIB_PATH)
    assert mot == set(_lib_mot.EXPORTS) and len(mot) == 6 and all(s.startswith("pt_mot_") for s in mot)
    _lib.build_library()
    hot = _defined(_lib.LIB_PATH)
    assert hot == set(_lib.EXPORTS) and not any(s.startswith(("pt_loc_", "pt_mot_")) for s in hot)


def test_derived_bindings_match_the_host_compiler(tmp_path):
    """sizeof / offsetof of the structs and the value of every constant of include/pt_loc.h, printed by a C program generated from the parsed
    header, equal the ctypes classes and attributes of _lib_loc (the check tests/test_tamos_readout_cpu.py makes for include/pt_mot.h)."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    with open(os.path.join(ROOT, "include", "pt_loc.h")) as fh:
        abi = _abi.parse(fh.read())
    assert list(abi.structs) == ["pt_loc_atom_state", "pt_loc_atom_params"] and list(abi.functions) == _lib_loc.EXPORTS
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "pt_loc.h"', "int main(void) {"]
    src += [f'    printf("{k} %lld\\n", (long long){k});' for k in abi.constants]
    for cname, cls in abi.structs.items():
        src.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        src += [f'    printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(src + ["    return 0;", "}"]) + "\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, text=True)
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                                                   text=True).stdout.splitlines()}
    want = {k: [getattr(_lib_loc, k)] for k in abi.constants}
    for cname in abi.structs:
        cls = getattr(_lib_loc, _abi.class_name(cname))
        want[cname] = [ctypes.sizeof(cls)]
        for f, t in cls._fields_:
            want[f"{cname}.{f}"] = [getattr(cls, f).offset, ctypes.sizeof(t)]
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    c = ctypes
    restype, args = abi.functions["pt_loc_atom_f32"]
    assert restype is c.c_int and [t.__name__ for t in args] == ["c_void_p", "c_int", "c_int", "c_int", "c_int", "c_int", "c_void_p", "LP_LocAtomParams",
                                                                 "c_void_p", "c_void_p", "c_void_p", "c_float", "c_void_p", c.c_size_t.__name__, "c_void_p"]
    assert abi.functions["pt_loc_atom_ws_bytes"] == (c.c_size_t, [c.c_int] * 5) and abi.functions["pt_loc_strerror"] == (c.c_char_p, [c.c_int])
    assert [_lib_loc.PT_AL_NORMAL, _lib_loc.PT_AL_HARD_NEGATIVE, _lib_loc.PT_AL_UNCERTAIN, _lib_loc.PT_AL_NOT_FOUND] == [0, 1, 2, 3]
    assert _lib_loc.FLAGS == _lib.PT_LOC_FLAGS == RN.FLAGS


def test_install_switch_is_off_by_default_and_the_module_never_imports_the_oracle():
    from pytracking_amd import install
    assert inspect.signature(install.install).parameters["atom_localize"].default is False
    src = open(os.path.join(ROOT, "pytracking_amd", "atom_localize.py")).read()
    assert "import oracle" not in src and "from oracle" not in src and "torch.rfft" in inspect.getdoc(__import__("pytracking_amd.atom_localize", fromlist=["x"]))


@f64_bound.needs_bundle
def test_install_round_trip_and_default_rebinds_nothing_new():
    from oracle import ref_harness
    ref_harness.install()
    from pytracking.tracker.atom.atom import ATOM
    from pytracking_amd import install as amd
    amd.uninstall()
    ref = vars(ATOM)["localize_target"]
    try:
        amd.install()
        assert vars(ATOM)["localize_target"] is ref                           # a default install() leaves the method alone
        default_ledger = [(o, n) for o, n, _, _ in amd._state["ledger"]]
        amd.uninstall()
        amd.install(atom_localize=True)
        assert vars(ATOM)["localize_target"] is not ref and amd.original(ATOM, "localize_target") is ref
        assert vars(ATOM)["localize_target"].__wrapped__ is ref
        extra = [(o, n) for o, n, _, _ in amd._state["ledger"]]
        assert extra[:len(default_ledger)] == default_ledger and extra[len(default_ledger):] == [(ATOM, "localize_target")]
        # a CPU tensor is not covered: handed to the reference method (counted), or refused under strict
        from pytracking_amd import atom_localize as AL
        import torch
        trk = C.bare_tracker(C.CASES["n4_g9"])
        assert not AL.covered_localize_target(trk, torch.from_numpy(C.CASES["n4_g9"]["scores"].copy()))
    finally:
        amd.uninstall()
    assert vars(ATOM)["localize_target"] is ref
