"""Loader of libpt_bbn.so, the fifth C-ABI library (the ResNet backbone forward of the trackers); its ctypes prototypes, structs and
constants are derived from include/pt_bbn.h by the reader of _abi.py, as _lib_mem.py derives libpt_mem's from include/pt_mem.h.

It is a library of its own because the function sets of include/pt_hot.h (tests/test_abi_cpu.py), include/pt_mot.h
(tests/test_tamos_readout_cpu.py), include/pt_loc.h (tests/test_atom_localize_cpu.py) and include/pt_mem.h (tests/test_mem_update_cpu.py)
are pinned.  Same flags as libpt_hot (`_lib.HIPCC_FLAGS`), sources pytracking_amd/csrc_bbn/*.hip, which may include unchanged headers of
csrc/, objects under pytracking_amd/build/bbn/.  No fallback: a missing library or a failed call raises.
"""
import ctypes
import os
import subprocess

from . import _abi, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpt_bbn.so")
_CSRC = os.path.join(_HERE, "csrc_bbn")
HEADER = os.path.join(_HERE, "..", "include", "pt_bbn.h")
SOURCES = sorted(f for f in os.listdir(_CSRC) if f.endswith(".hip"))
# what a source of csrc_bbn/ may include: its own headers, the headers of csrc/ and both public headers
_DEPS = ([os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith(".h")]
         + [os.path.join(_HERE, "csrc", h) for h in _lib.HEADERS] + [HEADER])

with open(HEADER) as _fh:
    _ABI = _abi.parse(_fh.read())
EXPORTS = list(_ABI.functions)                                             # every declared function, in header order
globals().update(_ABI.constants)                                           # PT_BBN_ERR_NULL, PT_BBN_R_T128, PT_BBN_OUT_LAYER3, ...
globals().update({c.__name__: c for c in _ABI.structs.values()})           # pt_bbn_desc -> BbnDesc, pt_bbn_launch -> BbnLaunch
OUTPUTS = ("conv1", "layer1", "layer2", "layer3", "layer4")                # PT_BBN_OUT_* by bit
if [_ABI.constants["PT_BBN_OUT_" + o.upper()] for o in OUTPUTS] != list(range(len(OUTPUTS))):
    raise _abi.AbiError("the PT_BBN_OUT_* codes of include/pt_bbn.h are not 0..4 in network order")
ROUTES = tuple(k[len("PT_BBN_R_"):] for k, v in sorted(_ABI.constants.items(), key=lambda kv: kv[1])
               if k.startswith("PT_BBN_R_") and k != "PT_BBN_R_COUNT")     # route names by code
KERNELS = ("k_conv", "k_conv_stem", "k_pool", "k_reduce")                  # PT_BBN_K_* by code


def _build_flags():
    return _lib._build_flags()


def _stamp():
    return os.path.join(_HERE, "build", "bbn", "flags.txt")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    if os.path.exists(_stamp()) and open(_stamp()).read() != " ".join(_build_flags()):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in [os.path.join(_CSRC, s) for s in SOURCES] + _DEPS)


def build_library(force=False, verbose=False) -> str:
    """hipcc --offload-arch=gfx950 -> pytracking_amd/libpt_bbn.so (in-tree), objects under pytracking_amd/build/bbn/."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _build_flags()
    bdir = os.path.dirname(_stamp())
    os.makedirs(bdir, exist_ok=True)
    objs = []
    for src in SOURCES:
        obj = os.path.join(bdir, os.path.splitext(src)[0] + ".o")
        cmd = [hipcc] + flags + ["-c", os.path.join(_CSRC, src), "-o", obj]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if verbose or res.returncode != 0:
            print(" ".join(cmd))
            print(res.stdout, res.stderr)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed building libpt_bbn.so:\n" + res.stderr)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd))
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed linking libpt_bbn.so:\n" + res.stderr)
    with open(_stamp(), "w") as fh:
        fh.write(" ".join(flags))
    return LIB_PATH


_loaded = None


def lib():
    """The loaded library (ctypes.CDLL) with argtypes set.  Raises if it has not been built."""
    global _loaded
    if _loaded is not None:
        return _loaded
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback on the product path)")
    L = ctypes.CDLL(LIB_PATH)
    missing = [name for name in EXPORTS if not hasattr(L, name)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} lacks symbols that include/pt_bbn.h declares: {missing}")
    for name, (restype, argtypes) in _ABI.functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _loaded = L
    return L


def check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what} failed: {lib().pt_bbn_strerror(status).decode()} ({status})")
