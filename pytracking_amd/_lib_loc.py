"""Loader of libpt_loc.so, the third C-ABI library (ATOM's per-frame score localisation); its ctypes prototypes, structs and constants are
derived from include/pt_loc.h by the reader of _abi.py, as _lib_mot.py derives libpt_mot's from include/pt_mot.h.

It is a library of its own because the function sets of include/pt_hot.h (tests/test_abi_cpu.py) and include/pt_loc.h
(tests/test_tamos_readout_cpu.py) are pinned.  Same flags as libpt_hot (`_lib.HIPCC_FLAGS`), sources pytracking_amd/csrc_loc/*.hip, which
may include unchanged headers of csrc/, objects under pytracking_amd/build/loc/.  No fallback: a missing library or a failed call raises.
"""
import ctypes
import os
import subprocess

from . import _abi, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpt_loc.so")
_CSRC = os.path.join(_HERE, "csrc_loc")
HEADER = os.path.join(_HERE, "..", "include", "pt_loc.h")
SOURCES = sorted(f for f in os.listdir(_CSRC) if f.endswith(".hip"))
# what a source of csrc_loc/ may include: its own headers, the headers of csrc/ and both public headers
_DEPS = ([os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith(".h")]
         + [os.path.join(_HERE, "csrc", h) for h in _lib.HEADERS] + [HEADER])

with open(HEADER) as _fh:
    _ABI = _abi.parse(_fh.read())
EXPORTS = list(_ABI.functions)                                             # every declared function, in header order
globals().update(_ABI.constants)                                           # PT_AL_ERR_NULL, PT_AL_REC_FLOATS, PT_AL_R_FLAG, ...
globals().update({c.__name__: c for c in _ABI.structs.values()})           # pt_loc_atom_state -> LocAtomState, pt_loc_atom_params -> LocAtomParams
FLAGS = _lib.PT_LOC_FLAGS                                                  # 'normal', 'hard_negative', 'uncertain', 'not_found' by code
if [_ABI.constants["PT_AL_" + n.upper()] for n in FLAGS] != list(range(len(FLAGS))):
    raise _abi.AbiError("the PT_AL_* flags of include/pt_loc.h are not the PT_LOC_* flags of include/pt_hot.h")


def _build_flags():
    return _lib._build_flags()


def _stamp():
    return os.path.join(_HERE, "build", "loc", "flags.txt")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    if os.path.exists(_stamp()) and open(_stamp()).read() != " ".join(_build_flags()):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in [os.path.join(_CSRC, s) for s in SOURCES] + _DEPS)


def build_library(force=False, verbose=False) -> str:
    """hipcc --offload-arch=gfx950 -> pytracking_amd/libpt_loc.so (in-tree), objects under pytracking_amd/build/loc/."""
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
            raise RuntimeError("hipcc failed building libpt_loc.so:\n" + res.stderr)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd))
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed linking libpt_loc.so:\n" + res.stderr)
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
        raise RuntimeError(f"{LIB_PATH} lacks symbols that include/pt_loc.h declares: {missing}")
    for name, (restype, argtypes) in _ABI.functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _loaded = L
    return L


def check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what} failed: {lib().pt_loc_strerror(status).decode()} ({status})")
