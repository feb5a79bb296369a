"""Loader of libpt_hot.so; its ctypes prototypes, structs and constants are derived from include/pt_hot.h (_abi.py).

The product path has no fallback: if the shared library is missing or a call fails, a RuntimeError is
raised.  `build_library()` compiles it in-tree with hipcc for gfx950 (cross-compiles without a GPU).
"""
import ctypes
import os
import subprocess

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PT_HOT_LIB", os.path.join(_HERE, "libpt_hot.so"))   # override: experiments only
_CSRC = os.path.join(_HERE, "csrc")
SOURCES = sorted(f for f in os.listdir(_CSRC) if f.endswith(".hip"))
HEADERS = sorted(f for f in os.listdir(_CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "pt_hot.h")]    # relative to csrc/
# kernarg preload: leading scalar kernel parameters arrive in SGPRs at wave launch (kernels that take them that way only)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-mllvm", "-amdgpu-kernarg-preload-count=14"]

# The C ABI, read from the header at import (_abi.py): nothing below restates a prototype, a struct layout or a constant.
with open(os.path.join(_CSRC, HEADERS[-1])) as _fh:
    _ABI = _abi.parse(_fh.read())
EXPORTS = list(_ABI.functions)                                             # every declared function, in header order
globals().update(_ABI.constants)                                           # PT_ERR_NULL, PT_SD_PRDIMP, PT_TCM_MAX_POINTS, ...
globals().update({c.__name__: c for c in _ABI.structs.values()})           # pt_sd_params -> SdParams, pt_eco_fu_block -> EcoFuBlock, ...


def _enum_run(prefix, keep=""):
    """(first value, names by value) of the enumerators `prefix*` without their _COUNT / _END sentinel; `keep` replaces the prefix."""
    run = sorted((v, keep + k[len(prefix):]) for k, v in _ABI.constants.items() if k.startswith(prefix) and not k.endswith(("_COUNT", "_END")))
    if [v for v, _ in run] != list(range(run[0][0], run[0][0] + len(run))):
        raise _abi.AbiError(f"the {prefix}* values of include/pt_hot.h are not consecutive")
    return run[0][0], tuple(n for _, n in run)


# what pt_tomp_*_routes report, and from 1000 / 2000 what pt_tamos_predict_routes and pt_tamos_bbreg_routes / pt_fpn2_routes report next to it
TOMP_ROUTES = _enum_run("PT_TOMP_R_")[1]
TAMOS_ROUTE_BASE, TAMOS_ROUTES = _enum_run("PT_TAMOS_R_", "TAMOS_")
HEADS_ROUTE_BASE, HEADS_ROUTES = _enum_run("PT_HEADS_R_", "HEADS_")
PT_LOC_FLAGS = tuple(n.lower() for n in _enum_run("PT_LOC_")[1])


def _build_flags():
    return HIPCC_FLAGS + os.environ.get("PT_HOT_CFLAGS", "").split()


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    if "PT_HOT_LIB" in os.environ:                           # an experiment's prebuilt variant is never rebuilt from the current sources
        return False
    stamp = os.path.join(_HERE, "build", "flags.txt")       # a changed PT_HOT_CFLAGS is a rebuild, not a silently stale library
    if os.path.exists(stamp) and open(stamp).read() != " ".join(_build_flags()):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(os.path.join(_CSRC, d)) > t for d in SOURCES + HEADERS)


def build_library(force=False, verbose=False) -> str:
    """hipcc --offload-arch=gfx950 -> pytracking_amd/libpt_hot.so (in-tree, travels with the repo snapshot).
    One object per source under pytracking_amd/build/ (compiled in parallel, only the stale ones unless `force`), then
    one link step."""
    if not force and not needs_build():
        return LIB_PATH
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _build_flags()
    bdir = os.path.join(_HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    stamp = os.path.join(bdir, "flags.txt")
    if not os.path.exists(stamp) or open(stamp).read() != " ".join(flags):
        force = True
    hdr_t = max(os.path.getmtime(os.path.join(_CSRC, h)) for h in HEADERS)

    def compile_one(src):
        spath = os.path.join(_CSRC, src)
        obj = os.path.join(bdir, os.path.splitext(src)[0] + ".o")
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(spath), hdr_t):
            return obj, None
        cmd = [hipcc] + flags + ["-c", spath, "-o", obj]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if verbose or res.returncode != 0:
            print(" ".join(cmd))
            print(res.stdout, res.stderr)
        return obj, (res.stderr if res.returncode != 0 else None)

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4, int(os.environ.get("MAX_JOBS", 16)))) as ex:
        results = list(ex.map(compile_one, SOURCES))
    errs = [e for _, e in results if e]
    if errs:
        raise RuntimeError("hipcc failed building libpt_hot.so:\n" + "\n".join(errs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + [o for o, _ in results]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd))
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed linking libpt_hot.so:\n" + res.stderr)
    with open(stamp, "w") as fh:
        fh.write(" ".join(flags))
    return LIB_PATH


_lib = None


def lib():
    """The loaded library (ctypes.CDLL) with argtypes set.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback on the product path)")
    L = ctypes.CDLL(LIB_PATH)
    missing = [name for name in EXPORTS if not hasattr(L, name)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} lacks symbols that include/pt_hot.h declares: {missing}")
    for name, (restype, argtypes) in _ABI.functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what} failed: {lib().pt_strerror(status).decode()} ({status})")

