#!/usr/bin/env python3
"""What pytracking_amd/_lib.py binds of libpt_hot.so, as JSON (CPU only; the library must be built).

    python tools/dump_abi.py [OUT.json]      # default: stdout

Reads only _lib's public names and the function objects of _lib.lib(), so the same script describes any state of _lib.py:
tests/golden/abi_parent.json is its output at the last commit whose bindings were typed by hand, and tests/test_abi_cpu.py
holds the bindings derived from include/pt_hot.h to it.
  functions  {name: {"restype": type name ("void" for None), "argtypes": [type names] or null where unset}} of _lib.EXPORTS
  structs    {class name: {"sizeof": bytes, "fields": [[name, type name, offset], ...]}} of every ctypes.Structure
  constants  {name: value} of every public upper-case integer;  tuples  {name: [items]} of every public tuple
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _tname(t):
    return "void" if t is None else t.__name__


def dump():
    from pytracking_amd import _lib
    L = _lib.lib()
    public = {k: v for k, v in vars(_lib).items() if not k.startswith("_")}
    functions = {}
    for name in _lib.EXPORTS:
        fn = getattr(L, name)
        functions[name] = {"restype": _tname(fn.restype), "argtypes": None if fn.argtypes is None else [_tname(t) for t in fn.argtypes]}
    structs = {k: {"sizeof": ctypes.sizeof(v), "fields": [[n, _tname(t), getattr(v, n).offset] for n, t in v._fields_]}
               for k, v in public.items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    constants = {k: v for k, v in public.items() if k.isupper() and isinstance(v, int) and not isinstance(v, bool)}
    tuples = {k: list(v) for k, v in public.items() if isinstance(v, tuple)}
    return {"functions": functions, "structs": structs, "constants": constants, "tuples": tuples}


if __name__ == "__main__":
    text = json.dumps(dump(), indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
