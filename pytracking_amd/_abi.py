"""Reader of include/pt_hot.h: the C ABI as ctypes, so that _lib.py restates none of it by hand.

`parse(text)` understands exactly what the header uses -- `#define PT_X <integer>`, enums, `typedef struct`, function prototypes -- and
raises AbiError, quoting the text, on anything else at file scope.  It never skips: a construct it would have to guess at (a union, a
bitfield, a function pointer, a conditional block, an unknown type name) is an error at import, not a binding that loads and then hands
the kernels garbage.

Type map: the C scalars below; a pointer to a struct of the header -> POINTER(that Structure); a `const char*` return -> c_char_p;
every other pointer, pointer to pointer or array parameter -> c_void_p.  The header cannot tell a host array from a device pointer,
and c_void_p takes both: `tensor.data_ptr()` integers, None, ctypes arrays, byref() and pointer instances.
"""
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double, "long": ctypes.c_long,
           "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "unsigned char": ctypes.c_ubyte}
_POINTEES = ("void", "char")                          # type names that are valid behind a `*` only
_DECLARATOR = r"((?:\*\s*)*)(\w+)\s*(?:\[\s*(\w+)\s*\])?"                  # [stars] name [[length]]
_FIRST = re.compile(r"(\w[\w ]*?)\s*" + _DECLARATOR)                        # base type, then the first declarator
_DEFINE = re.compile(r"#define (PT_\w+) (\S+)")
_ENUM = re.compile(r"(typedef\s+)?enum\s*(\w*)\s*\{(.*)\}\s*(\w*)", re.S)
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{(.*)\}\s*(\w+)", re.S)
_PROTO = re.compile(r"([\w\s*]+?)\b(\w+)\s*\((.*)\)", re.S)


class AbiError(ValueError):
    pass


class Abi:
    def __init__(self):
        self.constants = {}        # name -> int of every #define and enumerator, in header order
        self.structs = {}          # C name -> ctypes.Structure subclass, in header order
        self.functions = {}        # name -> (restype, [argtypes]), in header order


def class_name(c_name):
    """pt_sd_params -> SdParams"""
    return "".join(w.capitalize() for w in c_name.split("_")[1:])


def _integer(abi, s, what):
    s = s.strip()
    if re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", s):
        return int(s, 0)
    if s in abi.constants:
        return abi.constants[s]
    raise AbiError(f"not an integer or an earlier constant: {s!r} in {what!r}")


def _ctype(abi, base, stars, length, what, param=False, ret=False):
    if base not in SCALARS and base not in abi.structs and base not in _POINTEES:
        raise AbiError(f"unknown type {base!r} in {what!r}")
    if length is not None:                             # an array parameter is a pointer, an array field an array
        return ctypes.c_void_p if param else _ctype(abi, base, stars, None, what) * _integer(abi, length, what)
    if stars == 1 and base in abi.structs:
        return ctypes.POINTER(abi.structs[base])
    if stars:
        return ctypes.c_char_p if ret and (base, stars) == ("char", 1) else ctypes.c_void_p
    if base not in SCALARS:
        raise AbiError(f"{base!r} by value in {what!r}")
    return SCALARS[base]


def _declarators(abi, decl, what, param=False):
    """[(name, ctype)] of `float *filter, *mem_feat`, `float rand_u[60]`, `const pt_sd_params* sd`, `const float box[4]`, ..."""
    if re.search(r"[():{}]", decl):
        raise AbiError(f"function pointer, bitfield or nested aggregate: {what!r}")
    out, base = [], None
    for part in re.sub(r"\bconst\b", " ", decl).split(","):
        m = re.fullmatch(_DECLARATOR, part.strip()) if out else _FIRST.fullmatch(part.strip())
        if not m:
            raise AbiError(f"cannot read the declaration {what!r}")
        if not out:
            base = " ".join(m.group(1).split())
        stars, name, length = m.groups()[-3:]
        if name in SCALARS or name in _POINTEES:
            raise AbiError(f"declaration without a name: {what!r}")
        out.append((name, _ctype(abi, base, stars.count("*"), length, what, param=param)))
    return out


def _define(abi, m, stmt):
    if m.group(1) in abi.constants:
        raise AbiError(f"constant {m.group(1)!r} defined twice")
    abi.constants[m.group(1)] = _integer(abi, m.group(2), stmt)


def _enum(abi, m, stmt):
    if bool(m.group(1)) != bool(m.group(4)):
        raise AbiError(f"enum that declares a variable, or typedef without a name: {stmt[:80]!r}")
    value = -1
    for item in m.group(3).split(","):
        if not item.strip():
            continue                                   # trailing comma
        name, _, expr = (s.strip() for s in item.partition("="))
        if not re.fullmatch(r"[A-Za-z_]\w*", name) or name in abi.constants:
            raise AbiError(f"bad or repeated enumerator {item.strip()!r} in {stmt[:80]!r}")
        value = _integer(abi, expr, item) if expr else value + 1
        abi.constants[name] = value


def _struct(abi, m, stmt):
    name, fields = m.group(3), []
    if name in abi.structs:
        raise AbiError(f"struct {name!r} declared twice")
    for decl in m.group(2).split(";"):
        if decl.strip():
            fields += _declarators(abi, decl, decl.strip())
    abi.structs[name] = type(class_name(name), (ctypes.Structure,), {"__doc__": f"`{name}` of include/pt_hot.h.", "_fields_": fields})


def _prototype(abi, m, stmt):
    ret, name, params = re.sub(r"\bconst\b", " ", m.group(1)), m.group(2), m.group(3).strip()
    if name in abi.functions:
        raise AbiError(f"function {name!r} declared twice")
    base, stars = " ".join(ret.replace("*", " ").split()), ret.count("*")
    restype = None if (base, stars) == ("void", 0) else _ctype(abi, base, stars, None, stmt, ret=True)
    args = []
    for p in ([] if params == "void" else params.split(",")):
        args += [t for _, t in _declarators(abi, p, stmt, param=True)]
    abi.functions[name] = (restype, args)


def _statements(text):
    """The `;`-terminated statements at file scope (a `;` inside braces belongs to its statement)."""
    depth, start = 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            yield text[start:i].strip()
            start = i + 1
    if text[start:].strip():
        raise AbiError(f"unterminated text at file scope: {text[start:].strip()[:80]!r}")


def parse(text):
    abi = Abi()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    # the two conditional blocks a C header has: both halves of `extern "C"` for C++, and the include guard
    text = re.sub(r'#ifdef\s+__cplusplus\s*\n\s*(extern\s+"C"\s*\{|\})\s*\n\s*#endif', " ", text)
    guard = re.fullmatch(r"\s*#ifndef\s+(\w+)\s*\n\s*#define\s+\1[ \t]*\n(.*)#endif\s*", text, re.S)
    if guard:
        text = guard.group(2)
    lines = []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            d = re.fullmatch(r"\s*#\s*define\s+(\w+)\s+(\S+)\s*", line)
            if d:
                line = f"#define {d.group(1)} {d.group(2)};"           # a statement in its place: a later array length may name it
            elif re.fullmatch(r"\s*#\s*include\s*<[\w./]+>\s*", line):
                line = ""
            else:
                raise AbiError(f"preprocessor line the reader does not know: {line.strip()!r}")
        lines.append(line)
    for stmt in _statements("\n".join(lines)):
        for pattern, handler in ((_DEFINE, _define), (_ENUM, _enum), (_STRUCT, _struct), (_PROTO, _prototype)):
            m = pattern.fullmatch(stmt)
            if m:
                handler(abi, m, stmt)
                break
        else:
            raise AbiError(f"not a constant, an enum, a typedef struct or a prototype: {stmt[:120]!r}")
    return abi
