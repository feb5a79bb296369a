#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two states of pytracking_amd/csrc (CPU only, no GPU needed).

    python tools/isa_diff.py [REV]          # REV (default HEAD) against the working tree

Every source of _lib.SOURCES is compiled device-only with _lib.HIPCC_FLAGS from both states; kernels are compared by their
demangled name in disassembly (instruction text, addresses dropped) and in the code-object notes (registers, LDS, arguments).
Classes: identical / differing / removed / new.  For differing kernels the report says whether the instruction streams are equal
once the immediate offsets of scalar loads (kernel-argument segment) are masked, and lists the metadata keys that changed.
`--table SUBSTR` adds a before/after resource table of the kernels whose name contains SUBSTR, `--show SUBSTR` their instruction diff.  Exit status 0 always: it reports.
"""
import argparse, difflib, os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytracking_amd import _lib  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "llvm", "bin")


def run(cmd, **kw):
    res = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if res.returncode:
        sys.exit(" ".join(cmd) + "\n" + res.stderr)
    return res.stdout


def kernels_of(csrc, src, out):
    """{demangled name: (instruction lines, metadata dict)} of one source."""
    co = os.path.join(out, src + ".co")
    flags = [f for f in _lib.HIPCC_FLAGS if f != "-fPIC"]
    run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, src), "-o", co])
    notes = run([os.path.join(LLVM, "llvm-readelf"), "--notes", co])
    meta = {k[".name"]: k for k in yaml.safe_load(notes[notes.index("amdhsa.kernels:"):notes.rindex("...")])["amdhsa.kernels"]}
    body, cur = {}, None
    for line in run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co]).splitlines():
        m = re.match(r"<(\S+)>:$", line)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    names = sorted(meta)
    dem = run([shutil.which("llvm-cxxfilt", path=LLVM) or "c++filt"], input="\n".join(names) + "\n").splitlines()
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"\(.*\)$", "", d.replace("(anonymous namespace)::", "").replace("void ", ""))    # name<template arguments>
        while body[n] and body[n][-1].startswith("s_nop"):           # padding up to the next symbol
            body[n].pop()
        res[d] = (body[n], {k: v for k, v in meta[n].items() if k not in (".name", ".symbol")})
    return res


def all_kernels(csrc, out, jobs):
    os.makedirs(out, exist_ok=True)
    sources = [s for s in _lib.SOURCES if os.path.exists(os.path.join(csrc, s))]      # a source one state does not have yet: its kernels are new
    with ThreadPoolExecutor(jobs) as ex:
        per = list(ex.map(lambda s: kernels_of(csrc, s, out), sources))
    return {f"{s}: {k}": v for s, d in zip(sources, per) for k, v in d.items()}


def occupancy(m):                                                   # waves per SIMD: 512 unified registers, granule 8, at most 8
    return min(8, 512 // max(8, -(-m[".vgpr_count"] // 8) * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("--table", action="append", default=[])
    ap.add_argument("--show", action="append", default=[], metavar="SUBSTR", help="print the instruction diff of differing kernels that match")
    ap.add_argument("--alias", action="append", default=[], metavar="REGEX=REPL", help="rename kernels of REV before matching")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 4))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, "pytracking_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old = all_kernels(os.path.join(tmp, "pytracking_amd", "csrc"), os.path.join(tmp, "old"), a.j)
        new = all_kernels(os.path.join(ROOT, "pytracking_amd", "csrc"), os.path.join(tmp, "new"), a.j)
    for al in a.alias:
        pat, repl = al.split("=", 1)
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    mask = lambda ins: [re.sub(r"^(s_load_dword\S* \S+ \S+) \S+$", r"\1 OFF", i) for i in ins]
    same = [k for k in old if k in new and old[k] == new[k]]
    diff = [k for k in old if k in new and old[k] != new[k]]
    print(f"{a.rev} -> working tree: {len(old)} kernels before, {len(new)} after")
    print(f"identical (instructions and metadata): {len(same)}\ndiffering: {len(diff)}")
    for k in diff:
        (oi, om), (ni, nm) = old[k], new[k]
        ins = "equal" if oi == ni else ("equal but for scalar-load offsets" if mask(oi) == mask(ni) else f"DIFFER ({len(oi)} -> {len(ni)})")
        keys = ", ".join(f"{x} {om.get(x)} -> {nm.get(x)}" if x != ".args" else f".args {len(om[x])} -> {len(nm[x])} entries" for x in sorted(set(om) | set(nm)) if om.get(x) != nm.get(x))
        print(f"  {k}\n      instructions {ins}; metadata: {keys or 'equal'}")
        if any(sub in k for sub in a.show):
            print("\n".join("        " + ln for ln in difflib.unified_diff(oi, ni, "before", "after", n=1, lineterm="")))
    for title, names in (("removed", sorted(set(old) - set(new))), ("new", sorted(set(new) - set(old)))):
        print(f"{title}: {len(names)}")
        for k in names:
            print(f"  {k}")
    for sub in a.table:
        print(f"\n{sub}: instructions / VGPRs / SGPRs / static LDS bytes / waves per SIMD, before -> after")
        for k in sorted(k for k in old if sub in k and k in new):
            row = lambda v: (len(v[0]), v[1][".vgpr_count"], v[1][".sgpr_count"], v[1][".group_segment_fixed_size"], occupancy(v[1]))
            o, n = row(old[k]), row(new[k])
            print(f"  {k}\n      " + "  ".join(f"{x} -> {y}" for x, y in zip(o, n)) + ("" if all(y <= x for x, y in zip(o[:4], n[:4])) and n[4] >= o[4] else "   WORSE"))


if __name__ == "__main__":
    main()
