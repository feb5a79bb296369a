"""The compiled schedule of k_corr2's feature stream (gfx950 assembly, cross-compiled on the CPU box; no GPU).

The source of the correlation pass can say "two k-steps ahead" while the ISA drains the pipeline: the compiler places every
`s_waitcnt vmcnt(N)` from its own count of the loads in flight, and a count that has to hold for a static path that skips loads
(a wave-uniform branch around a request) comes out as a smaller N than the waves need, down to vmcnt(0).  These tests read the
three instantiations the DiMP-50 frame launches, and then every other compiled instantiation with its own k-step count and depth,
and check what profiles/r10a_corr2_feature_stream.txt relies on:

 (i)   no `s_waitcnt vmcnt(0)` between the first feature load of a loop body and the first MFMA of its k-step NK - D;
 (ii)  every wait in front of k-step k < NK - D leaves at least (D - 1) x (loads per k-step of that wave kind) loads in flight;
 (iii) no conditional branch between two MFMAs of a body whose target block holds a buffer load (and, stricter: none at all);
 (iv)  the wait in front of the store of the filter operand to LDS leaves every feature load issued before it in flight, or none
       was issued before it.

A loop body = the MFMAs of one wave kind (full tile / half 0 + leftover quads / half 1 of tile 0): a run of MFMAs that no LDS store
and no barrier interrupts.  A k-step starts at every MFMA that writes the accumulator of the body's first MFMA.  A feature load
belongs to the k-step whose MFMAs read its destination registers.  D is read from the source (PT_C2_D)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytracking_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NK = 16
FRAME_KERNELS = {                      # template arguments <NK, LEFT, FUSE, K16, NH, MIX> in Itanium mangling
    "fuse8": "_Z7k_corr2ILi16ELb1ELi8ELb1ELi1ELb1EE",
    "lazy": "_Z7k_corr2ILi16ELb1ELin1ELb1ELi1ELb1EE",
    "plain": "_Z7k_corr2ILi16ELb1ELi0ELb1ELi1ELb1EE",
}


def source_depth():
    text = open(os.path.join(CSRC, "fast_passes.hip")).read()
    m = re.search(r"^#define PT_C2_D (\d+)", text, re.M)
    assert m, "PT_C2_D not defined in fast_passes.hip"
    return min(int(m.group(1)), NK)


def kernel_lines(asm, mangled):
    """The instruction / label lines of one kernel, comments stripped."""
    out, on = [], False
    for line in asm.splitlines():
        if not on:
            if line.startswith(mangled) and line.split(";")[0].strip().endswith(":"):
                on = True
            continue
        if line.startswith(".Lfunc_end"):
            break
        s = line.split(";")[0].strip()
        if s:
            out.append(s)
    assert out, mangled
    return out


def _regs(tok):
    """'v[6:9]' -> {6,7,8,9}; 'v12' -> {12}; anything else -> empty."""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def _ops(line):
    return [t.strip() for t in line.split(None, 1)[1].split(",")] if " " in line or "\t" in line else []


def _vmcnt(line):
    m = re.search(r"vmcnt\((\d+)\)", line)
    return int(m.group(1)) if line.startswith("s_waitcnt") and m else None


def analyse(lines, depth, NK=NK):
    """NK: k-steps per wave of the instantiation.  -> (bodies, failures).  bodies: [{"first_load", "ksteps", "loads_per_kstep"}]; failures: ["(i) ...", ...]."""
    fails = []
    mf = [n for n, l in enumerate(lines) if l.startswith("v_mfma")]
    assert mf, "no MFMA"
    groups, cur = [], [mf[0]]
    for a, b in zip(mf, mf[1:]):
        if any(lines[n].startswith(("ds_write", "s_barrier")) for n in range(a, b)):
            groups.append(cur)
            cur = []
        cur.append(b)
    groups.append(cur)
    labels = {l[:-1]: n for n, l in enumerate(lines) if l.endswith(":")}
    rsrcs, bodies = set(), []
    for g in groups:
        starts, chain = [g[0]], _ops(lines[g[0]])[0]               # the first accumulator's chain: D = A x B + C, C = the previous D
        for n in g[1:]:
            if _ops(lines[n])[3] == chain:
                starts.append(n)
                chain = _ops(lines[n])[0]
        assert len(starts) == NK, ("k-steps per body", len(starts))
        # where both bodies of a kernel request the same feature quads in front of barrier 1 the compiler hoists those requests above the
        # wave-kind branch: the text between them and this body then holds the loops of the bodies in front, which this wave never runs
        def entry(o):                                               # a body starts behind the wave-kind branch in front of its first MFMA
            return max([m for m in range(o[0]) if lines[m].startswith(("s_cbranch", "s_branch")) or lines[m].endswith(":")], default=0)
        mine = lambda n: not any(entry(o) <= n <= o[-1] for o in groups if o is not g)
        # feature loads: the last buffer load in front of an MFMA that writes the register its B operand reads
        kstep_of, per_k = {}, [set() for _ in range(NK)]
        for n in g:
            k = max(i for i, s in enumerate(starts) if s <= n)
            breg = _regs(_ops(lines[n])[2])
            for p in range(n - 1, -1, -1):
                if mine(p) and lines[p].startswith("buffer_load") and (_regs(_ops(lines[p])[0]) & breg):
                    kstep_of[p] = k
                    per_k[k].add(p)
                    rsrcs.add(_ops(lines[p])[2])
                    break
            else:
                raise AssertionError("no load feeds " + lines[n])
        # (where the compiler copied an operand into another register in front of its MFMA the search above lands on an older load of
        # that register: the count of a k-step is the one most k-steps agree on)
        counts = [len(s) for s in per_k]
        lpk = max(set(counts), key=counts.count)
        first_load = min(kstep_of)
        bodies.append({"first_load": first_load, "ksteps": starts, "loads_per_kstep": lpk, "mfmas": g})
        name = "body of %d MFMAs, %d load(s) per k-step" % (len(g), lpk)
        if depth < NK:
            stop = starts[NK - depth]
            for n in range(first_load, stop):
                if mine(n) and _vmcnt(lines[n]) == 0:
                    fails.append("(i) %s: vmcnt(0) at line %d, %d lines in front of k-step %d" % (name, n, stop - n, NK - depth))
            need = (depth - 1) * lpk
            for k in range(NK - depth):
                lo = first_load if k == 0 else starts[k - 1]
                for n in range(lo, starts[k]):
                    v = _vmcnt(lines[n])
                    if mine(n) and v is not None and v < need:
                        fails.append("(ii) %s: vmcnt(%d) in front of k-step %d leaves fewer than %d loads in flight" % (name, v, k, need))
        for n in range(g[0], g[-1]):
            if lines[n].startswith("s_cbranch"):
                fails.append("(iii+) %s: conditional branch inside the loop (line %d)" % (name, n))
                t = labels.get(_ops(lines[n])[0])
                assert t is not None, lines[n]
                end = next((m for m in range(t + 1, len(lines)) if lines[m].endswith(":")), len(lines))
                if any(lines[m].startswith("buffer_load") for m in range(t, end)):
                    fails.append("(iii) %s: branch at line %d to a block with a buffer load" % (name, n))
    # (iv) the filter operand's LDS store: the first ds_write behind the late argument block (the first s_load_dwordx16)
    late = next(n for n, l in enumerate(lines) if l.startswith("s_load_dwordx16"))
    store = next(n for n in range(late, len(lines)) if lines[n].startswith("ds_write"))
    assert len(rsrcs) == 1, rsrcs
    rs = next(iter(rsrcs))
    before = [n for n in range(store) if lines[n].startswith("buffer_load") and _ops(lines[n])[2] == rs]
    if before:
        waits = [_vmcnt(lines[n]) for n in range(before[0], store) if _vmcnt(lines[n]) is not None]
        if waits and min(waits) < len(before):
            fails.append("(iv) %d feature loads in front of the filter operand's LDS store, a wait there allows %d" % (len(before), min(waits)))
    return bodies, fails


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    sys.path.insert(0, ROOT)
    from pytracking_amd import _lib
    out = tmp_path_factory.mktemp("isa") / "fast_passes.s"
    cmd = [HIPCC, *[f for f in _lib.HIPCC_FLAGS if f != "-fPIC"], "--cuda-device-only", "-S", "-I", CSRC, "-I",
           os.path.join(ROOT, "include"), os.path.join(CSRC, "fast_passes.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


@pytest.mark.parametrize("which", sorted(FRAME_KERNELS))
def test_feature_stream_stays_in_flight(asm, which):
    depth = source_depth()
    bodies, fails = analyse(kernel_lines(asm, FRAME_KERNELS[which]), depth)
    # mixed pairs with leftover quads: half 0 + leftover (2 + 1 MFMAs, 2 loads per k-step), half 1 (2, 1), full tile (4, 1)
    assert sorted((len(b["mfmas"]) // NK, b["loads_per_kstep"]) for b in bodies) == [(2, 1), (3, 2), (4, 1)], bodies
    assert not fails, "\n".join(fails)


def arm_depth(nk, nh, depth):
    """The depth an instantiation runs with (k_corr2: D): the k-half arms of up to 8 k-steps keep 2 (80-VGPR cap), never more than NK."""
    return min(2 if (nk <= 8 and nh == 2 and depth > 2) else depth, nk)


def test_every_instantiation_has_exact_waits(asm):
    """The same four checks on every compiled k_corr2<NK, LEFT, FUSE, K16, NH, MIX>, with the k-steps and the depth of that arm."""
    arms = sorted(set(re.findall(r"^(_Z7k_corr2ILi(\d+)ELb[01]ELin?\d+ELb[01]ELi([12])ELb[01]EE)\w*:", asm, re.M)))
    assert len(arms) >= 100, len(arms)
    bad = []
    for mangled, nk, nh in arms:
        nk, nh = int(nk), int(nh)
        bodies, fails = analyse(kernel_lines(asm, mangled), arm_depth(nk, nh, source_depth()), nk)
        assert 1 <= len(bodies) <= 3, (mangled, len(bodies))
        bad += [mangled + ": " + f for f in fails]
    assert not bad, "\n".join(bad[:40])


if __name__ == "__main__":                                         # python tests/test_corr2_feature_stream_isa.py file.s [depth]
    text = open(sys.argv[1]).read()
    d = int(sys.argv[2]) if len(sys.argv) > 2 else source_depth()
    for key, mangled in sorted(FRAME_KERNELS.items()):
        bodies, fails = analyse(kernel_lines(text, mangled), d)
        print(key, "D =", d, [(len(b["mfmas"]) // NK, b["loads_per_kstep"]) for b in bodies], "failures:", len(fails))
        for f in fails:
            print("   ", f)
