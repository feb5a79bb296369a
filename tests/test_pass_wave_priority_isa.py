"""Static wave priority in the two feature passes (gfx950 assembly, cross-compiled on the CPU box; no GPU): where `s_setprio` occurs in
the compiled csrc/fast_passes.hip, and that it occurs nowhere else (PT_C2_PRIO / PT_ADJ_PRIO; profiles/r12a_pass_wave_arbitration.txt).

`s_setprio` is a scalar instruction and ignores EXEC: under a vector condition (`s_and_saveexec`) every wave of the workgroup would
run it, which changes nothing.  It pays only for the waves the others wait for, so it has to sit

  k_corr2 (the three arms the DiMP-50 frame launches): inside the straight-line code of the wave kind with the leftover quads -- the
      body of 3 MFMAs and 2 loads per k-step, selected by a scalar branch -- and never between the first and the last MFMA of a body;
  k_adj2<V_DIMP_RELU, 6, 16>: directly under a scalar conditional branch (`s_cbranch_scc*`), as its fall-through or its target,
      with no `s_and_saveexec` between the branch and it; once, nothing in the MFMA loop.

What ships is read from the defaults of the two macros in the source (0 or no such macro: that part does not ship, and the instruction
must be absent from its kernels).  No other kernel of the file may hold the instruction."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_corr2_feature_stream_isa import CSRC, FRAME_KERNELS, NK, analyse, asm, kernel_lines, source_depth  # noqa: E402,F401

ADJ_ARM = "_Z6k_adj2ILi1ELi6ELi16ELb0EE"                         # k_adj2<V_DIMP_RELU, 6, 16, INIT = false>
# PT_C2_PRIO -> (s_setprio per frame arm, raises in the (3, 2) body, raises in the full-tile body)
C2_COUNTS = {0: (0, 0, 0), 1: (2, 1, 0), 2: (2, 1, 0), 3: (1, 1, 0), 4: (4, 1, 1)}


def shipped(name):
    m = re.search(r"^#define %s (\d+)" % name, open(os.path.join(CSRC, "fast_passes.hip")).read(), re.M)
    return int(m.group(1)) if m else 0


def all_kernels(text):
    return sorted(set(re.findall(r"^(_Z\w+):", text, re.M)))


def prio_lines(lines):
    return [n for n, l in enumerate(lines) if l.startswith("s_setprio")]


def _is_edge(l):
    return l.endswith(":") or l.startswith(("s_cbranch", "s_branch"))


def corr2_findings(lines, variant):
    """-> failures of one frame arm of k_corr2 for PT_C2_PRIO = variant."""
    fails = []
    bodies, _ = analyse(lines, source_depth())
    kinds = {(len(b["mfmas"]) // NK, b["loads_per_kstep"]): b for b in bodies}
    assert sorted(kinds) == [(2, 1), (3, 2), (4, 1)], sorted(kinds)
    total, in_lt, in_full = C2_COUNTS[variant]
    at = prio_lines(lines)
    if len(at) != total:
        fails.append("%d s_setprio, want %d" % (len(at), total))
    for n in at:
        for b in bodies:
            if b["mfmas"][0] < n < b["mfmas"][-1]:
                fails.append("line %d (%s) between the first and the last MFMA of a body" % (n, lines[n]))

    def span(b):                                                    # the body's straight-line code up to its first MFMA
        entry = max(m for m in range(b["first_load"]) if _is_edge(lines[m]))
        return entry, b["mfmas"][0]

    def raises_in(b, own_branch):
        lo, hi = span(b)
        hits = [n for n in at if lo < n < hi and not lines[n].endswith(" 0")]
        if own_branch:                                              # under a scalar branch of its own inside the body
            hits = [n for n in hits if any(lines[m].startswith("s_cbranch_scc") for m in range(max(lo, n - 8), n))
                    and not any(lines[m].startswith("s_and_saveexec") for m in range(max(lo, n - 8), n))]
        return hits

    lt = kinds[(3, 2)]
    if len(raises_in(lt, False)) != in_lt:
        fails.append("%d raises in the (3, 2) body, want %d" % (len(raises_in(lt, False)), in_lt))
    if len(raises_in(kinds[(4, 1)], True)) != in_full:
        fails.append("%d raises under a scalar branch in the full-tile body, want %d" % (len(raises_in(kinds[(4, 1)], True)), in_full))
    if raises_in(kinds[(2, 1)], False):
        fails.append("a raise in the half-1 body")
    # a lowering follows the last MFMA of its body in straight-line code
    for n in at:
        if lines[n].endswith(" 0"):
            ends = [b["mfmas"][-1] for b in bodies if b["mfmas"][-1] < n]
            if not ends or any(_is_edge(lines[m]) for m in range(max(ends), n)):
                fails.append("line %d: s_setprio 0 not in the straight-line code behind a body's last MFMA" % n)
    return fails


def adj2_findings(lines, variant):
    """-> failures of k_adj2<V_DIMP_RELU, 6, 16> for PT_ADJ_PRIO = variant."""
    fails = []
    at = prio_lines(lines)
    if len(at) != (1 if variant else 0):
        fails.append("%d s_setprio, want %d" % (len(at), 1 if variant else 0))
    mf = [n for n, l in enumerate(lines) if l.startswith("v_mfma")]
    labels = {l[:-1]: n for n, l in enumerate(lines) if l.endswith(":")}
    for n in at:
        if not lines[n].endswith(" 1"):
            fails.append("line %d: %s, want a raise to 1" % (n, lines[n]))
        if mf[0] < n < mf[-1]:
            fails.append("line %d inside the MFMA loop" % n)
        br = next((m for m in range(n - 1, -1, -1) if lines[m].startswith(("s_cbranch", "s_branch"))), None)
        if br is None or not lines[br].startswith("s_cbranch_scc"):
            fails.append("line %d: no s_cbranch_scc in front of the raise (%s)" % (n, None if br is None else lines[br]))
            continue
        between = lines[br + 1:n]
        if any(l.startswith("s_and_saveexec") for l in between):
            fails.append("line %d: s_and_saveexec between the branch and the raise" % n)
        marks = [m for m in range(br + 1, n) if lines[m].endswith(":")]
        target = labels.get(lines[br].split()[-1])
        if marks and marks != [target]:                             # not the fall-through: then the branch's own target block
            fails.append("line %d: the raise is neither the fall-through nor the target of the branch at line %d" % (n, br))
    return fails


@pytest.mark.parametrize("which", sorted(FRAME_KERNELS))
def test_corr2_frame_arm_priority(asm, which):
    fails = corr2_findings(kernel_lines(asm, FRAME_KERNELS[which]), shipped("PT_C2_PRIO"))
    assert not fails, "\n".join(fails)


def test_adj2_young_half_priority(asm):
    names = [k for k in all_kernels(asm) if k.startswith(ADJ_ARM)]
    assert len(names) == 1, names
    fails = adj2_findings(kernel_lines(asm, names[0]), shipped("PT_ADJ_PRIO"))
    assert not fails, "\n".join(fails)


def test_no_other_kernel_changes_priority(asm):
    want = set()
    if shipped("PT_C2_PRIO"):
        want |= {k for k in all_kernels(asm) if any(k.startswith(f) for f in FRAME_KERNELS.values())}
        assert len(want) == 3, want
    if shipped("PT_ADJ_PRIO"):
        want |= {k for k in all_kernels(asm) if k.startswith(ADJ_ARM)}
    names = all_kernels(asm)
    assert len(names) >= 150, len(names)
    have = {k for k in names if prio_lines(kernel_lines(asm, k))}
    assert have == want, (sorted(have - want), sorted(want - have))


if __name__ == "__main__":                                         # python tests/test_pass_wave_priority_isa.py file.s C2_PRIO ADJ_PRIO
    text = open(sys.argv[1]).read()
    c2, adj = int(sys.argv[2]), int(sys.argv[3])
    for key, mangled in sorted(FRAME_KERNELS.items()):
        print(key, corr2_findings(kernel_lines(text, mangled), c2))
    print("adj2", adj2_findings(kernel_lines(text, [k for k in all_kernels(text) if k.startswith(ADJ_ARM)][0]), adj))
    print("kernels with s_setprio:", [k[:48] for k in all_kernels(text) if prio_lines(kernel_lines(text, k))])
