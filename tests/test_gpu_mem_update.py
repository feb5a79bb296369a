"""The trackers' per-frame sample-memory update on the MI355X (csrc_mem/mem_update.hip through the C ABI of include/pt_mem.h and through
pytracking_amd.memory_update) against the float64 run of the numpy restatement (tests/mem_update_np.py) on the whole case table
(tests/mem_update_cases.py): no case is excluded -- tests/test_mem_update_cpu.py asserts that every discrete decision is an exact tie of
the float32 keys or keeps a margin of 16 x the bound below.

Bounds.  Indices and floor flags equal the restatement's.  The weights and the normalising sum lie within FACTOR x max(ref_err,
2^-23 max|want|) of float64: the bound of tests/f64_bound.py with its ulp_of_max floor, ref_err being the unmodified reference's own fp32
distance from its float64 run of that call (the goldens' after32 against after64; carried: against carry64).  Inserted rows are bit-equal
to their source (the threshold row to the reference's expression); every other slot, and the guard regions around every buffer, keep their
NaN prefill.  Figures are printed before they are asserted and, when MEM_UPDATE_F64_OUT names a file, written there as a table
(profiles/mem_update_f64.txt is the table of such a run)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import f64_bound
import mem_update_cases as C
import mem_update_np as RN
from pytracking_amd import _lib_mem as M
from pytracking_amd import memory_update as MU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# worst ratio of a device output to max(ref_err, ulp of max) measured on the MI355X (profiles/mem_update_f64.txt)
WORST_MEASURED = 1.67
F_MAX = 8                                          # tests/test_mem_update_cpu.py: every seeded defect misses this many units
FACTOR = f64_bound.raised_factor(WORST_MEASURED, F_MAX)
TABLE = f64_bound.Table("MEM_UPDATE_F64_OUT",
                        "Per-frame sample-memory update on the MI355X against float64 (tests/test_gpu_mem_update.py):\n"
                        "per case the worst call's max |out - float64| and its ratio to max(ref_err, 2^-23 max|want|) -- the unmodified reference's\n"
                        f"own fp32 distance from its float64 run of that call, floored at one fp32 ulp of the output's range; bound = {FACTOR} x that.")
GUARD = 64                                         # floats of NaN in front of and behind every buffer: 256 bytes, keeps 16-byte alignment
PROBE = 5                                          # floats per slot of the probe row every block of the weight cases carries


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """`count` buffers of `size` floats, each between two guards, NaN prefilled, in one device tensor"""

    def __init__(self, count, size):
        self.size, self.pitch = size, (size + 3) // 4 * 4 + 2 * GUARD
        self.t = torch.full((count, self.pitch), float("nan"), device=DEV)

    def view(self, i):
        return self.t[i, GUARD:GUARD + self.size]

    def ptr(self, i):
        return self.t.data_ptr() + 4 * (i * self.pitch + GUARD)

    def host(self):
        a = self.t.cpu().numpy()
        inner = a[:, GUARD:GUARD + self.size]
        guards = np.concatenate([a[:, :GUARD], a[:, GUARD + self.size:]], 1)
        assert np.isnan(guards).all(), "a guard region was written"
        return inner


def c_block(s, blk, weights_ptr, cert_ptr):
    q = M.MemBlock()
    q.weights, q.certainty, q.n, q.num_init, q.num_stored = weights_ptr, cert_ptr, s["n"], s["num_init"], blk["num_stored"]
    q.prev_ind = -1 if blk["prev_ind"] is None else blk["prev_ind"]
    q.rule, q.lower_init_weight, q.lr, q.floor = RN.RULES.index(s["rule"]), int(s["lower"]), blk["lr"], s["floor"]
    return q


def c_row(src, dst, elems, block, op=RN.COPY, arg=0.0):
    q = M.MemRow()
    q.src, q.dst, q.elems, q.block, q.op, q.arg = src, dst, elems, block, op, arg
    return q


def held(tag, rows):
    """rows: (what, err, ref_err, ulp floor).  Prints and records the worst, asserts all."""
    worst = max(rows, key=lambda r: r[1] / max(r[2], r[3]))
    ratio = worst[1] / max(worst[2], worst[3])
    print(f"\n{tag}: worst {worst[0]} max |out - float64| {worst[1]:.3e} = {ratio:.2f} x max(ref_err {worst[2]:.3e}, ulp of max {worst[3]:.3e}); bound {FACTOR} x")
    TABLE.row(tag, worst[1], worst[2], worst[3], ratio)
    for what, err, ref_err, floor in rows:
        assert err <= f64_bound.bound(ref_err, FACTOR, floor), (tag, what, err, ref_err, floor)


@pytest.mark.parametrize("name", C.CASES)
def test_every_case_through_the_c_abi(name):
    """every call of the case on the reference's fp32 state in front of it, NaN-prefilled record and probe memories"""
    specs, steps = C.CASES[name]
    T, B = len(steps), len(specs)
    g, seqs, runs = C.golden(name), C.states(name), C.run(name)
    W = [Guarded(T, s["n"]) for s in specs]
    P = [Guarded(T, s["n"] * PROBE) for s in specs]
    cert = [f64_bound.dev(g[f"cert_{b}"]) if s["rule"] == "D" else None for b, s in enumerate(specs)]
    rec = Guarded(T, M.PT_MEM_REC_FLOATS)
    ws = torch.zeros(256 * T, dtype=torch.uint8, device=DEV)
    src = torch.arange(1, T * B * PROBE + 1, dtype=torch.float32, device=DEV).reshape(T, B, PROBE)
    for b in range(B):
        for k in range(T):
            W[b].view(k).copy_(f64_bound.dev(g[f"before32_{b}"][k]))
    L = M.lib()
    for k, lr in enumerate(steps):
        blocks = (M.MemBlock * B)(*[c_block(s, C.block(s, seqs[b][k], lr), W[b].ptr(k), None if cert[b] is None else cert[b][k].data_ptr())
                                    for b, s in enumerate(specs)])
        rows = (M.MemRow * B)(*[c_row(src[k, b].data_ptr(), P[b].ptr(k), PROBE, b) for b in range(B)])
        assert L.pt_mem_update_f32(blocks, B, rows, B, rec.ptr(k), float(k + 1), ws.data_ptr() + 256 * k, 256, stream()) == 0
    torch.cuda.synchronize()
    R, found = rec.host(), []
    for b, s in enumerate(specs):
        w, p = W[b].host(), P[b].host().reshape(T, s["n"], PROBE)
        for k in range(T):
            r = runs[k][b]
            assert int(R[k, M.PT_MEM_R_INDEX + b]) == r["index"] and int(R[k, M.PT_MEM_R_FLOOR + b]) == r["floor"], (name, k, b, R[k])
            assert np.array_equal(p[k, r["index"]], src[k, b].cpu().numpy()) and np.isnan(np.delete(p[k], r["index"], 0)).all(), (name, k, b)
            ref = C.ref_err(name, b, k)
            found.append((f"weights[{b}] call {k}", float(np.abs(w[k] - r["weights"]).max()), ref, f64_bound.ulp_of_max(r["weights"])))
            found.append((f"sum[{b}] call {k}", abs(float(R[k, M.PT_MEM_R_SUM + b]) - float(r["total"])), ref, f64_bound.ulp_of_max(r["total"])))
    for k in range(T):
        assert (R[k, M.PT_MEM_R_SEQ:] == k + 1).all() and (R[k, M.PT_MEM_R_INDEX + B:M.PT_MEM_R_FLOOR] == 0).all(), (name, k, R[k])
    held(name, found)


@pytest.mark.parametrize("name", C.CASES)
def test_carried_sequence_through_memory_update_run(name):
    """the case carried on the device through MemoryUpdate.run: within the bound of the float64 restatement carried from the same start at
    every step; no wait while pt_mem_host_index answers, one wait otherwise"""
    specs, steps = C.CASES[name]
    B = len(specs)
    want = C.carried(name)
    sts = [C.initial(s) for s in specs]
    W = Guarded(B, max(s["n"] for s in specs))
    cert = [None if st["certainty"] is None else f64_bound.dev(st["certainty"]) for st in sts]
    for b, s in enumerate(specs):
        W.view(b)[:s["n"]].copy_(f64_bound.dev(sts[b]["weights"]))
    P = [torch.full((s["n"], PROBE), float("nan"), device=DEV) for s in specs]
    ctx, found, waits = MU.context(DEV), [], 0
    for k, lr in enumerate(steps):
        blocks = [MU.Block(W.view(b)[:s["n"]], s["num_init"], sts[b]["num_stored"], sts[b]["prev_ind"], s["lr"] if lr is None else lr, s["floor"],
                           s["rule"], cert[b], s["lower"]) for b, s in enumerate(specs)]
        x = torch.full((B, PROBE), float(k), device=DEV)
        before = ctx.waits
        idx = MU.run(blocks, [MU.Row(x[b], P[b], b) for b in range(B)])
        need_wait = any(RN.host_index(C.block(s, sts[b], lr, weights=np.empty(s["n"], np.float32))) < 0 for b, s in enumerate(specs))
        assert ctx.waits - before == int(need_wait), (name, k)
        waits += need_wait
        assert idx == [r["index"] for r in want[k]], (name, k, idx)
        w = W.host()
        for b, s in enumerate(specs):
            found.append((f"weights[{b}] call {k}", float(np.abs(w[b, :s["n"]] - want[k][b]["weights"]).max()), C.ref_err_carried(name, b, k),
                          f64_bound.ulp_of_max(want[k][b]["weights"])))
            assert (P[b][idx[b]] == k).all()
            sts[b] = C.advance(s, sts[b], idx[b], None, k)
            if cert[b] is not None:
                cert[b].copy_(f64_bound.dev(sts[b]["certainty"]))
    print(f"\n{name}: {waits} of {len(steps)} calls waited")
    held(name + " carried", found)


def _row_buffers(n, rows):
    out = []
    rng = np.random.default_rng(77)
    for name, elems, op, arg, off, block in rows:
        v = rng.standard_normal(off + elems + 3).astype(np.float32)
        if op == RN.THRESH:
            below = np.nextafter(np.float32(arg), np.float32(-1)) if arg else -np.finfo(np.float32).tiny      # the largest normal value below
            v[off], v[off + 1], v[off + 2] = np.float32(arg), np.nan, below
        out.append((f64_bound.dev(v), Guarded(1, n[block] * elems)))
    return out


@pytest.mark.parametrize("part", [0, 1])
def test_rows_are_stored_bit_for_bit_and_nothing_else_is_touched(part):
    """every row shape of the table, each op, a source at an offset inside a larger tensor, a row of the second block: the slot equals the
    source bit for bit, every other slot and both guards keep their NaN.  Block 0 chooses the odd slot 3 (a 5-float slot there is not 16-byte
    aligned), block 1 slot 1."""
    rows = C.ROWS[:8] if part == 0 else C.ROWS[8:]
    n = (7, 4)
    w0 = np.array([0.2, 0.15, 0.2, 0.05, 0.1, 0.2, 0.1], np.float32)
    w1 = np.array([0.4, 0.1, 0.3, 0.2], np.float32)
    blocks = [dict(weights=w, certainty=None, num_init=0, num_stored=len(w), prev_ind=0, rule="A", lower_init_weight=False, lr=0.1, floor=0.0) for w in (w0, w1)]
    want = [RN.update(b)["index"] for b in blocks]
    assert want == [3, 1]
    W = [f64_bound.dev(w0), f64_bound.dev(w1)]
    bufs = _row_buffers(n, rows)
    cb = (M.MemBlock * 2)(*[c_block(dict(n=n[b], num_init=0, rule="A", lower=False, floor=0.0), blocks[b], W[b].data_ptr(), None) for b in range(2)])
    cr = (M.MemRow * len(rows))(*[c_row(None if op == RN.SCALAR else src.data_ptr() + 4 * off, mem.ptr(0), elems, block, op, arg)
                                 for (_, elems, op, arg, off, block), (src, mem) in zip(rows, bufs)])
    rec, ws = torch.full((16,), float("nan"), device=DEV), torch.zeros(256, dtype=torch.uint8, device=DEV)
    assert M.lib().pt_mem_update_f32(cb, 2, cr, len(rows), rec.data_ptr(), 3.0, ws.data_ptr(), 256, stream()) == 0
    torch.cuda.synchronize()
    assert rec[:2].tolist() == [3.0, 1.0]
    for (name, elems, op, arg, off, block), (src, mem) in zip(rows, bufs):
        got = mem.host().reshape(n[block], elems)
        s = src[off:off + elems]
        expect = RN.row_value(s.cpu().numpy(), op, arg)
        if op == RN.THRESH:
            assert np.array_equal(expect, (s >= arg).float().cpu().numpy()) and expect[0] == 1 and expect[1] == 0 and expect[2] == 0     # atom.py:599 on the device
        assert np.array_equal(got[want[block]].view(np.uint32), expect.view(np.uint32)), name
        assert np.isnan(np.delete(got, want[block], 0)).all(), name


def _three_updates(W, P, x, rec, ws, name="seqA_n7_i3_f025", first=12):
    """calls first .. first + 2 of a case in a row on the state in W (host state: the reference's)"""
    specs, steps = C.CASES[name]
    seqs, s = C.states(name), C.CASES[name][0][0]
    for j in range(3):
        k = first + j
        blk = (M.MemBlock * 1)(c_block(s, C.block(s, seqs[0][k], steps[k]), W.data_ptr(), None))
        row = (M.MemRow * 1)(c_row(x[j].data_ptr(), P.data_ptr(), x.shape[1], 0))
        assert M.lib().pt_mem_update_f32(blk, 1, row, 1, rec[j].data_ptr(), float(j + 1), ws.data_ptr(), 256, stream()) == 0


def test_repeat_and_graph_replay_give_the_same_bits():
    name, first = "seqA_n7_i3_f025", 12
    g = C.golden(name)
    start = f64_bound.dev(g["before32_0"][first])
    W, P = start.clone(), torch.zeros(7, 1027, device=DEV)
    x = torch.randn(3, 1028, device=DEV)[:, :1027]                             # every source row 16-byte aligned: slot 4 takes the vector path and its tail
    rec, ws = torch.zeros(3, 16, device=DEV), torch.zeros(256, dtype=torch.uint8, device=DEV)
    snap = lambda: (W.clone(), P.clone(), rec.clone())
    reset = lambda: (W.copy_(start), P.zero_(), rec.zero_())
    _three_updates(W, P, x, rec, ws)
    torch.cuda.synchronize()
    one = snap()
    assert rec[:, 0].tolist() == [float(v) for v in g["index_0"][first:first + 3]] == [3.0, 4.0, 5.0]
    assert torch.equal(P[3:6], x) and not P[[0, 1, 2, 6]].any()
    reset()
    _three_updates(W, P, x, rec, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one, snap()))
    reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _three_updates(W, P, x, rec, ws)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one, snap()))


def test_no_wait_path_returns_the_host_index_and_the_record_agrees():
    s = C.spec("A", 7, 3, 0.25)
    st = C.initial(s)
    W, mem = f64_bound.dev(st["weights"]), torch.full((7, 1027), float("nan"), device=DEV)
    x = torch.randn(1, 1027, device=DEV)
    ctx = MU.context(DEV)
    before = ctx.waits
    idx = MU.run([MU.Block(W, 3, 3, None, 0.1, 0.25)], [MU.Row(x, mem)])
    assert idx == [3] and ctx.waits == before                                  # the fill phase: a host value, nothing waited for
    index, floor, total = ctx.wait()
    want = RN.update(C.block(s, st, None))
    assert index[0] == 3 == want["index"] and floor[0] == want["floor"] and abs(total[0] - want["total"]) <= FACTOR * f64_bound.ulp_of_max(want["total"])
    assert torch.equal(mem[3], x[0]) and torch.isnan(mem[[0, 1, 2, 4, 5, 6]]).all()
    with pytest.raises(NotImplementedError):                                   # refused by the library: nothing queued, nothing written
        MU.run([MU.Block(W, 7, 7, None, 0.1, 0.25)], [])
    with pytest.raises(ValueError):
        MU.run([MU.Block(W, 3, 3, None, 0.1, 0.25)], [MU.Row(x, mem[:6])])


@f64_bound.needs_bundle
@pytest.mark.parametrize("name", ["DiMP", "KYS", "ToMP", "DiMPSimple", "TaMOs", "KeepTrack", "ATOM", "LWL", "RTS"])
def test_drop_ins_reproduce_the_whole_method_goldens(name):
    """the drop-in of each class on a bare object on the device against the unmodified method's CPU golden: indices, counters and every
    memory exactly (KeepTrack's certainty is one correctly rounded sqrt either way), the weights within one ulp of the range per call"""
    from oracle import ref_harness
    ref_harness.install()
    import mem_update_methods as MM
    g = dict(np.load(os.path.join(C.GOLDEN_DIR, "mem_update_methods.npz")))
    covered, fast = MU.make(name)
    t = MM.bare(name, DEV)
    for k in range(MM.CALLS):
        args = MM.arguments(name, k, DEV)
        assert covered(t, *args), (name, k)
        assert fast(t, *args) is None
        for key, v in MM.snapshot(t, name).items():
            ref = g[f"{name}.{k}.{key}"]
            if key.startswith("sample_weights"):
                err = float(np.abs(v.astype(np.float64) - ref).max())
                assert err <= FACTOR * (k + 1) * f64_bound.ulp_of_max(ref), (name, k, key, err)
            else:
                assert np.array_equal(v, ref), (name, k, key)
    assert all(isinstance(i, int) for i in t.previous_replace_ind)
