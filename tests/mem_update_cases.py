"""TEST INFRASTRUCTURE ONLY -- the case table of the sample-memory update (include/pt_mem.h): the smallest shapes at which the kernels can
still go wrong, as carried sequences of updates.  A case is a list of block specs (one entry of the tracker's `sample_weights` each) and a
list of steps; a step is the `learning_rate` argument of that call (None: the default of the block).  The tools/make_golden_mem_update.py
goldens hold, per case and block, what the UNMODIFIED reference made of it (tests/golden/mem_update_<case>.npz):
    before32 (T, n)   the fp32 run's weights in front of call k             cert (T, n)   rule D: the certainties in front of call k
    after32  (T, n)   ... behind it                                         index (T)     replace index (fp32 run)
    after64  (T, n)   the float64 run of call k alone, started from before32[k]
    carry64  (T, n)   the float64 run carried from the start                index64 (T), floor64 (T)   its decisions
    floor (T)         1 where the floor was applied (fp32 run)
keys are suffixed with the block number.  numpy only; the restatement is tests/mem_update_np.py."""
import os
from collections import OrderedDict

import numpy as np

import mem_update_np as RN

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LRS12 = [None, 0.2, None, None, 0.3, None, None, None, 0.2, None, None, None]
LRS36 = LRS12 * 3
LRS_HN = [None, 0.02, None, 0.3, None, 0.2]


def spec(rule, n, num_init, floor=0.0, lr=0.1, lower=False, start="init", prev=None, seed=0):
    """start: 'init' -- the state behind init_memory (num_init weights of 1 / num_init, num_stored = num_init, no previous index);
    'full' -- a full memory of seeded weights, previous index `prev`; 'empty' -- nothing stored"""
    return dict(rule=rule, n=n, num_init=num_init, floor=floor, lr=lr, lower=lower, start=start, prev=prev, seed=seed)


CASES = OrderedDict([
    # 36 carried updates: the fill phase, the full memory, the floor
    ("seqA_n7_i3_f025", ([spec("A", 7, 3, 0.25)], LRS36)),
    ("seqA_n7_i3_f06", ([spec("A", 7, 3, 0.6)], LRS36)),
    ("seqA_n4_i1_f025", ([spec("A", 4, 1, 0.25)], LRS36)),
    ("seqA_n33_i13_f05", ([spec("A", 33, 13, 0.5)], LRS36)),
    ("seqB_n7_i3_f025", ([spec("B", 7, 3, 0.25)], LRS36)),                  # fills the memory through its zero ties
    ("seqB_n33_i13", ([spec("B", 33, 13)], LRS36)),
    ("seqC_n7_i3_f025_lower", ([spec("C", 7, 3, 0.25, lower=True)], LRS36)),
    ("seqC_n4_i1_f06", ([spec("C", 4, 1, 0.6)], LRS36)),
    ("seqD_n7_i3_f025", ([spec("D", 7, 3, 0.25, seed=3)], LRS36)),          # certainty of the written slot updated between calls
    ("seqD_n33_i13_f06", ([spec("D", 33, 13, 0.6, seed=4)], LRS36)),
    # sizes, num_init 0 / 1 / n - 1 / n, the reset
    ("a_n1_full", ([spec("A", 1, 1, start="full")], [None, 0.2, None])),
    ("a_n1_empty", ([spec("A", 1, 0, start="empty")], [None, None, 0.3])),
    ("a_n2_i1_f025", ([spec("A", 2, 1, 0.25)], LRS_HN)),
    ("a_n7_empty", ([spec("A", 7, 0, start="empty")], LRS12[:10])),
    ("a_n7_lr1", ([spec("A", 7, 3, 0.25)], [None, None, 1.0, None, 0.2, 1.0, None])),
    ("a_n33_i32_f06", ([spec("A", 33, 32, 0.6)], [None, 0.3, None, None])),
    ("a_n33_i33", ([spec("A", 33, 33, start="full", prev=5, seed=5)], [None, 0.02, None])),
    ("b_n250_i13_f025", ([spec("B", 250, 13, 0.25, lr=0.01)], [None, 0.2, None])),
    ("b_n250_i250_full", ([spec("B", 250, 250, start="full", prev=17, seed=6)], [None, 0.3, None])),
    ("b_n4_lr1", ([spec("B", 4, 1, 0.25)], [None, 1.0, None])),
    ("c_n2_lower", ([spec("C", 2, 1, lower=True)], [None, None, 0.2])),
    ("c_n32_i1", ([spec("C", 32, 1, lower=True)], LRS12[:6])),
    ("c_n1024_i1", ([spec("C", 1024, 1, 0.25)], [None, 0.2])),
    ("a_n1024_full_f025", ([spec("A", 1024, 13, 0.25, start="full", prev=None, seed=7)], [None, None, 0.02])),
    ("a_n1024_full_prev", ([spec("A", 1024, 3, start="full", prev=1000, seed=8)], [None, 0.2])),
    ("d_n1024_full_f06", ([spec("D", 1024, 3, 0.6, start="full", prev=700, seed=9)], [None, None, 0.3])),
    ("d_n250_full", ([spec("D", 250, 13, start="full", prev=None, seed=10)], [None, None, None, 0.2])),
    ("d_n2_i1_f025", ([spec("D", 2, 1, 0.25, seed=11)], LRS_HN)),
    # two entries of `sample_weights` with different n in one call
    ("two_a_n4_n33", ([spec("A", 4, 1, 0.25), spec("A", 33, 13, 0.25)], LRS_HN)),
    ("two_b_n7_n250", ([spec("B", 7, 3, 0.25), spec("B", 250, 13, lr=0.2, start="full", prev=3, seed=12)], LRS_HN)),
])

# Refusals of pt_mem_update_f32 ("unsupported", nothing queued): (what, block overrides)
REFUSALS = (("n above the limit", dict(n=1025)), ("no weight", dict(n=0)), ("num_init above n", dict(n=7, num_init=8)),
            ("floor, num_init == n, full memory", dict(n=7, num_init=7, num_stored=7, floor=0.25)),
            ("floor, num_init == n, rule B", dict(n=7, num_init=7, num_stored=7, floor=0.25, rule="B")),
            ("floor without initial samples", dict(n=7, num_init=0, num_stored=2, floor=0.25)),
            ("unknown rule", dict(rule=4)), ("rule D without certainties", dict(rule="D")))

# Rows of k_mem_insert: (name, elems, op, arg, src offset in floats inside a larger tensor, block)
ROWS = (("e1", 1, RN.COPY, 0.0, 0, 0), ("e4", 4, RN.COPY, 0.0, 0, 0), ("e5_odd_slot", 5, RN.COPY, 0.0, 0, 0), ("e255", 255, RN.COPY, 0.0, 0, 0),
        ("e1027", 1027, RN.COPY, 0.0, 0, 0), ("e2304", 64 * 6 * 6, RN.COPY, 0.0, 0, 0), ("e2304_slice", 64 * 6 * 6, RN.COPY, 0.0, 2 * 64 * 6 * 6, 0),
        ("e1027_src_off1", 1027, RN.COPY, 0.0, 1, 0), ("thresh_e324", 18 * 18, RN.THRESH, 0.05, 0, 0), ("thresh_e5", 5, RN.THRESH, 0.0, 3, 1),
        ("scalar", 1, RN.SCALAR, 0.625, 0, 0), ("e4_second_block", 4, RN.COPY, 0.0, 0, 1), ("deployed_512x18x18", 512 * 18 * 18, RN.COPY, 0.0, 0, 0))


def initial(s):
    """the block state in front of the first call: dict(weights fp32, certainty fp32 or None, num_stored, prev_ind)"""
    rng = np.random.default_rng(1000 + s["seed"])
    n = s["n"]
    w = np.zeros(n, np.float32)
    if s["start"] == "init":
        w[:s["num_init"]] = np.float32(1.0) / np.float32(s["num_init"])
        stored, prev = s["num_init"], None
    elif s["start"] == "full":
        v = rng.uniform(0.5, 1.5, n)
        w[:] = (v / v.sum()).astype(np.float32)
        stored, prev = n, s["prev"]
    else:
        stored, prev = 0, None
    cert = rng.uniform(0.2, 1.0, n).astype(np.float32) if s["rule"] == "D" else None
    return dict(weights=w, certainty=cert, num_stored=stored, prev_ind=prev)


def step_certainty(s, k):
    """rule D: the certainty the tracker stores into the written slot behind call k; every sixth one is low enough for the next arg-min to
    come back to that slot once (r_ind == prev_ind).  Not more often: a run of such calls leaves the weights alone, and the sum of the initial
    weights then converges to the floor from below -- the reference's own floor test becomes a near tie (margin / 16 per call)"""
    return np.float32(0.02) if k % 6 == 1 else np.float32(np.random.default_rng(7000 + 100 * s["seed"] + k).uniform(0.6, 1.0))


def block(s, state, lr_arg, weights=None, dtype=None):
    """the restatement's block of a spec, a state and the call's learning_rate argument"""
    w = state["weights"] if weights is None else weights
    return dict(weights=w if dtype is None else np.asarray(w, dtype), certainty=state["certainty"], num_init=s["num_init"], num_stored=state["num_stored"],
                prev_ind=state["prev_ind"], rule=s["rule"], lower_init_weight=s["lower"], lr=s["lr"] if lr_arg is None else lr_arg, floor=s["floor"])


def advance(s, state, index, weights, k):
    """the state behind call k: what `update_memory` does around `update_sample_weights` (lwl.py:471 saturates the counter)"""
    cert = state["certainty"]
    if cert is not None:
        cert = cert.copy()
        cert[index] = step_certainty(s, k)
    stored = state["num_stored"]
    stored = (stored + 1 if stored < s["n"] else stored) if s["rule"] == "C" else stored + 1
    return dict(weights=weights, certainty=cert, num_stored=stored, prev_ind=int(index))


_GOLDEN, _RUNS = {}, {}


def golden(name):
    if name not in _GOLDEN:
        with np.load(os.path.join(GOLDEN_DIR, f"mem_update_{name}.npz")) as z:
            _GOLDEN[name] = {k: z[k] for k in z.files}
    return _GOLDEN[name]


def states(name):
    """per block the list of states in front of every call, on the reference's fp32 trajectory (weights from the golden, the host state from
    the golden's decisions)"""
    specs, steps = CASES[name]
    g = golden(name)
    out = []
    for b, s in enumerate(specs):
        st, seq = initial(s), []
        for k in range(len(steps)):
            st = dict(st, weights=g[f"before32_{b}"][k])
            seq.append(st)
            st = advance(s, st, int(g[f"index_{b}"][k]), g[f"after32_{b}"][k], k)
        out.append(seq)
    return out


def run(name, defect=None):
    """the float64 restatement of every call of a case, each started from the reference's fp32 state: [step][block] -> update() result"""
    key = (name, defect)
    if key not in _RUNS:
        specs, steps = CASES[name]
        seqs = states(name)
        _RUNS[key] = [[RN.update(block(s, seqs[b][k], lr, dtype=np.float64), np.float64, defect) for b, s in enumerate(specs)]
                      for k, lr in enumerate(steps)]
    return _RUNS[key]


def carried(name, dtype=np.float64):
    """the restatement carried from the first state in `dtype`: [step][block] -> update() result"""
    specs, steps = CASES[name]
    sts = [initial(s) for s in specs]
    out = []
    for k, lr in enumerate(steps):
        row = []
        for b, s in enumerate(specs):
            r = RN.update(block(s, sts[b], lr, dtype=dtype), dtype)
            sts[b] = advance(s, sts[b], r["index"], r["weights"], k)
            row.append(r)
        out.append(row)
    return out


def ref_err(name, b, k):
    """the unmodified reference's fp32 distance from its own float64 run of call k of block b"""
    g = golden(name)
    return float(np.abs(g[f"after32_{b}"][k].astype(np.float64) - g[f"after64_{b}"][k]).max())


def ref_err_carried(name, b, k):
    g = golden(name)
    return float(np.abs(g[f"after32_{b}"][k].astype(np.float64) - g[f"carry64_{b}"][k]).max())
