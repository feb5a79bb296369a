"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the trackers' sample-memory update (include/pt_mem.h): the four variants of
`update_sample_weights` (pytracking/tracker/dimp/dimp.py:445-484 A, atom.py:603-639 B, lwl.py:474-516 C, keep_track.py:667-708 D) and the row
operations of `update_memory`.  Written from the reference's statements one by one; `dtype` is the type every statement stores in
(np.float64: the anchor; np.float32: the reference's own arithmetic with numpy's correctly rounded operations and sums in index order).

A block is a dict: weights (n), certainty (n) or None, num_init, num_stored, prev_ind (None or int), rule ('A'..'D'), lower_init_weight,
lr (the resolved Python float), floor (0.0 = none).  `update(block)` leaves the block alone and returns
    weights      the new weights (dtype)
    index        replace index
    floor        1 when the floor was applied
    total        `sw.sum()` in front of the floor test
    head         `sw[:num_init].sum()` of the floor test (None without a floor)
    margins      every discrete decision's distance from flipping: 'argmin' -> relative gap between the chosen key and the runner-up
                 (None: no arg-min ran; 0.0: an exact tie of the keys' float32 bits, resolved to the lowest index), 'floor' -> |head - floor|
                 (None without a floor)
Seeded defects (DEFECTS) are what the CPU test shows the bounds and the table catch."""
import numpy as np

RULES = ("A", "B", "C", "D")
DEFECTS = ("tie_last", "argmin_from_zero", "floor_unnormalised", "floor_divisor", "rule_d_weights", "ignore_lower")
COPY, THRESH, SCALAR = 0, 1, 2


def is_reset(b):
    return b["num_stored"] == 0 or b["lr"] == 1


def host_index(b):
    """the replace index where the reference's index is a host value, else -1"""
    if is_reset(b):
        return 0
    if b["rule"] != "B" and b["num_stored"] < len(b["weights"]):
        return int(b["num_stored"])
    return -1


def keys32(b):
    """the float32 values the reference's torch.min compares (deployed arithmetic)"""
    w = np.asarray(b["weights"], np.float32)
    return (np.asarray(b["certainty"], np.float32) * w).astype(np.float32) if b["rule"] == "D" else w


def update(b, dtype=np.float64, defect=None):
    sw = np.array(b["weights"], dtype=dtype)
    n, num_init, prev, rule, lr = len(sw), int(b["num_init"]), b["prev_ind"], b["rule"], float(b["lr"])
    floor = float(b["floor"]) or None
    s_ind = 0 if floor is None or defect == "argmin_from_zero" else num_init
    margins = {"argmin": None, "floor": None}
    if is_reset(b):
        sw[:] = 0
        sw[0] = 1
        r = 0
    else:
        if rule != "B" and b["num_stored"] < n:
            r = int(b["num_stored"])
        else:
            if rule == "D" and defect != "rule_d_weights":
                key = np.asarray(b["certainty"], dtype) * sw if dtype == np.float64 else keys32(b)
            else:
                key = sw
            cand = key[s_ind:]
            if cand.size == 0:
                raise IndexError("torch.min of an empty tensor")
            lo = cand.min()
            at = np.flatnonzero(cand == lo)
            r = int(at[-1 if defect == "tie_last" else 0]) + s_ind
            if len(at) > 1 or cand.size == 1:
                margins["argmin"] = 0.0 if len(at) > 1 else np.inf
            else:
                second = np.partition(cand, 1)[1]
                margins["argmin"] = float((second - lo) / abs(lo)) if lo != 0 else np.inf
        if prev is None:
            if rule == "C" and b["lower_init_weight"] and defect != "ignore_lower":
                sw[r] = 1
            else:
                sw /= dtype(1 - lr)
                sw[r] = lr
        elif rule == "D" and r == prev:
            pass
        else:
            sw[r] = sw[prev] / dtype(1 - lr)
    unnormalised_head = _sum(sw[:num_init])
    total = _sum(sw)
    sw /= total
    head, applied = None, 0
    if floor is not None:
        head = unnormalised_head if defect == "floor_unnormalised" else _sum(sw[:num_init])
        margins["floor"] = abs(float(head) - floor)
        if head < floor:
            applied = 1
            sw /= dtype(floor + (0.0 if defect == "floor_divisor" else _sum(sw[num_init:])))
            sw[:num_init] = floor / num_init
    return dict(weights=sw, index=r, floor=applied, total=dtype(total), head=head, margins=margins)


def _sum(v):
    """index order in the array's own type (float64: the anchor; float32: one of the orders fp32 hardware may take)"""
    s = v.dtype.type(0)
    for x in v:
        s = s + x
    return s


def row_value(src, op=COPY, arg=0.0):
    """what `update_memory` stores into the slot"""
    if op == SCALAR:
        return np.array([arg], np.float32)
    src = np.asarray(src, np.float32).reshape(-1)
    return (src >= np.float32(arg)).astype(np.float32) if op == THRESH else src.copy()


def insert(memory, index, src, op=COPY, arg=0.0):
    """memory (n, elems) with the slot `index` overwritten; everything else untouched"""
    out = np.array(memory, np.float32)
    out.reshape(out.shape[0], -1)[index] = row_value(src, op, arg)
    return out
