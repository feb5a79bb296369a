"""TEST INFRASTRUCTURE ONLY -- goldens of the trackers' sample-memory update from the UNMODIFIED reference on the CPU (needs the reference
tree):
    python -B tools/make_golden_mem_update.py            tests/golden/mem_update_<case>.npz, tests/golden/mem_update_methods.npz
For every case of tests/mem_update_cases.CASES the reference's own `update_sample_weights` (rule A: DiMP's, B: ATOM's, C: LWL's, D:
KeepTrack's `update_sample_weights_based_on_certainty`) is called on a bare object -- a namespace carrying `params` (and `fparams` for
ATOM) -- over the carried sequence of the case: in fp32 as deployed, in float64 from every fp32 state (call k alone) and in float64 carried
from the start.  The floor decision, which the method does not return, is read off a second call on the same state with a floor of 1e-300 (the arg-min
still starts behind the initial samples, the floor is never applied): the two results differ exactly when the floor was applied.  Keys: tests/mem_update_cases.py.

mem_update_methods.npz: the whole `update_memory` of each of the nine classes (DiMP, KYS, ToMP, DiMPSimple, TaMOs, KeepTrack, ATOM, LWL,
RTS) on a bare object with small memories (tests/mem_update_methods.py builds it), five updates each: every memory, counter and index
behind each call.  From tests/mem_update_cases.py only the table, `initial` and `advance` (the seeded states and the host bookkeeping between
calls) are used; that module imports the numpy restatement for its own `run`, but no function of the restatement is called here."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import mem_update_cases as C  # noqa: E402
import mem_update_methods as MM  # noqa: E402

NEVER = 1e-300              # a floor no sum of weights is below: the arg-min still starts behind the initial samples, the floor is never applied
OUT = os.environ.get("MEM_UPDATE_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))


def reference_call(specs, sts, weights, lr_arg, floor_on=True):
    """one call of the reference method on `weights` (list of torch tensors, updated in place) -> replace_ind"""
    from pytracking import TensorList
    from pytracking.utils import TrackerParams
    rule = specs[0]["rule"]
    assert all(s["rule"] == rule for s in specs)
    floors = [s["floor"] if floor_on or not s["floor"] else NEVER for s in specs]
    p = TrackerParams()
    p.learning_rate, p.lower_init_weight = specs[0]["lr"], specs[0]["lower"]
    if floors[0]:
        p.init_samples_minimum_weight = floors[0]
    me = SimpleNamespace(params=p)
    prevs, stored, inits = [st["prev_ind"] for st in sts], [st["num_stored"] for st in sts], [s["num_init"] for s in specs]
    sw = TensorList(weights)
    if rule == "B":
        from pytracking.tracker.atom.atom import ATOM
        fparams = []
        for s, f in zip(specs, floors):
            fp = SimpleNamespace(learning_rate=s["lr"])
            if f:
                fp.init_samples_minimum_weight = f
            fparams.append(fp)
        return ATOM.update_sample_weights(me, sw, prevs, stored, inits, fparams, lr_arg)
    assert len({(s["lr"], s["floor"], s["lower"]) for s in specs}) == 1        # one `params` serves every block of the call
    if rule == "D":
        from pytracking.tracker.keep_track.keep_track import KeepTrack
        certs = [torch.from_numpy(st["certainty"].copy()).to(w.dtype).view(-1) * w.view(-1) for st, w in zip(sts, weights)]   # keep_track.py:633
        return KeepTrack.update_sample_weights_based_on_certainty(me, certs, sw, prevs, stored, inits, lr_arg)
    if rule == "C":
        from pytracking.tracker.lwl.lwl import LWL
        return LWL.update_sample_weights(me, sw, prevs, stored, inits, lr_arg)
    from pytracking.tracker.dimp.dimp import DiMP
    return DiMP.update_sample_weights(me, sw, prevs, stored, inits, lr_arg)


def call(specs, sts, arrays, lr_arg, dtype):
    """-> (weights behind the call, indices, floor flags) for the weights `arrays` in `dtype`"""
    w = [torch.from_numpy(np.array(a, dtype=np.float64)).to(dtype) for a in arrays]
    idx = reference_call(specs, sts, w, lr_arg)
    plain = [torch.from_numpy(np.array(a, dtype=np.float64)).to(dtype) for a in arrays]
    idx_plain = reference_call(specs, sts, plain, lr_arg, floor_on=False)
    flags = [int(not torch.equal(a, b)) for a, b in zip(w, plain)]
    assert list(idx) == list(idx_plain)
    return [t.numpy() for t in w], [int(i) for i in idx], flags


def case_golden(name):
    specs, steps = C.CASES[name]
    B = len(specs)
    sts32 = [C.initial(s) for s in specs]
    sts64 = [dict(st, weights=st["weights"].astype(np.float64)) for st in sts32]
    g = {f"{k}_{b}": [] for b in range(B) for k in ("before32", "after32", "after64", "carry64", "index", "index64", "floor", "floor64", "cert")}
    for k, lr in enumerate(steps):
        a32, i32, f32 = call(specs, sts32, [st["weights"] for st in sts32], lr, torch.float32)
        a64, i64, f64 = call(specs, sts32, [st["weights"] for st in sts32], lr, torch.float64)
        c64, ic, fc = call(specs, sts64, [st["weights"] for st in sts64], lr, torch.float64)
        assert i32 == i64 and f32 == f64, (name, k, i32, i64, f32, f64)           # call k alone: float64 takes the fp32 run's decisions
        for b, s in enumerate(specs):
            g[f"before32_{b}"].append(sts32[b]["weights"])
            g[f"cert_{b}"].append(sts32[b]["certainty"] if sts32[b]["certainty"] is not None else np.zeros(0, np.float32))
            g[f"after32_{b}"].append(a32[b]); g[f"after64_{b}"].append(a64[b]); g[f"carry64_{b}"].append(c64[b])
            g[f"index_{b}"].append(i32[b]); g[f"index64_{b}"].append(ic[b]); g[f"floor_{b}"].append(f32[b]); g[f"floor64_{b}"].append(fc[b])
            sts32[b] = C.advance(s, sts32[b], i32[b], a32[b], k)
            sts64[b] = C.advance(s, sts64[b], ic[b], c64[b], k)
    return {k: np.array(v) for k, v in g.items()}


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in C.CASES:
        g = case_golden(name)
        np.savez_compressed(os.path.join(OUT, f"mem_update_{name}.npz"), **g)
        T = len(C.CASES[name][1])
        err = max(float(np.abs(g[f"after32_{b}"].astype(np.float64) - g[f"carry64_{b}"]).max()) for b in range(len(C.CASES[name][0])))
        same = all(np.array_equal(g[f"index_{b}"], g[f"index64_{b}"]) and np.array_equal(g[f"floor_{b}"], g[f"floor64_{b}"])
                   for b in range(len(C.CASES[name][0])))
        print(f"{name:24s} T {T:2d} index {g['index_0'].tolist()} floor applied {int(g['floor_0'].sum())}/{T} carried fp32 - float64 {err:.2e} "
              f"same decisions {same}")
    np.savez_compressed(os.path.join(OUT, "mem_update_methods.npz"), **MM.reference_goldens())
    print("methods:", ", ".join(MM.CLASSES))


if __name__ == "__main__":
    main()
