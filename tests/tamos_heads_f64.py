"""The float64 anchor of the cases of tests/tamos_heads_cases.py, shared by tests/test_tamos_heads_cpu.py and tests/test_gpu_tamos_heads.py,
built like tests/tamos_f64.py.  For a case the numpy restatement (tests/tamos_heads_np.py) runs once in float64 (`want`) and once in fp32;
`ref_err` is the largest |fp32 - float64| over the case's outputs.  A device output is held to F x ref_err.

numpy's BLAS blocks its sums by the thread count, so ref_err moves with the machine: tamos_heads_cases.REF_ERR carries the values measured
where the table was written, the CPU test holds the recomputed value to [0.5, 2] x the committed one, and the GPU test uses the committed one.

The anchor, the bound and the report are those of tests/f64_bound.py; F starts from its FACTOR.  After the MI355X run every ratio is in
profiles/tamos_heads_f64.txt; where the worst is at most FACTOR / 2, F stays FACTOR, otherwise ceil(2 x worst), and never above F_MAX: the weakest seeded defect of
tests/test_tamos_heads_cpu.py has to fail (see F_MAX below).

`python tests/tamos_heads_f64.py` prints the ROUTES_TEXT and REF_ERR tables of tests/tamos_heads_cases.py from the built library and this CPU.
Reads nothing outside the repository.  Test infrastructure only."""
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f64_bound                               # noqa: E402
import tamos_heads_cases as HC                 # noqa: E402
import tamos_heads_np as HN                    # noqa: E402

# The weakest seeded defect, a GroupNorm eps of 2e-5, sits at 16 x ref_err on reg_d128_9x13_t1 (28 - 98 x on the other small cases; the
# halo, statistics-without-bias and nearest-`round` defects are four orders of magnitude above): F_MAX = 8 keeps every one failing.
F_MAX = 8
# The largest max |MI355X - float64| / ref_err over every output of every case (profiles/tamos_heads_f64.txt: feat2 of fpn_x2; the FPN's
# high-resolution map sits at 3.4 - 4.0 everywhere, the regressor at 1.3 - 2.5).  Above FACTOR / 2 = 2, so F is twice it, rounded up.
WORST_MEASURED = 3.96
F = f64_bound.raised_factor(WORST_MEASURED, F_MAX)
REF_ERR_BAND = (0.5, 2.0)
# defect -> the small cases on which it has to exceed F_MAX x ref_err
DEFECT_CASES = {"gn_eps": HC.SMALL_REG, "halo": HC.SMALL_REG, "stats_nobias": HC.SMALL_REG, "nearest_round": HC.SMALL_FPN}


def outputs(name, dtype, defect=None):
    """One run of the restatement in `dtype` -> OrderedDict {output: array}"""
    if name in HC.REG:
        p, feat, filt = HC.reg_case(name)
        return OrderedDict(ltrb=HN.regressor({k: v.astype(dtype) for k, v in p.items()}, feat.astype(dtype), filt.astype(dtype), defect))
    if name in HC.FPN:
        p, hi, lo = HC.fpn_case(name)
        f2, f3 = HN.fpn({k: v.astype(dtype) for k, v in p.items()}, hi.astype(dtype), lo.astype(dtype), defect)
        return OrderedDict(feat2=f2, feat3=f3)
    fname, rp, filt = HC.chain_case(name)
    p, hi, lo = HC.fpn_case(fname)
    f2, _ = HN.fpn({k: v.astype(dtype) for k, v in p.items()}, hi.astype(dtype), lo.astype(dtype), defect)
    return OrderedDict(feat2=f2, ltrb=HN.regressor({k: v.astype(dtype) for k, v in rp.items()}, f2, filt.astype(dtype), defect))


def anchor(name):
    return f64_bound.anchor(("tamos_heads", name), lambda dtype: outputs(name, dtype))


def _main():
    from pytracking_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    print("ROUTES_TEXT = {")
    for name in list(HC.REG) + list(HC.FPN):
        rc, r = HC.case_routes(L, name)
        assert rc == 0, (name, rc)
        print(f'    "{name}": "{HC.compress(r)}",')
    print("}\nREF_ERR = {")
    for name in list(HC.REG) + list(HC.FPN) + list(HC.CHAIN):
        print(f'    "{name}": {anchor(name).ref_err:.3e},', flush=True)
    print("}")
    for defect, cases in DEFECT_CASES.items():
        for name in cases:
            e = max(f64_bound.errors(anchor(name).want, outputs(name, np.float32, defect)).values())
            print(f"defect {defect:14s} {name:22s} {e:.3e} = {e / anchor(name).ref_err:7.1f} x ref_err", flush=True)


if __name__ == "__main__":
    _main()
