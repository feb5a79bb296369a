"""The float64 anchor of the ToMP model predictor cases of tests/tomp_cases.py, shared by tests/test_tomp_routes_cpu.py and
tests/test_gpu_tomp_routes.py.  For a case the numpy oracle (oracle/tomp_oracle.py, dtype-generic) runs once in float64 (`want`, per
output) and once in fp32; `ref_err` is the largest |fp32 - float64| over the outputs of a group: what fp32 arithmetic costs on this very
case in an order of summation nobody tuned.  A device output is held to bound(ref_err) = F x its group's ref_err of `want`.  The groups
are the predictor's own outputs (filters and encoded features, magnitude 3 to 6), the classifier's scores (a D-term dot product of
the two, magnitude up to 70: its fp32 error is ten to twenty times the predictor's) and the regressor's boxes; one ref_err over all of
them would hold the filters to the scores' error.

numpy's BLAS blocks its sums by the thread count, so ref_err moves with the machine: tomp_cases.REF_ERR carries the values measured where
the table was written, the CPU test holds the recomputed value to [0.5, 2] x the committed one, and the GPU test uses the committed one.

The anchor, the bound and the report are those of tests/f64_bound.py.  F starts from its FACTOR and is defined here and nowhere else.
The predictor's device error was measured against ref_err on the MI355X (profiles/tomp_routes_f64.txt): where every case stays at or
below half of FACTOR x ref_err, F is FACTOR; otherwise twice the worst measured ratio, rounded up (the 2 covers the tens of per cent by which ref_err itself moves with the
summation blocking), and never above F_MAX = 32 -- the weakest seeded defect of tests/test_tomp_routes_cpu.py, a LayerNorm eps of 2e-5,
still has to fail by a wide margin.

`python tests/tomp_f64.py` prints the ROUTES_TEXT and REF_ERR tables of tests/tomp_cases.py from the built library and this CPU.
Reads nothing outside the repository.  Test infrastructure only."""
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f64_bound                               # noqa: E402
import tomp_cases as TC                        # noqa: E402
from oracle import tomp_oracle as TO           # noqa: E402

F_MAX = 32
# The largest max |MI355X - float64| / ref_err over every output of every case (profiles/tomp_routes_f64.txt: the scores of swz_pad_532;
# fifteen more outputs between 2.0 and 2.9, spread over the D = 128 ... 512 cases, none apart from the rest).  Above FACTOR / 2 = 2, so
# F is twice it, rounded up.
WORST_MEASURED = 2.98
F = f64_bound.raised_factor(WORST_MEASURED, F_MAX)
REF_ERR_BAND = (0.5, 2.0)                     # recomputed ref_err / committed ref_err the CPU test accepts

PREDICTOR = ("cls_filter", "bbreg_filter", "cls_enc", "bbreg_enc", "filter", "enc")


def bound(ref_err):
    return f64_bound.bound(ref_err, F)


def group(output):
    return "predictor" if output in PREDICTOR else output


def predict_outputs(cfg, params, inputs, dtype, gth=None, feature_sz=None):
    """One oracle run of a predictor case in `dtype` -> OrderedDict {output: array}.  gth / feature_sz override the case's own (the seeded
    defects of the CPU test)."""
    p = {k: v.astype(dtype) for k, v in params.items()}
    tr, te, lb, lt = [a.astype(dtype) for a in inputs]
    a = (cfg["nhead"], cfg["n_enc"], cfg["n_dec"], cfg["feature_sz"] if feature_sz is None else feature_sz)
    if cfg["mode"] == "parallel":
        g = cfg["num_gth_frames"] if gth is None else gth
        cw, bw, cenc, benc = TO.predict_cls_bbreg_filters_parallel(p, tr, te, lb, g, lt, *a)
        return OrderedDict((("cls_filter", cw), ("bbreg_filter", bw), ("cls_enc", cenc), ("bbreg_enc", benc),
                            ("scores", TO.linear_filter_classifier(p, cenc, cw)), ("ltrb", TO.dense_box_regressor(p, benc, bw))))
    w, enc = TO.predict_filter(p, tr, te, lb, lt, *a)
    return OrderedDict((("filter", w), ("enc", enc)))


def bbreg_outputs(params, feat, filt, dtype):
    return OrderedDict(ltrb=TO.dense_box_regressor({k: v.astype(dtype) for k, v in params.items()}, feat.astype(dtype), filt.astype(dtype)))


def linear_outputs(w, b, x, relu, dtype):
    y = x.astype(dtype) @ w.astype(dtype).T
    if b is not None:
        y = y + b.astype(dtype)
    return OrderedDict(y=np.maximum(y, 0) if relu else y)


def outputs(kind, name, dtype):
    if kind == "predict":
        cfg, params, inputs = TC.predict_case(name)
        return predict_outputs(cfg, params, inputs, dtype)
    if kind == "bbreg":
        _, _, _, _, params, feat, filt = TC.bbreg_case(name)
        return bbreg_outputs(params, feat, filt, dtype)
    _, _, _, _, relu, w, b, x = TC.linear_case(name)
    return linear_outputs(w, b, x, relu, dtype)


def anchor(kind, name):
    """want, the fp32 oracle run and its distance from want per group, computed once per session."""
    return f64_bound.anchor(("tomp", kind, name), lambda dtype: outputs(kind, name, dtype), group)


TABLES = (("predict", TC.PREDICT), ("bbreg", TC.BBREG), ("linear", TC.LINEAR))


def _main():
    from pytracking_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    print("ROUTES_TEXT = {")
    for name in TC.PREDICT:
        rc, r = TC.case_routes(L, name)
        assert rc == 0, (name, rc)
        print(f'    "{name}": "{TC.compress(r)}",')
    for name, (n, D, H, W) in TC.BBREG.items():
        rc, r = TC.bbreg_routes(L, n, D, H, W)
        assert rc == 0, (name, rc)
        print(f'    "{name}": "{TC.compress(r)}",')
    for name, (B, N, K, _, _) in TC.LINEAR.items():
        rc, r = TC.linear_routes(L, B, N, K)
        assert rc == 0, (name, rc)
        print(f'    "{name}": "{TC.compress(r)}",')
    print("}\nREF_ERR = {")
    for kind, table in TABLES:
        for name in table:
            print(f'    "{name}": {{' + ", ".join(f'"{g}": {r:.3e}' for g, r in anchor(kind, name).ref_err.items()) + "},", flush=True)
    print("}")


if __name__ == "__main__":
    _main()
