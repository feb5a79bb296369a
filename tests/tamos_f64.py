"""The float64 anchor of the TaMOs cases of tests/tamos_cases.py, shared by tests/test_tamos_cpu.py and tests/test_gpu_tamos.py, built
like tests/tomp_f64.py.  For a case the numpy restatement (tests/tamos_np.py) runs once in float64 (`want`) and once in fp32; `ref_err`
is the largest |fp32 - float64| over the outputs of a group -- the predictor's own outputs (filters and encoded maps) and the
classifier's scores, whose D-term dot products carry ten times the predictor's error.  A device output is held to F x its group's ref_err.

numpy's BLAS blocks its sums by the thread count, so ref_err moves with the machine: tamos_cases.REF_ERR carries the values measured where
the table was written, the CPU test holds the recomputed value to [0.5, 2] x the committed one, and the GPU test uses the committed one.

The anchor, the bound and the report are those of tests/f64_bound.py; F starts from its FACTOR.  After the MI355X run every ratio is in
profiles/tamos_f64.txt; where the worst is at most FACTOR / 2, F stays FACTOR, otherwise ceil(2 x worst), and never above F_MAX = 8: the weakest seeded defect of
tests/test_tamos_cpu.py, a LayerNorm eps of 2e-5, sits at 8 - 13 x ref_err and has to fail.

`python tests/tamos_f64.py` prints the ROUTES_TEXT and REF_ERR tables of tests/tamos_cases.py from the built library and this CPU.
Reads nothing outside the repository.  Test infrastructure only."""
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f64_bound                               # noqa: E402
import tamos_cases as TC                       # noqa: E402
import tamos_np as TN                          # noqa: E402

F_MAX = 8
# The largest max |MI355X - float64| / ref_err over every output of every case (profiles/tamos_f64.txt: the filters of mask9_gth0; three more
# outputs at 2.8 - 2.9, all on D >= 256).  Above FACTOR / 2 = 2, so F is twice it, rounded up.
WORST_MEASURED = 3.13
F = f64_bound.raised_factor(WORST_MEASURED, F_MAX)
REF_ERR_BAND = (0.5, 2.0)

PREDICTOR = ("cls_filter", "bbreg_filter", "cls_enc", "bbreg_enc", "filter", "enc")


def bound(ref_err):
    return f64_bound.bound(ref_err, F)


def group(output):
    return "predictor" if output in PREDICTOR else "scores"


def outputs(name, dtype, defect=None):
    """One run of the restatement in `dtype` -> OrderedDict {output: array}: the predictor's outputs in the mirror's shapes, then the
    classifier's T score maps per sequence on the (classification) encoded map."""
    cfg, params, inputs = TC.case(name)
    p = {k: v.astype(dtype) for k, v in params.items()}
    tr, te, lb, lt = [a.astype(dtype) for a in inputs]
    a = (cfg["nhead"], cfg["n_enc"], cfg["n_dec"], cfg["feature_sz"])
    if cfg["mode"] == "parallel":
        cw, bw, cenc, benc = TN.predict_cls_bbreg_filters_parallel(p, tr, te, lb, cfg["num_gth_frames"], lt, *a, defect=defect)
        return OrderedDict((("cls_filter", cw[None]), ("bbreg_filter", bw[None]), ("cls_enc", cenc), ("bbreg_enc", benc),
                            ("scores", TN.classifier_scores(p, cenc, cw[None]))))
    w, enc = TN.predict_filter(p, tr, te, lb, lt, *a, defect=defect)
    return OrderedDict((("filter", w), ("enc", enc), ("scores", TN.classifier_scores(p, enc, w))))


def anchor(name):
    return f64_bound.anchor(("tamos", name), lambda dtype: outputs(name, dtype), group)


def _main():
    from pytracking_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    print("ROUTES_TEXT = {")
    for name in TC.CASES:
        rc, r = TC.case_routes(L, name)
        assert rc == 0, (name, rc)
        print(f'    "{name}": "{TC.compress(r)}",')
    print("}\nREF_ERR = {")
    for name in TC.CASES:
        print(f'    "{name}": {{' + ", ".join(f'"{g}": {r:.3e}' for g, r in anchor(name).ref_err.items()) + "},", flush=True)
    print("}")


if __name__ == "__main__":
    _main()
