"""profiles/box_enc_f64.txt: the box label encoders on one MI355X against float64, per case and output the largest |gpu - float64 stand-in|
as a multiple of ref_err -- the figures tests/test_gpu_box_enc.py::test_matches_float64_and_golden prints before it asserts.
    python -B tools/report_box_enc_f64.py [--out profiles/box_enc_f64.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import box_enc_cases as BC  # noqa: E402
import fused_f64 as F64  # noqa: E402
from pytracking_amd import box_encoder as BE  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_enc_f64.txt"))
    a = ap.parse_args()
    rows, worst = [], (0.0, "")
    for kind, name in BC.ALL:
        _, c, _, boxes, feat = BC.case(kind, name)
        net = BC.module(kind, name, DEV)
        with torch.no_grad():
            out = BE.forward(net, *BC.call_args(kind, c, boxes, feat, DEV))
        out = out if kind == BC.BOX else (out,)
        got = {q: out[k].cpu().numpy() for k, q in enumerate(BC.outputs(kind, c))}
        an = BC.anchor(kind, name)
        errs = BC.errors(an.want, got)
        ulp = BC.ulp_of_range(an.want)
        cells = [f"{errs[q]:.3e} ({errs[q] / an.ref_err:.2f}x)" if q in errs else "-" for q in ("label_enc", "sample_w")]
        rows.append(f"{kind + '_' + name:<24} {cells[0]:<20} {cells[1]:<20} {an.ref_err:.3e}   {F64.FACTOR * max(an.ref_err, ulp):.3e}"
                    + ("  (one ulp of the range x FACTOR)" if ulp > an.ref_err else ""))
        if ulp <= an.ref_err:
            worst = max(worst, (max(errs.values()) / an.ref_err, f"{kind}_{name}"))
    text = ("Box label encoders on one MI355X against float64, written by tools/report_box_enc_f64.py.\n"
            "Per case: the largest |gpu - float64 stand-in| per output as a multiple of ref_err, the fp32 CPU stand-in's own distance from\n"
            f"float64 on that case ({BC.THREADS} threads).  Bound: FACTOR x max(ref_err, one fp32 ulp of the output's range), FACTOR = {F64.FACTOR}\n"
            f"(tests/fused_f64.py).  Worst multiple where ref_err sets the bound: {worst[0]:.2f} ({worst[1]}).\n\n"
            f"{'case':<24} {'label_enc':<20} {'sample_w':<20} ref_err     bound\n" + "\n".join(rows) + "\n")
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
