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
import f64_bound  # noqa: E402
from pytracking_amd import box_encoder as BE  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_enc_f64.txt"))
    os.environ["BOX_ENC_F64_OUT"] = ap.parse_args().out
    table = f64_bound.Table("BOX_ENC_F64_OUT",
                            "Box label encoders on one MI355X against float64, written by tools/report_box_enc_f64.py.\n"
                            "Per case and output: the largest |gpu - float64 stand-in|, ref_err = the fp32 CPU stand-in's own distance from float64\n"
                            f"on that case ({BC.THREADS} threads), floor = one fp32 ulp of the output's range, ratio = err / max(ref_err, floor); bound\n"
                            f"{f64_bound.FACTOR} (tests/f64_bound.py).")
    for kind, name in BC.ALL:
        _, c, _, boxes, feat = BC.case(kind, name)
        net = BC.module(kind, name, DEV)
        with torch.no_grad():
            out = BE.forward(net, *BC.call_args(kind, c, boxes, feat, DEV))
        out = out if kind == BC.BOX else (out,)
        an = BC.anchor(kind, name)
        f64_bound.held(f"{kind}_{name}", {q: out[k] for k, q in enumerate(BC.outputs(kind, c))}, an.want, an.ref_err,
                       floor=f64_bound.spacing_of_max(an.want), table=table)


if __name__ == "__main__":
    main()
