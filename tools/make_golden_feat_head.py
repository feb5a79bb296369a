"""TEST INFRASTRUCTURE ONLY -- tests/golden/feat_head_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_feat_head.py
`residual_bottleneck(num_blocks=0, final_conv=True, l2norm=True, final_stride=2)` (ltr/models/target_classifier/features.py:49-73; the RTS
classifier head, rts_net.py:339-344) in fp32 on every case of synth.FEAT_HEAD_CASES, inputs and weights from synth.feat_head_problem.
Every file holds the shape, the seed, the weight, the output (n, Cout, Ho, Wo) and, up to feat_head_cases.X_STORED_MAX values, the input
(larger inputs are regenerated from the seed by the tests).  `ref_fp32_err` is the largest difference between that fp32 run (8 threads)
and the SAME module in float64; asserted <= 1e-5, a tenth of the 1e-4 the GPU tests hold against these files.  The stride-1 twin of the
first case, `residual_basic_block(num_blocks=0, final_conv=True, l2norm=True)` (features.py:9-28; the LWL / RTS target-model head), must
give the bits of `residual_bottleneck(..., final_stride=1)`: the two constructors build the same two layers."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import feat_head_cases as FC  # noqa: E402
import f64_bound  # noqa: E402
from pytracking_amd import synth  # noqa: E402

OUT = os.environ.get("FEAT_HEAD_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
REF_ERR_MAX = 1e-5


def reference_module(Cin, Cout, w, stride, basic=False):
    import ltr.models.target_classifier.features as rfeat
    if basic:
        net = rfeat.residual_basic_block(feature_dim=Cin, num_blocks=0, l2norm=True, final_conv=True, norm_scale=FC.SCALE, out_dim=Cout)
    else:
        net = rfeat.residual_bottleneck(feature_dim=Cout, num_blocks=0, l2norm=True, final_conv=True, norm_scale=FC.SCALE, out_dim=Cout,
                                        input_dim=Cin, final_stride=stride)
    net.load_state_dict({"0.weight": w.clone()}, strict=True)
    return net.eval()


def main():
    torch.set_num_threads(f64_bound.THREADS)
    for k, (name, (n, Cin, Cout, H, W)) in enumerate(synth.FEAT_HEAD_CASES.items()):
        x, w = FC.problem(name)
        with torch.no_grad():
            out = reference_module(Cin, Cout, w, 2)(x)
            out64 = reference_module(Cin, Cout, w, 2).double()(x.double())
            if k == 0:
                assert torch.equal(reference_module(Cin, Cout, w, 1, basic=True)(x), reference_module(Cin, Cout, w, 1)(x))
        err = float((out.double() - out64).abs().max())
        g = dict(n=n, Cin=Cin, Cout=Cout, H=H, W=W, stride=2, seed=FC.SEED + k, norm_scale=FC.SCALE, eps=FC.EPS, weight=w.numpy(),
                 out=out.numpy(), ref_fp32_err=err, max_abs=float(out.abs().max()))
        if x.numel() <= FC.X_STORED_MAX:
            g["x"] = x.numpy()
        print(f"feat_head_{name}: out {tuple(out.shape)}  ref_fp32_err {err:.3e}  max |v| {g['max_abs']:.3f}")
        assert err <= REF_ERR_MAX, (name, err)
        path = os.path.join(OUT, f"feat_head_{name}.npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) < 200 * 1024, (path, os.path.getsize(path))


if __name__ == "__main__":
    main()
