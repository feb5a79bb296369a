"""TEST INFRASTRUCTURE ONLY -- tests/golden/iou_mod_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_iou_mod.py
AtomIoUNet.get_modulation (ltr/models/bbreg/atom_iou_net.py:138-170) on synth.iou_mod_state / synth.iou_mod_inputs for every case of
synth.IOU_MOD_CASES.  The module is the reference's AtomIoUNet; for channel counts its constructor does not offer, the five
reference-branch blocks are rebuilt with the reference's own `conv()` helper (atom_iou_net.py:7-12).

PrRoIPool is PARITY-UNPINNED: the reference vendors it as a submodule that is empty in the snapshot, so oracle/ref_harness.install()
provides oracle/prroi_torch.py, the restatement of the published definition (self-pinned by tests/test_oracle_prroi.py).  The goldens pin
everything around the pooling -- the five blocks, the RoI construction, the concatenation -- and the pooling only as far as that
restatement goes.

The outputs are tiny (n x (P3 + P4) values), so every file holds all of them, deployed cases included:
  seeds, dims, `boxes`            what regenerates state and inputs (synth.iou_mod_state / iou_mod_inputs)
  `out3`, `out4`                  the reference's fp32 outputs
  `out3_f64`, `out4_f64`          the same module run with .double() on the same inputs
  `ref_fp32_err`                  their largest distance, taken with torch.set_num_threads(f64_bound.THREADS); asserted <= 2.5e-5, a
                                  quarter of the flat 1e-4 the GPU tests hold against these files next to the float64 bound."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

from pytracking_amd import synth  # noqa: E402
import f64_bound  # noqa: E402

OUT = os.environ.get("IOU_MOD_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
STATE_SEED, INPUT_SEED = 2600, 2700
REF_ERR_MAX = 2.5e-5
BLOCKS = ("conv3_1r", "conv4_1r", "fc3_1r", "fc34_3r", "fc34_4r")


def reference_module(cin3, cin4, dims, sd):
    from ltr.models.bbreg import atom_iou_net as M
    A, B, D, P3, P4 = dims
    net = M.AtomIoUNet(input_dim=(cin3, cin4), pred_input_dim=(P3, P4))
    net.conv3_1r, net.conv4_1r = M.conv(cin3, A, kernel_size=3, stride=1), M.conv(cin4, D, kernel_size=3, stride=1)
    net.fc3_1r = M.conv(A, B, kernel_size=3, stride=1, padding=0)
    net.fc34_3r = M.conv(B + D, P3, kernel_size=1, stride=1, padding=0)
    net.fc34_4r = M.conv(B + D, P4, kernel_size=1, stride=1, padding=0)
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and not [k for k in missing if k.split(".")[0] in BLOCKS]
    return net.eval()


def main():
    torch.set_num_threads(f64_bound.THREADS)
    for k, (name, (n, (cin3, h3, w3), (cin4, h4, w4), dims)) in enumerate(synth.IOU_MOD_CASES.items()):
        sseed, iseed = STATE_SEED + k, INPUT_SEED + k
        sd = synth.iou_mod_state(sseed, cin3, cin4, *dims)
        f3, f4, bb = synth.iou_mod_inputs(iseed, name)
        net = reference_module(cin3, cin4, dims, sd)
        with torch.no_grad():
            o3, o4 = [t.numpy().reshape(n, -1) for t in net.get_modulation([torch.from_numpy(f3), torch.from_numpy(f4)], torch.from_numpy(bb))]
            net = net.double()
            d3, d4 = [t.numpy().reshape(n, -1) for t in net.get_modulation([torch.from_numpy(f3).double(), torch.from_numpy(f4).double()],
                                                                          torch.from_numpy(bb).double())]
        assert o3.dtype == np.float32 and d3.dtype == np.float64 and o3.shape == (n, dims[3]) and o4.shape == (n, dims[4])
        err = max(float(np.abs(o3 - d3).max()), float(np.abs(o4 - d4).max()))
        g = dict(state_seed=sseed, input_seed=iseed, n=n, level3=np.array((cin3, h3, w3)), level4=np.array((cin4, h4, w4)), dims=np.array(dims),
                 boxes=bb, out3=o3, out4=o4, out3_f64=d3, out4_f64=d4, ref_fp32_err=err,
                 max_abs=max(float(np.abs(d3).max()), float(np.abs(d4).max())))
        print(f"iou_mod_{name}: ref_fp32_err {err:.3e}  max |v| {g['max_abs']:.3f}  zeros {float((d3 == 0).mean()):.2f} / {float((d4 == 0).mean()):.2f}")
        assert err <= REF_ERR_MAX, (name, err)
        np.savez_compressed(os.path.join(OUT, f"iou_mod_{name}.npz"), **g)


if __name__ == "__main__":
    main()
