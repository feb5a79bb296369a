"""TEST INFRASTRUCTURE ONLY -- tests/golden/iou_feat_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_iou_feat.py
AtomIoUNet.get_iou_feat (ltr/models/bbreg/atom_iou_net.py:172-179) on synth.iou_feat_state / synth.iou_feat_inputs for every case of
synth.IOU_FEAT_CASES.  The module is the reference's AtomIoUNet; for channel counts its constructor does not offer, the four test-branch
blocks are rebuilt with the reference's own `conv()` helper (atom_iou_net.py:7-12).
  small cases      seeds + shape + the reference's full fp32 outputs `c3`, `c4`
  deployed cases   seeds + shape + a fixed 2000-entry sample of each output (`idx3`, `c3`, `idx4`, `c4`): a deployed weight set is too
                   large to commit, the GPU box regenerates state and inputs from the seeds
  every case       `ref_fp32_err`: the largest difference between the reference's own fp32 output and the float64 restatement
                   (tests/iou_feat_np.py); asserted <= 2.5e-5, a quarter of the 1e-4 bound the GPU tests hold against these files."""
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
import iou_feat_np  # noqa: E402

OUT = os.environ.get("IOU_FEAT_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
STATE_SEED, INPUT_SEED = 1600, 1700
SAMPLE = 2000
REF_ERR_MAX = 2.5e-5
DEPLOYED = ("dimp50", "prdimp50", "atom18")


def reference_module(t3, t4, sd):
    from ltr.models.bbreg import atom_iou_net as M
    net = M.AtomIoUNet(input_dim=(t3[0], t4[0]), pred_input_dim=(t3[2], t4[2]))
    net.conv3_1t, net.conv3_2t = M.conv(t3[0], t3[1]), M.conv(t3[1], t3[2])
    net.conv4_1t, net.conv4_2t = M.conv(t4[0], t4[1]), M.conv(t4[1], t4[2])
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and not [k for k in missing if k.split(".")[0] in ("conv3_1t", "conv3_2t", "conv4_1t", "conv4_2t")]
    return net.eval()


def main():
    for k, (name, (n, t3, t4)) in enumerate(synth.IOU_FEAT_CASES.items()):
        sseed, iseed = STATE_SEED + k, INPUT_SEED + k
        sd = synth.iou_feat_state(sseed, t3[0], t4[0], t3[1], t3[2], t4[1], t4[2])
        f3, f4 = synth.iou_feat_inputs(iseed, n, t3[0], t3[3], t3[4], t4[0], t4[3], t4[4])
        net = reference_module(t3, t4, sd)
        with torch.no_grad():
            c3, c4 = [t.numpy() for t in net.get_iou_feat([torch.from_numpy(f3), torch.from_numpy(f4)])]
        r3, r4 = iou_feat_np.get_iou_feat(sd, f3, f4)
        err = max(float(np.abs(c3 - r3).max()), float(np.abs(c4 - r4).max()))
        g = dict(state_seed=sseed, input_seed=iseed, n=n, tower3=np.array(t3), tower4=np.array(t4), ref_fp32_err=err,
                 max_abs=max(float(np.abs(c3).max()), float(np.abs(c4).max())))
        if name in DEPLOYED:
            for tag, c in (("3", c3), ("4", c4)):
                idx = np.sort(np.random.default_rng(sseed + int(tag)).choice(c.size, SAMPLE, replace=False))
                g["idx" + tag], g["c" + tag] = idx, c.reshape(-1)[idx]
        else:
            g["c3"], g["c4"] = c3, c4
        print(f"iou_feat_{name}: ref_fp32_err {err:.3e}  max |v| {g['max_abs']:.3f}  zeros {float((c3 == 0).mean()):.2f} / {float((c4 == 0).mean()):.2f}")
        assert err <= REF_ERR_MAX, (name, err)
        np.savez_compressed(os.path.join(OUT, f"iou_feat_{name}.npz"), **g)


if __name__ == "__main__":
    main()
