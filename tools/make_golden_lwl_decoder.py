"""TEST INFRASTRUCTURE ONLY -- tests/golden/lwl_decoder_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_lwl_decoder.py
LWTLDecoder.forward (ltr/models/lwl/decoder.py:87-160) in fp32 on synth.lwl_decoder_state / synth.lwl_decoder_inputs for every case of
synth.LWL_DECODER_CASES.  Weights and inputs are NOT stored (the deployed state is about 13 MB): every file holds the seeds, the fp32
outputs and `ref_fp32_err`, the largest difference between that fp32 run and the SAME module in float64 over the mask and every level;
asserted <= 1e-5, a tenth of the 1e-4 bound the GPU tests hold against these files (a case beyond it gets rescaled weights, never a wider
bound).  Small cases store the mask and every '{L}_dec' map in full; `deployed` stores mask[..., ::4, ::4] and layer4_dec in full.  The RTS
class (ltr/models/rts/decoder.py) is run on the first case and must give the same bits."""
import importlib
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

ref_harness.install()

from pytracking_amd import synth  # noqa: E402

OUT = os.environ.get("LWL_DECODER_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
STATE_SEED, INPUT_SEED = 2300, 2400
REF_ERR_MAX = 1e-5


def reference_module(case, sd, package="lwl"):
    M = importlib.import_module(f"ltr.models.{package}.decoder")
    cls = M.LWTLDecoder if package == "lwl" else M.RTSDecoder
    net = cls(case["ic"], case["mdim"], OrderedDict((L, fc) for L, fc, _, _ in case["levels"]), use_bn=case["use_bn"])
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return net.eval()


def main():
    for k, (name, case) in enumerate(synth.LWL_DECODER_CASES.items()):
        sseed, iseed = STATE_SEED + k, INPUT_SEED + k
        sd = synth.lwl_decoder_state(sseed, case["mdim"], case["ic"], case["use_bn"], case["levels"])
        s, feats = synth.lwl_decoder_inputs(iseed, case["n"], case["ic"], case["levels"], case["scores"])
        s = torch.from_numpy(s)
        feats = {L: torch.from_numpy(v) for L, v in feats.items()}
        names = ["{}_dec".format(L) for L, _, _, _ in case["levels"]]
        with torch.no_grad():
            mask, outs = reference_module(case, sd)(s, feats, case["image"], names)
            mask64, outs64 = reference_module(case, sd).double()(s.double(), {L: v.double() for L, v in feats.items()}, case["image"], names)
            if k == 0:
                m2, o2 = reference_module(case, sd, "rts")(s, feats, case["image"], names)
                assert torch.equal(mask, m2) and all(torch.equal(outs[q], o2[q]) for q in names)
        err = max([float((mask - mask64).abs().max())] + [float((outs[q] - outs64[q]).abs().max()) for q in names])
        g = dict(state_seed=sseed, input_seed=iseed, ref_fp32_err=err, max_abs=float(mask.abs().max()))
        if name == "deployed":
            g["mask"] = mask[..., ::4, ::4].numpy()
            g[names[0]] = outs[names[0]].numpy()
        else:
            g["mask"] = mask.numpy()
            g.update({q: outs[q].numpy() for q in names})
        print(f"lwl_decoder_{name}: mask {tuple(mask.shape)}  ref_fp32_err {err:.3e}  max |mask| {g['max_abs']:.3f}  "
              + "  ".join(f"{q} {float(outs[q].abs().max()):.2f}/{float((outs[q] == 0).float().mean()):.2f}" for q in names))
        assert err <= REF_ERR_MAX, (name, err)
        path = os.path.join(OUT, f"lwl_decoder_{name}.npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))


if __name__ == "__main__":
    main()
