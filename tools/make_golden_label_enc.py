"""TEST INFRASTRUCTURE ONLY -- tests/golden/label_enc_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_label_enc.py
ResidualDS16SW.forward (ltr/models/lwl/label_encoder.py:9-55) in fp32 on synth.label_enc_state / synth.label_enc_masks for every case of
synth.LABEL_ENC_CASES.  Every file holds the state (`sd.<key>`), the seeds, the shape and both outputs as (n, F, h, w); the masks are
regenerated from `mask_seed` by the tests.  `ref_fp32_err` is the largest difference between that fp32 run and the SAME module in float64;
asserted <= 1e-5, a tenth of the 1e-4 bound the GPU tests hold against these files (a case beyond it gets rescaled weights, never a wider
bound).  The RTS module (ltr/models/rts/label_encoder.py) is run on the first case and must give the same bits."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

ref_harness.install()

from pytracking_amd import synth  # noqa: E402

OUT = os.environ.get("LABEL_ENC_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
STATE_SEED, MASK_SEED = 2100, 2200
REF_ERR_MAX = 1e-5


def reference_module(dims, use_bn, sd, package="lwl"):
    import importlib
    M = importlib.import_module(f"ltr.models.{package}.label_encoder")
    net = M.ResidualDS16SW(layer_dims=dims, use_bn=use_bn)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return net.eval()


def main():
    for k, (name, (n, H, W, dims, use_bn)) in enumerate(synth.LABEL_ENC_CASES.items()):
        sseed, mseed = STATE_SEED + k, MASK_SEED + k
        sd = synth.label_enc_state(sseed, dims, use_bn)
        masks = torch.from_numpy(synth.label_enc_masks(mseed, n, H, W))[:, None]         # (frames, 1 sequence, H, W)
        net = reference_module(dims, use_bn, sd)
        with torch.no_grad():
            enc, sw = [t[:, 0].numpy() for t in net(masks)]
            enc64, sw64 = [t[:, 0].numpy() for t in reference_module(dims, use_bn, sd).double()(masks.double())]
            if k == 0:
                for a, b in zip(net(masks), reference_module(dims, use_bn, sd, "rts")(masks)):
                    assert torch.equal(a, b)
        err = max(float(np.abs(enc - enc64).max()), float(np.abs(sw - sw64).max()))
        g = {"sd." + key: v for key, v in sd.items()}
        g.update(state_seed=sseed, mask_seed=mseed, n=n, H=H, W=W, dims=np.array(dims), use_bn=use_bn, ref_fp32_err=err,
                 max_abs=max(float(np.abs(enc).max()), float(np.abs(sw).max())), label_enc=enc, sample_w=sw)
        print(f"label_enc_{name}: out {enc.shape}  ref_fp32_err {err:.3e}  max |v| {g['max_abs']:.3f}  zeros in label_enc {float((enc == 0).mean()):.2f}")
        assert err <= REF_ERR_MAX, (name, err)
        path = os.path.join(OUT, f"label_enc_{name}.npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))


if __name__ == "__main__":
    main()
