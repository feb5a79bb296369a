"""TEST INFRASTRUCTURE ONLY -- tests/golden/box_enc_*.npz and tests/golden/box_cat_enc_*.npz from the UNMODIFIED reference on CPU (needs
the reference tree):
    python -B tools/make_golden_box_enc.py
ResidualDS16FeatSWBox.forward and ResidualDS16FeatSWBoxCatMultiBlock.forward (ltr/models/lwl/label_encoder.py:58-216) with use_gauss=False
in fp32 on the seeded state, features and boxes of every case of synth.BOX_ENC_CASES / synth.BOX_CAT_ENC_CASES.  Every file holds the
outputs as (n, F, h, w), the boxes, the seeds, `max_abs` and `ref_fp32_err`: the largest difference between that fp32 run (8 threads) and
the SAME module in float64.  A state of up to box_enc_cases.STORED_STATE_FLOATS floats is stored (`sd.<key>`); a larger one (res3 of the
deployed encoder alone is 5.9 MB) is regenerated from `state_seed` by the tests and checked against `state_checksum`.  The RTS classes
(ltr/models/rts/label_encoder.py) are run on the first case of each kind and must give the same bits."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import box_enc_cases as BC  # noqa: E402
from pytracking_amd import synth  # noqa: E402

OUT = os.environ.get("BOX_ENC_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
STATE_SEED, FEAT_SEED = {BC.BOX: 2300, BC.CAT: 2400}, {BC.BOX: 2350, BC.CAT: 2450}
REF_ERR_MAX = 1e-5


def reference_module(kind, c, sd, package="lwl"):
    M = importlib.import_module(f"ltr.models.{package}.label_encoder")
    if kind == BC.BOX:
        net = M.ResidualDS16FeatSWBox(layer_dims=c["dims"], feat_dim=c["feat_dim"], use_final_relu=c["final_relu"], use_gauss=False,
                                      use_bn=c["use_bn"], use_sample_w=c["use_sample_w"])
    else:
        net = M.ResidualDS16FeatSWBoxCatMultiBlock(layer_dims=c["dims"], feat_dim=c["feat_dim"], use_final_relu=c["final_relu"],
                                                   use_gauss=False, use_bn=c["use_bn"], final_bn=c["final_bn"])
    net.load_state_dict(BC.state_tensors(sd), strict=True)
    return net.eval()


def reference_module_f64(kind, c, sd):
    """The same module in float64.  bbox_to_mask always yields a float32 mask: the Cat class promotes it in its torch.cat, the FeatSWBox
    stem gets it cast by a forward pre-hook (the reference's code is not touched)."""
    net = reference_module(kind, c, sd).double()
    if kind == BC.BOX:
        net.conv_block.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    return net


def main():
    torch.set_num_threads(BC.THREADS)
    for kind in BC.KINDS:
        for k, name in enumerate(BC.CASES[kind]):
            c = BC.config(kind, name)
            sseed, fseed = STATE_SEED[kind] + k, FEAT_SEED[kind] + k
            sd = BC.state(kind, c, sseed)
            h, w = c["feat"]
            feat = synth.box_enc_feat(fseed, c["n"], c["feat_dim"], h, w)
            boxes = np.asarray(c["boxes"], dtype=np.float32).reshape(c["n"], 4)
            net = reference_module(kind, c, sd)
            out = BC.run(kind, net, BC.call_args(kind, c, boxes, feat), c)
            out64 = BC.run(kind, reference_module_f64(kind, c, sd), BC.call_args(kind, c, boxes, feat, dtype=torch.float64), c)
            if k == 0:
                other = BC.run(kind, reference_module(kind, c, sd, "rts"), BC.call_args(kind, c, boxes, feat), c)
                assert all(torch.equal(out[q], other[q]) for q in out)
            err = max(float((out[q].double() - out64[q]).abs().max()) for q in out)
            g = {q: t.numpy() for q, t in out.items()}
            stored = BC.state_floats(sd) <= BC.STORED_STATE_FLOATS
            if stored:
                g.update({"sd." + key: v for key, v in sd.items()})
            g.update(state_seed=sseed, feat_seed=fseed, state_checksum=np.float64(BC.checksum(sd)), boxes=boxes, ref_fp32_err=err,
                     max_abs=max(float(t.abs().max()) for t in out.values()))
            print(f"{kind}_{name}: out {tuple(out['label_enc'].shape)}  ref_fp32_err {err:.3e}  max |v| {g['max_abs']:.3f}  "
                  f"zeros in label_enc {float((out['label_enc'] == 0).float().mean()):.2f}  state {'stored' if stored else 'seed + checksum'}")
            assert err <= REF_ERR_MAX, (kind, name, err)
            path = os.path.join(OUT, f"{kind}_{name}.npz")
            np.savez_compressed(path, **g)
            assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))


if __name__ == "__main__":
    main()
