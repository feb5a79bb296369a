"""Writes the goldens of the TaMOs heads (CPU; the regressor's need the reference tree, like tools/make_golden_tamos.py):

    tests/golden/tamos_heads_<case>.npz         for every regressor case of tests/tamos_heads_cases.py: the UNMODIFIED reference's
        `ltr.models.transformer.heads.DenseBoxRegressor` (through oracle.ref_harness) run on the case's seeded parameters and inputs in fp32
        and after `.double()`: ltrb_f32, ltrb_f64, keys (the reference's state_dict key names), stride (the deployed case keeps every
        DEPLOYED_KEEP-th element of the flattened output; 1 elsewhere)
    tests/golden/tamos_heads_fpn_deployed.npz   the FPN at the workload's size has no reference to run (torchvision is absent): the float64
        numpy restatement's own output (tests/tamos_heads_np.py), strided, so that the GPU test does not spend minutes in numpy

Only recorded outputs and key names are stored.  `python tools/make_golden_tamos_heads.py [case ...]`"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tamos_heads_cases as HC                 # noqa: E402
import tamos_heads_f64 as F64                  # noqa: E402


def reference_regressor(name):
    from oracle import ref_harness
    ref_harness.install()
    import ltr.models.transformer.heads as heads
    n_img, T, D, H, W = HC.REG[name]
    params, feat, filt = HC.reg_case(name)
    reg = heads.DenseBoxRegressor(num_channels=D)
    keys = list(reg.state_dict().keys())
    reg.load_state_dict(HC.to_sd(params), strict=True)
    reg.eval()
    out = {}
    with torch.no_grad():
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            m = reg.to(dt)
            o = m(torch.from_numpy(feat.copy()).to(dt)[None], torch.from_numpy(filt.copy()).to(dt).reshape(n_img, T, D, 1, 1))
            assert tuple(o.shape) == (1, n_img, T, 4, H, W) and o.dtype == dt
            out[tag] = o.numpy().reshape(-1)
    return keys, out


def main(names):
    gdir = os.path.join(ROOT, "tests", "golden")
    for name in names:
        if name in HC.REG:
            keys, out = reference_regressor(name)
            stride = HC.DEPLOYED_KEEP["ltrb"] if name == HC.REG_DEPLOYED else 1
            path = os.path.join(gdir, f"tamos_heads_{name}.npz")
            np.savez_compressed(path, ltrb_f32=out["f32"][::stride], ltrb_f64=out["f64"][::stride], stride=stride, keys=np.array(keys))
            print(f"{name}: reference |f32 - f64| max {np.abs(out['f32'].astype(np.float64) - out['f64']).max():.3e}, values up to "
                  f"{out['f64'].max():.3f}, {os.path.getsize(path)} bytes", flush=True)
        elif name == HC.FPN_DEPLOYED:
            w = F64.anchor(name).want
            path = os.path.join(gdir, "tamos_heads_fpn_deployed.npz")
            np.savez_compressed(path, **{f"{q}_f64": v.reshape(-1)[::HC.DEPLOYED_KEEP[q]] for q, v in w.items()},
                                **{f"{q}_stride": HC.DEPLOYED_KEEP[q] for q in w})
            print(f"{name}: {os.path.getsize(path)} bytes", flush=True)
        else:
            raise SystemExit(f"no golden for {name}")


if __name__ == "__main__":
    main(sys.argv[1:] or list(HC.REG) + [HC.FPN_DEPLOYED])
