"""Timing of GNSteepestDescent on LinearFilterHinge (DiMP-simple / RTS classifier) on one GPU: microseconds per solve for
  fused      pytracking_amd.gn_hinge (pt_gn_hinge_solve_f32)
  ref        the reference's GNSteepestDescent (double autograd) on the device, no install()
  ref_bound  the same reference class after install(): its apply_filter / apply_feat_transpose are the rebound gfx950 ops
at the DiMP-simple size (n=50, 512x22x22, 4x4; 2 and 10 iterations) and the RTS classifier size (n=50, 512x15x26, 10 iterations),
plus the fused path's fraction of the HBM roofline: 8*n*C*H*W bytes per iteration at 8 TB/s.  Prints one JSON line.
Needs the reference (mounted tree or the oracle/_ref bundle).
    python tools/bench_gn_hinge.py [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from pytracking_amd import _lib, synth  # noqa: E402

HBM_BYTES_PER_S = 8e12


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    trials = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        trials.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(trials))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if _lib.needs_build():
        _lib.build_library()
    ref_harness.install()
    from pytracking import TensorList
    import ltr.models.meta.steepestdescent as smod
    import ltr.models.target_classifier.residual_modules as rm
    from pytracking_amd import gn_hinge as GH, install as amd
    dev = torch.device("cuda", 0)
    ref_gn = smod.GNSteepestDescent
    out = {"metric": "gn_hinge_us_per_solve"}
    cases = (("dimp_simple_it2", synth.DIMP_SIMPLE, 2), ("dimp_simple_it10", synth.DIMP_SIMPLE, 10), ("rts_clf_it10", synth.RTS_CLF, 10))
    for name, cfg, iters in cases:
        n, C, H, W, K = (cfg[k] for k in ("n", "C", "H", "W", "K"))
        w0, feat, label, sw = synth.gn_hinge_problem(11, n, C, H, W, K, 1, "per_image")
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        f, lab, sww, w = d(feat[:, 0]), d(label[:, 0])[:, None], d(sw).view(-1, 1, 1, 1), d(w0)
        res = rm.LinearFilterHinge(init_filter_reg=cfg["filter_reg"], hinge_threshold=cfg["hinge_threshold"],
                                   activation_leak=cfg["activation_leak"], score_act="relu").to(dev)
        kw = dict(feat=f, bb=None, train_label=lab, sample_weight=sww)
        fused = GH.GNSteepestDescent(res, num_iter=iters, compute_losses=False, residual_batch_dim=1)
        ref = ref_gn(residual_module=res, num_iter=iters, compute_losses=False, residual_batch_dim=1)

        def run(o):
            with torch.no_grad():
                o(TensorList([w]), **kw)
        row = {"fused": _time(lambda: run(fused), a.reps), "ref": _time(lambda: run(ref), max(3, a.reps // 3))}
        amd.install()
        try:
            row["ref_bound"] = _time(lambda: run(ref), max(3, a.reps // 3))
        finally:
            amd.uninstall()
        roof_us = 8.0 * n * C * H * W * iters / HBM_BYTES_PER_S * 1e6
        row["hbm_fraction"] = roof_us / row["fused"]
        row["route"] = "fast" if _lib.lib().pt_gn_hinge_route(
            f.data_ptr(), f.stride(0), w[0].data_ptr(), w.data_ptr(), n, C, H, W, K) == 1 else "generic"
        out[name] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
