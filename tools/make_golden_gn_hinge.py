"""TEST INFRASTRUCTURE ONLY -- tests/golden/gn_hinge_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_gn_hinge.py
`ltr.models.meta.steepestdescent.GNSteepestDescent` driving `ltr.models.target_classifier.residual_modules.LinearFilterHinge`
(dimpnet.py:236-242, rts_net.py:325-333: residual_batch_dim=1, compute_losses=True).  Inputs come from
pytracking_amd.synth.gn_hinge_problem; the small cases store them, the deployed sizes store (seed, shape) + outputs only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

ref_harness.install()

from pytracking_amd import synth  # noqa: E402

OUT = os.environ.get("GN_HINGE_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))   # (tests regenerate into a scratch dir)
T = torch.from_numpy

# name: (seed, n, C, H, W, K, S, sw_mode, score_act, act_param, thr, leak, filter_reg (float: learn_filter_reg=False), steplength_reg,
#        num_iter, store_inputs)
CASES = {
    "gn_hinge_relu_none": (701, 5, 16, 7, 8, 4, 1, "none", "relu", None, 0.05, 0.1, 0.1, 0.0, 3, True),
    "gn_hinge_relu_img_leak0": (702, 4, 24, 6, 9, 3, 1, "per_image", "relu", None, 0.05, 0.0, 0.05, 0.0, 3, True),
    "gn_hinge_bent_img": (703, 6, 16, 8, 8, 4, 1, "per_image", "bentpar", 0.2, 0.05, 0.1, 0.1, 0.0, 3, True),
    "gn_hinge_bent_slreg": (704, 3, 20, 5, 7, 1, 1, "none", "bentpar", 1.0, 0.1, 0.1, 0.1, 0.5, 4, True),
    "gn_hinge_relu_s2": (705, 4, 16, 6, 6, 4, 2, "per_image", "relu", None, 0.05, 0.1, 0.1, 0.2, 2, True),
    "gn_hinge_relu_floatreg": (706, 5, 16, 7, 6, 2, 1, "none", "relu", None, 0.05, 0.0, 0.08, 0.0, 3, True),
    "gn_hinge_fast_small": (707, 8, 128, 8, 8, 4, 1, "per_image", "relu", None, 0.05, 0.1, 0.1, 0.0, 3, True),
    "gn_hinge_dimp_simple_it10": (750, 50, 512, 22, 22, 4, 1, "none", "relu", None, 0.05, 0.1, 0.1, 0.0, 10, False),
    "gn_hinge_dimp_simple_it2": (751, 50, 512, 22, 22, 4, 1, "per_image", "relu", None, 0.05, 0.1, 0.1, 0.0, 2, False),
    "gn_hinge_rts_clf_it10": (752, 50, 512, 15, 26, 4, 1, "per_image", "relu", None, 0.05, 0.0, 0.1, 0.0, 10, False),
}
FLOAT_REG = {"gn_hinge_relu_floatreg", "gn_hinge_rts_clf_it10"}


def run_reference(seed, n, C, H, W, K, S, sw_mode, score_act, act_param, thr, leak, reg, slreg, num_iter, float_reg):
    from pytracking import TensorList
    from ltr.models.meta.steepestdescent import GNSteepestDescent
    from ltr.models.target_classifier.residual_modules import LinearFilterHinge
    import ltr.models.layers.filter as rfilter
    w0, feat, label, sw = synth.gn_hinge_problem(seed, n, C, H, W, K, S, sw_mode)
    res = LinearFilterHinge(feat_stride=16, init_filter_reg=reg, hinge_threshold=thr, activation_leak=leak, score_act=score_act,
                            act_param=act_param, learn_filter_reg=not float_reg)
    opt = GNSteepestDescent(residual_module=res, num_iter=num_iter, compute_losses=True, steplength_reg=slreg, residual_batch_dim=1)
    f = T(feat) if S > 1 else T(feat[:, 0])
    lab = T(label) if S > 1 else T(label[:, 0])[:, None]
    sww = None if sw is None else T(sw).view(-1, 1, 1, 1)       # dimp_simple.py:679
    w, its, losses = opt(TensorList([T(w0)]), feat=f, bb=None, train_label=lab, sample_weight=sww)
    with torch.no_grad():
        scores = rfilter.apply_filter(T(feat), w[0].detach())
    return w0, feat, label, sw, dict(
        iterates=torch.stack([i[0].detach() for i in its], dim=1).numpy(),       # (S, T+1, C, K, K)
        losses=torch.stack([l.detach().reshape(()) for l in losses]).numpy(),
        scores=scores.numpy())                                                  # (n, S, OH, OW)


RTS_CASES = ("gn_rts_small", "gn_rts_cfg5_n32")


def run_rts(name):
    """RTS segmentation learner: the reference's GNSteepestDescent on RTSResidual (rts_net.py:309-315, residual_batch_dim=1), called
    as rts/linear_filter.py:85 does: label and sample weight per element, (n, 1, F, H, W)."""
    from pytracking import TensorList
    from ltr.models.meta.steepestdescent import GNSteepestDescent
    from ltr.models.rts.loss_residual_modules import RTSResidual
    import ltr.models.layers.filter as rfilter
    if name == "gn_rts_small":
        cfg, seed, it = dict(n=3, F=4, C=16, H=7, W=9, K=3, filter_reg=0.1), 801, 3
    else:
        cfg, seed, it = synth.LWL, 802, 3
    w0, feat, label, sw = synth.lwl_problem(seed, cfg)
    res = RTSResidual(init_filter_reg=cfg["filter_reg"])
    opt = GNSteepestDescent(residual_module=res, num_iter=it, compute_losses=True, residual_batch_dim=1)
    w, its, losses = opt(TensorList([T(w0)[None]]), feat=T(feat)[:, None], label=T(label)[:, None], sample_weight=T(sw)[:, None])
    with torch.no_grad():
        scores = rfilter.apply_filter(T(feat[:2] if name != "gn_rts_small" else feat)[:, None], w[0].detach())[:, 0].numpy()
    out = dict(seed=seed, num_iter=it, filter_reg=cfg["filter_reg"], **{k: cfg[k] for k in ("n", "F", "C", "H", "W", "K")},
               losses=torch.stack([l.detach().reshape(()) for l in losses]).numpy())
    iters = torch.stack([i[0][0].detach() for i in its]).numpy()
    if name == "gn_rts_small":
        out.update(w0=w0, feat=feat, label=label, sw=sw, iterates=iters, scores=scores)
    else:                  # what fits in 1 MB: the full iterate stack is 1.8 MB
        out.update(iterate1=iters[1], final=iters[-1], scores_first2=scores)
    return out


def run_tracker():
    """The unmodified DiMPSimple on CPU (tests/dimp_simple_tracker.py), its boundary calls event by event."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dimp_simple_tracker as DST
    _, rec, _ = DST.run(**DST.RUN)
    return rec.to_npz_dict()


def main():
    which = sys.argv[1:] or list(CASES) + list(RTS_CASES) + ["tracker_dimp_simple"]
    for name in which:
        if name in RTS_CASES or name == "tracker_dimp_simple":
            meta = run_rts(name) if name in RTS_CASES else run_tracker()
            path = os.path.join(OUT, name + ".npz")
            np.savez_compressed(path, **{k: np.asarray(v) for k, v in meta.items()})
            print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")
            continue
        c = CASES[name]
        seed, n, C, H, W, K, S, sw_mode, act, b, thr, leak, reg, slreg, it, store = c
        w0, feat, label, sw, out = run_reference(seed, n, C, H, W, K, S, sw_mode, act, b, thr, leak, reg, slreg, it, name in FLOAT_REG)
        meta = dict(seed=seed, n=n, C=C, H=H, W=W, K=K, S=S, sw_mode=sw_mode, score_act=act, act_param=0.0 if b is None else b,
                    hinge_threshold=thr, activation_leak=leak, filter_reg=reg, float_reg=name in FLOAT_REG, steplength_reg=slreg,
                    num_iter=it)
        if store:
            meta.update(w0=w0, feat=feat, label=label, sw=np.zeros(0, np.float32) if sw is None else sw, **out)
        else:    # deployed sizes: seed + outputs (the full iterate stack and the inputs are regenerated / not stored)
            meta.update(iterate1=out["iterates"][:, 1], final=out["iterates"][:, -1], losses=out["losses"],
                        scores_first4=out["scores"][:4])
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in meta.items()})
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
