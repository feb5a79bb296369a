"""TEST INFRASTRUCTURE ONLY -- tests/golden/rts_fusion_*.npz from the UNMODIFIED reference on CPU (needs the reference tree):
    python -B tools/make_golden_rts_fusion.py
  rts_fusion_enc_<case>    ResidualDS16SW_Clf.forward (ltr/models/rts/label_encoder.py:57-103) on synth.label_enc_state / synth.score_maps for
                           every case of synth.SCORE_ENC_CASES: the state (`sd.<key>`), the seeds, the shape, both outputs as (n, F, H, W)
  rts_fusion_fuse_<case>   interpolate (ltr/models/rts/utils.py) + LearnersFusion.forward (ltr/models/rts/learners_fusion.py), as
                           RTSNet.segment_target chains them, for every case of synth.LEARNERS_FUSE_CASES and both fusion types: the
                           'concat' state (`sd.concat.<key>`), the seeds, the shape, `out.add` / `out.concat` as (n, F, Ht, Wt).  The
                           reference fixes the convolution at 32 -> 16 channels; for a case with another F the module's `fusion_conv1` is
                           replaced by a Conv2d(2F, F, 3, padding=1) before the state is loaded -- its forward is the reference's.
  rts_fusion_chain_deployed  the encoder at 16 x 27, then the fuse to 30 x 52, for both fusion types; to stay within the size of the other
                           files it stores the 'concat' state only: the encoder's is synth.label_enc_state(state_seed).
Inputs are regenerated from the stored seeds by the tests.  `ref_fp32_err` (per fusion type: `ref_fp32_err.<type>`) is the largest
difference between the fp32 run, with the 8 threads tests/f64_bound.py pins, and the SAME modules in float64; asserted <= 1e-5, a tenth of
the 1e-4 bound the GPU tests hold against these files."""
import copy
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
import rts_fusion_cases as RC  # noqa: E402

OUT = os.environ.get("RTS_FUSION_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
REF_ERR_MAX = 1e-5


def t(a):
    return torch.from_numpy(np.array(a))


def reference_encoder(dims, use_bn, sd):
    from ltr.models.rts.label_encoder import ResidualDS16SW_Clf
    net = ResidualDS16SW_Clf(layer_dims=dims, use_bn=use_bn)
    net.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return net.eval()


def reference_fusion(kind, f, sd):
    from ltr.models.rts.learners_fusion import LearnersFusion
    net = LearnersFusion(kind)
    if kind == "concat" and f != 16:
        net.fusion_conv1 = torch.nn.Conv2d(2 * f, f, kernel_size=3, padding=1, stride=1)
    net.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return net.eval()


def reference_fuse(fusion, seg, clf):
    """rts_net.py:227-230 with mask_encoding_pred = seg (1, n, F, Ht, Wt) and encoded_clf_scores = clf (1, n, F, Hs, Ws)."""
    from ltr.models.rts.utils import interpolate
    return fusion(seg, interpolate(clf[0, :, :, :, :], seg.shape[-2:]).unsqueeze(0))


def both(fn, nets, args):
    """(fp32 outputs with the pinned thread count, largest |fp32 - float64|)."""
    with torch.no_grad():
        want = fn([copy.deepcopy(m).double() for m in nets], [a.double() for a in args])
        threads = torch.get_num_threads()
        try:
            torch.set_num_threads(f64_bound.THREADS)
            got = fn(nets, args)
        finally:
            torch.set_num_threads(threads)
    return [g.numpy() for g in got], max(float((g.double() - w).abs().max()) for g, w in zip(got, want))


def save(tag, g):
    path = os.path.join(OUT, f"rts_fusion_{tag}.npz")
    np.savez_compressed(path, **g)
    assert os.path.getsize(path) < 560 * 1024, (path, os.path.getsize(path))         # what the label-encoder goldens keep


def main():
    for k, (name, (n, H, W, dims, use_bn)) in enumerate(synth.SCORE_ENC_CASES.items()):
        sseed, iseed = RC.ENC_STATE_SEED + k, RC.ENC_INPUT_SEED + k
        sd = synth.label_enc_state(sseed, dims, use_bn)
        scores = t(synth.score_maps(iseed, n, H, W))[:, None]                        # (frames, 1 sequence, H, W)
        (enc, sw), err = both(lambda nets, a: [o[:, 0] for o in nets[0](a[0])], [reference_encoder(dims, use_bn, sd)], [scores])
        g = {"sd." + key: v for key, v in sd.items()}
        g.update(state_seed=sseed, input_seed=iseed, n=n, H=H, W=W, dims=np.array(dims), use_bn=use_bn, ref_fp32_err=err,
                 max_abs=max(float(np.abs(enc).max()), float(np.abs(sw).max())), label_enc=enc, sample_w=sw)
        print(f"enc_{name}: out {enc.shape}  ref_fp32_err {err:.3e}  max |v| {g['max_abs']:.3f}  zeros in label_enc {float((enc == 0).mean()):.2f}")
        assert err <= REF_ERR_MAX, (name, err)
        save("enc_" + name, g)
    for k, (name, (n, f, source, target)) in enumerate(synth.LEARNERS_FUSE_CASES.items()):
        sseed, iseed = RC.FUSE_STATE_SEED + k, RC.FUSE_INPUT_SEED + k
        seg, clf = [t(a) for a in synth.learners_fuse_inputs(iseed, n, f, source, target)]
        g = dict(state_seed=sseed, input_seed=iseed, n=n, F=f, source=np.array(source), target=np.array(target))
        for kind in synth.FUSION_TYPES:
            sd = synth.learners_fusion_state(sseed, f, kind)
            (out,), err = both(lambda nets, a: [reference_fuse(nets[0], a[0], a[1])[0]], [reference_fusion(kind, f, sd)], [seg, clf])
            g.update({"sd.concat." + key: v for key, v in sd.items()})
            g.update({"out." + kind: out, "ref_fp32_err." + kind: err, "max_abs." + kind: float(np.abs(out).max())})
            print(f"fuse_{name} {kind}: out {out.shape}  ref_fp32_err {err:.3e}  max |v| {float(np.abs(out).max()):.3f}")
            assert err <= REF_ERR_MAX, (name, kind, err)
        save("fuse_" + name, g)
    c = synth.RTS_CHAIN_CASE
    f = c["dims"][3]
    sd_enc = synth.label_enc_state(RC.CHAIN_SEED, c["dims"], False)
    scores = t(synth.score_maps(RC.CHAIN_SEED + 1, 1, c["H"], c["W"]))[None]
    seg = t(synth.learners_fuse_inputs(RC.CHAIN_SEED + 2, 1, f, (c["H"], c["W"]), c["target"])[0])
    g = dict(state_seed=RC.CHAIN_SEED, input_seed=RC.CHAIN_SEED + 1)         # the encoder state is regenerated from state_seed (size)
    for kind in synth.FUSION_TYPES:
        sd = synth.learners_fusion_state(RC.CHAIN_SEED + 3, f, kind)
        (out,), err = both(lambda nets, a: [reference_fuse(nets[1], a[1], nets[0](a[0])[0])[0]],
                           [reference_encoder(c["dims"], False, sd_enc), reference_fusion(kind, f, sd)], [scores, seg])
        g.update({"sd.concat." + key: v for key, v in sd.items()})
        g.update({"out." + kind: out, "ref_fp32_err." + kind: err, "max_abs." + kind: float(np.abs(out).max())})
        print(f"{RC.CHAIN} {kind}: out {out.shape}  ref_fp32_err {err:.3e}  max |v| {float(np.abs(out).max()):.3f}")
        assert err <= REF_ERR_MAX, (kind, err)
    save(RC.CHAIN, g)


if __name__ == "__main__":
    main()
