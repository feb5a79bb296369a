"""Device time of KeepTrack's target-candidate matching on one MI355X: the gfx950 path (pytracking_amd.candidate_matching) beside the
reference's own modules run on the same GPU in stock PyTorch-ROCm (needs the reference bundle, oracle/_ref).
    python -B tools/bench_keep_track.py [--reps 200] [--out FILE] [--no-track]
Sizes: default_fast (22x22 layer3, 23x23 score map) and default (30x30, 31x31); the last leg times a whole KeepTrack track().  Each figure is the mean over `reps` back-to-back
calls bracketed by one event pair (host launch cost included where a call is host-bound), after a warm-up."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from pytracking_amd import candidate_matching as CM, synth  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def track_leg():
    """One KeepTrack track() (tests/keep_track_tracker.py: stub backbone, 22x22 maps, DiMP-simple classifier + IoU refinement,
    candidate matching on every frame after the first) through install() against the same run without it, both on the GPU.
    Median wall time of frames 3..N (device synchronised around each call; the stub backbone's host-to-device copies included in both)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import keep_track_tracker as KT
    from pytracking_amd import install as amd
    run = dict(KT.RUN, n_frames=12)
    t_ref = []
    KT.run(device=DEV, rec_events=False, times=t_ref, **run)
    amd.install()
    try:
        t_fast = []
        KT.run(device=DEV, rec_events=False, times=t_fast, **run)
    finally:
        amd.uninstall()
    med = lambda t: sorted(t[2:])[len(t[2:]) // 2] * 1e6
    r = dict(piece="track", size="default_fast", fast_us=round(med(t_fast), 1), reference_us=round(med(t_ref), 1),
             speedup=round(med(t_ref) / med(t_fast), 1), frames=len(t_fast) - 2)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-track", action="store_true", help="skip the whole-track() leg (kernel-trace runs)")
    args = ap.parse_args()
    ref_harness.install()
    import ltr.data.processing_utils as prutils
    from ltr.models.target_candidate_matching.target_candidate_matching import DescriptorExtractor
    from ltr.models.target_candidate_matching.superglue import SuperGlue
    rows = []

    def rec(piece, size, fast_us, ref_us, **kw):
        r = dict(piece=piece, size=size, fast_us=round(fast_us, 2), reference_us=round(ref_us, 2),
                 speedup=round(ref_us / fast_us, 1), **kw)
        rows.append(r)
        print(json.dumps(r), flush=True)

    torch.manual_seed(0)
    with torch.no_grad():
        for size, cfg in (("default_fast", synth.TCM_FAST), ("default", synth.TCM_DEFAULT)):
            H, W = cfg["H"], cfg["W"]
            sm = torch.rand(H + 1, W + 1, device=DEV) * 0.3
            sm[5, 5], sm[H - 4, W - 6], sm[H // 2, 3] = 0.9, 0.6, 0.4
            c, _ = CM.find_local_maxima(sm, 0.1, 5)
            rec("peaks", size, timed(lambda: CM.find_local_maxima(sm, 0.1, 5), args.reps),
                timed(lambda: prutils.find_local_maxima(sm, 0.1, 5), args.reps), peaks=int(c.shape[0]))
            ext = DescriptorExtractor(1024, 256, 4).to(DEV).eval()
            x = torch.from_numpy(synth.tcm_layer3(3, 1, 1024, H, W)).to(DEV)
            for P in (1, 8, 32):
                coords = torch.stack([torch.randint(0, H + 1, (P,)), torch.randint(0, W + 1, (P,))], 1).to(DEV)
                rec("descriptors", size, timed(lambda: CM.get_descriptors(ext, x, coords), args.reps),
                    timed(lambda: ext.get_descriptors(x, coords), args.reps), P=P)
        sg = SuperGlue({'skip_gnn': False, 'GNN_layers': ['self', 'cross'] * 2, 'num_sinkhorn_iterations': 10,
                        'output_normalization': 'sinkhorn'})
        sg.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.tcm_superglue_state(11).items()})
        sg = sg.to(DEV).eval()
        for M, N in ((2, 2), (8, 8), (32, 32)):
            d = {k: torch.from_numpy(v).to(DEV) for k, v in synth.tcm_match_inputs(12, M, N).items()}
            d["image_size0"] = d["image_size1"] = torch.Size((480, 640))
            rec("matcher", "M=%d,N=%d" % (M, N), timed(lambda: CM.match(sg, d), args.reps),
                timed(lambda: sg._forward(d), max(20, args.reps // 10)))
    if not args.no_track:
        rows.append(track_leg())
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
