"""KeepTrack target-candidate matching on the MI355X (tcm.hip through pytracking_amd.candidate_matching) against the float64 restatement
tests/tcm_np.py on the cases of tests/tcm_cases.py, which lie off the shapes of the two deployed configurations: peaks exactly (several
compaction passes, more than 1024 hits, H != W, ks of 1, 3 and 127, ties, non-finite values, the 4-D form); descriptors (B > 1, H != W, both
coordinate forms, 16 / 17 / 32 / 33 points, one K slice) and the matcher (1x1, 64x1, 1x64, T = 17 and 49, unequal image sizes, four layer
masks, zero and one Sinkhorn iteration) within f64_bound.bound(ref_err) of float64, ref_err being the fp32 CPU run's own distance from
float64 on the case; the matcher's matches0 / matches1 and the zero pattern of its scores exactly (every case is well-conditioned:
tests/test_keep_track_cpu.py); every second call bit-equal to the first.

match_scores = exp(z) of a mutual maximum z of log_assignment, so an error dz of z moves it by exp(z) dz: where the score is at most 1 it is
held to the bound of z itself, and where it exceeds 1 (without a Sinkhorn iteration Z is not normalised: `it0` has scores of 1e13, which
fp32 resolves to 1e6) to the bound times the score.

Every test prints the measured figures before it asserts (run with -s; profiles/keep_track_f64.txt)."""
import types

import numpy as np
import pytest
import torch

import f64_bound
import tcm_cases as TC
from f64_bound import dev, needs_bundle
from oracle import ref_harness
from pytracking_amd import candidate_matching as CM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", [pytest.param(n, marks=needs_bundle) if TC.PEAK_CASES[n][4] == "batch3" else n for n in TC.PEAK_CASES])
def test_peaks_exact(name):
    H, W, ks, th, how, _ = TC.PEAK_CASES[name]
    want = TC.peak_want(name)
    if how == "batch3":
        ref_harness.install()                  # the 4-D form returns the reference's TensorList
    scores = dev(TC.peak_map(name))
    cs, vs = CM.find_local_maxima(scores, th, ks)
    cs2, vs2 = CM.find_local_maxima(scores, th, ks)
    if how == "batch3":
        assert type(cs).__name__ == "TensorList" and len(cs) == len(vs) == len(want)
    else:
        cs, vs, cs2, vs2 = [cs], [vs], [cs2], [vs2]
    print(f"\npeaks {name}: hits {[len(c) for c in cs]}, float64 anchor {[len(c) for c, _ in want]}")
    for c, v, c2, v2, (wc, wv) in zip(cs, vs, cs2, vs2, want):
        assert c.dtype == torch.int64 and v.dtype == torch.float32 and c.shape == (len(wc), 2) and v.shape == (len(wc),)
        np.testing.assert_array_equal(c.cpu().numpy(), wc)
        np.testing.assert_array_equal(v.cpu().numpy(), wv)
        assert torch.equal(c, c2) and torch.equal(v, v2)


@pytest.mark.parametrize("name", list(TC.DESC_CASES))
def test_descriptors_within_the_float64_bound(name):
    B, C, H, W, D, P, form, _ = TC.DESC_CASES[name]
    i, a = TC.desc_inputs(name), TC.desc_anchor(name)
    conv = torch.nn.Conv2d(C, D, 4, padding=2)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(i.weight))
        conv.bias.copy_(torch.from_numpy(i.bias))
    ext = types.SimpleNamespace(conv=conv.to(DEV).eval())
    x, coords = dev(i.x), dev(i.coords)
    with torch.no_grad():
        assert CM.covered_get_descriptors(ext, x, coords)
        out = CM.get_descriptors(ext, x, coords)
        again = CM.get_descriptors(ext, x, coords)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, D, P)
    err = np.abs(out.double().cpu().numpy() - a.want)
    print(f64_bound.report(f"desc {name}", {f"image {b}": float(err[b].max()) for b in range(B)}, a.ref_err))
    assert err.max() <= f64_bound.bound(a.ref_err)
    assert torch.equal(out, again)


@needs_bundle
@pytest.mark.parametrize("name", list(TC.MATCH))
def test_matcher_within_the_float64_bound(name):
    _, M, N, layers, iters, _, _, _ = TC.MATCH[name]
    a = TC.match_anchor(name)
    sg, data = TC.superglue(name, device=DEV), TC.match_data(name, device=DEV)
    with torch.no_grad():
        assert CM.covered_match(sg, data)
        pred = CM.match(sg, data)
        again = CM.match(sg, data)
    got = {k: pred[k][0].cpu().numpy() for k in TC.MATCH_OUTPUTS}
    assert pred["log_assignment"].shape == (1, M + 1, N + 1) and pred["log_assignment"].dtype == torch.float32
    assert pred["matches0"].dtype == torch.int64 and pred["matches0"].shape == (1, M) and pred["matches1"].shape == (1, N)
    assert pred["match_scores0"].dtype == torch.float32 and pred["bin_score"] is sg.bin_score
    b = f64_bound.bound(a.ref_err)
    errs = {"log_assignment": float(np.abs(got["log_assignment"].astype(np.float64) - a.want["log_assignment"]).max())}
    for k in ("match_scores0", "match_scores1"):                  # in units of the score's own bound: b where it is <= 1, b x score above
        errs[k + " / max(1, score)"] = float((np.abs(got[k].astype(np.float64) - a.want[k]) / np.maximum(1.0, a.want[k])).max())
    print(f64_bound.report(f"match {name} ({M}x{N}, {len(layers)} layers, {iters} iterations)", errs, a.ref_err)
          + f"  matches {int((a.want['matches0'] >= 0).sum())}")
    assert all(e <= b for e in errs.values()), errs
    np.testing.assert_array_equal(got["matches0"], a.want["matches0"])
    np.testing.assert_array_equal(got["matches1"], a.want["matches1"])
    np.testing.assert_array_equal(got["match_scores0"] == 0, a.want["match_scores0"] == 0)
    np.testing.assert_array_equal(got["match_scores1"] == 0, a.want["match_scores1"] == 0)
    for k in TC.MATCH_OUTPUTS:
        assert torch.equal(pred[k], again[k]), k
