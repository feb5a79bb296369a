"""Every plan of the banded tap-major 3x3 correlation (k_mf_corr<9, VW, true, NPG>) and the GEMM route of iou_feat.hip on the MI355X:
the cases of tests/corr_tm_cases.py through pytracking_amd.iou_feat.get_iou_feat against the same module and inputs in float64 on the
CPU -- full maps of both towers within the project's 1e-4 absolute (BASELINE.json; ATOL of tests/test_gpu_iou_feat.py), two calls
bit-identical -- and one call per route on one-hot inputs against power-of-two taps, compared exactly.  Needs no reference tree.

Every test prints its measured maximum error and the fp32 CPU module's own distance from float64 before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import corr_tm_cases as CT
from f64_bound import dev
from pytracking_amd import _lib, iou_feat as IF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4


def _where(name, n, t3, t4, got, ref):
    """The worst element of each tower, located in the plan: '(image, channel, row, col)' and the band / row within the band it falls in
    for the band heights of the tower's two layers."""
    L = _lib.lib()
    lines, worst = [], 0.0
    for tag, t, g, r in (("3", t3, got[0], ref[0]), ("4", t4, got[1], ref[1])):
        d = np.abs(g - r)
        i, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))
        worst = max(worst, float(d.max()))
        where = []
        for l in range(2):
            p, Wp = CT.plan(L, n, t[l + 1], t[l], t[3], t[4])
            where.append(f"layer {l + 1} GEMM route" if p is CT.GEMM else
                         f"layer {l + 1} (ks, br, npg, nb, last, vw, out_vec) = {p}, Wp {Wp}: band {y // p[1]}, row {y % p[1]} of the band")
        lines.append(f"{name} tower {tag} {t}: max |gpu - float64| = {float(d.max()):.3e} at (image {i}, channel {c}, row {y}, col {x}) "
                     f"gpu {g[i, c, y, x]!r} float64 {r[i, c, y, x]!r}; " + "; ".join(where) + f"; {int((d > ATOL).sum())} elements off")
    return worst, "\n".join(lines)


@pytest.mark.parametrize("name", list(CT.CASES))
def test_full_maps_match_float64(name):
    n, t3, t4, sd, feats = CT.case(name)
    ref, f32_err = CT.reference(name)
    net = CT.module(name, DEV)
    with torch.no_grad():
        fd = [dev(f) for f in feats]
        assert IF.covered(net, fd)
        c3, c4 = IF.get_iou_feat(net, fd)
        d3, d4 = IF.get_iou_feat(net, fd)
    assert c3.shape == (n, t3[2], t3[3], t3[4]) and c4.shape == (n, t4[2], t4[3], t4[4])
    got = [c3.cpu().numpy().astype(np.float64), c4.cpu().numpy().astype(np.float64)]
    err, msg = _where(name, n, t3, t4, got, ref)
    print(f"\ncorr_tm_{name}: max |gpu - float64| = {err:.3e} (bound {ATOL:.0e}; fp32 CPU module - float64 = {f32_err:.3e})\n{msg}")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), msg
    assert err <= ATOL, msg
    assert torch.equal(c3, d3) and torch.equal(c4, d4), f"{name}: two calls differ"        # fixed-order sums: bit-identical


@pytest.mark.parametrize("route", list(CT.STRUCTURED))
def test_one_hot_maps_against_power_of_two_taps_are_exact(route):
    """A shifted row, a leaked padding column, a swapped tap or a lost channel split is a whole-number error here."""
    n, t3, t4 = CT.STRUCTURED[route]
    L = _lib.lib()
    assert tuple(CT.plan(L, *shape)[0] for _, _, *shape in CT.layers(n, t3, t4)) == CT.STRUCTURED_PLANS[route]
    feats = []
    for t in (t3, t4):
        plans = [CT.plan(L, n, t[l + 1], t[l], t[3], t[4])[0] for l in range(2)]
        rows = sorted({p[1] for p in plans}) if route == "banded" else [1]
        feats.append(CT.structured_input(n, t[0], t[3], t[4], CT.hot_spots(t[3], t[4], rows)))
    ref = CT.run_cpu(CT.structured_module(t3, t4), feats, torch.float64)
    assert all(float(r.max()) < 2 ** 24 and np.array_equal(r, np.round(r)) for r in ref) and float(ref[0].max()) >= 256
    net = CT.structured_module(t3, t4).to(DEV)
    with torch.no_grad():
        fd = [dev(f) for f in feats]
        assert IF.covered(net, fd)
        got = [c.cpu().numpy().astype(np.float64) for c in IF.get_iou_feat(net, fd)]
    err, msg = _where(route, n, t3, t4, got, ref)
    print(f"\ncorr_tm structured {route}: max |gpu - float64| = {err:.3e} (exact expected)\n{msg}")
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), msg
