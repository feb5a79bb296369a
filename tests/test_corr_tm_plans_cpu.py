"""The plan space of the banded tap-major 3x3 correlation without a GPU: every convolution of tests/corr_tm_cases.py lands on the plan
pinned next to it (pt_mf_corr_tm_plan: the launcher's own mf_tm_config + mf_plan, host only), pt_iou_feat_ws_bytes switches routes and
refuses shapes exactly at its limits, and the new cases together with synth.IOU_FEAT_CASES cover every cell of the plan space named
below -- a condition on the case table, not a measurement."""
import pytest

import corr_tm_cases as CT
from pytracking_amd import _lib, synth


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


@pytest.mark.parametrize("name", list(CT.CASES))
def test_case_lands_on_its_pinned_plan(L, name):
    n, t3, t4 = CT.CASES[name]
    assert L.pt_iou_feat_ws_bytes(n, *t3, *t4) > 0
    for (tag, layer, *shape), want in zip(CT.layers(n, t3, t4), CT.PLANS[name]):
        got, Wp = CT.plan(L, *shape)
        assert got == want, f"{name} tower {tag} layer {layer} {shape}: plan {got}, pinned {want}"
        if got is not CT.GEMM:
            ks, br, npg, nb, last, vw, out_vec = got
            H, W = shape[-2:]
            assert nb == -(-H // br) and last == H - (nb - 1) * br and 1 <= last <= br
            assert Wp == (W + 4) // 4 * 4 and br * Wp <= 64 * npg and (br + 2) * W <= 512


@pytest.mark.parametrize("route", list(CT.STRUCTURED))
def test_structured_case_lands_on_its_pinned_plan(L, route):
    n, t3, t4 = CT.STRUCTURED[route]
    assert L.pt_iou_feat_ws_bytes(n, *t3, *t4) > 0
    assert tuple(CT.plan(L, *shape)[0] for _, _, *shape in CT.layers(n, t3, t4)) == CT.STRUCTURED_PLANS[route]


def test_query_refuses_what_the_kernel_does_not_cover(L):
    assert L.pt_mf_corr_tm_plan(1, 16, 64, 3, 170, None) == _lib.PT_ERR_NULL
    for shape in ((1, 16, 64, 2, 171), (1, 24, 64, 4, 4), (1, 16, 40, 4, 4), (1, 16, 64, 0, 4), (1, 0, 64, 4, 4)):
        rc, out = CT.query(L, *shape)
        assert rc == _lib.PT_ERR_UNSUPPORTED and out == [0] * 6, (shape, rc, out)
    rc, out = CT.query(L, 1, 512, 1024, 18, 18)                         # the DiMP-50 classification head
    assert rc == 0 and out[0] >= 1 and out[3] * out[1] >= 18 and out[5] == 20


def _gemm_floor(n, t):
    """Bytes the GEMM route needs at least for a tower: 9 partial maps of the larger layer, the mid map, the token matrix."""
    Cin, Cmid, Cout, H, W = t
    return 4 * n * H * W * (9 * max(Cmid, Cout) + Cmid + 64 * -(-max(Cin, Cmid) // 64))


def test_routes_switch_at_the_widest_banded_row(L):
    tiny = (64, 16, 16, 1, 1)
    for W, banded in ((170, True), (171, False), (172, False)):
        t = (64, 16, 16, 2, W)
        assert (CT.plan(L, 1, 16, 64, 2, W)[0] is not CT.GEMM) == banded and (CT.plan(L, 1, 16, 16, 2, W)[0] is not CT.GEMM) == banded
        ws = L.pt_iou_feat_ws_bytes(1, *t, *tiny)
        assert ws > 0
        # the workspace tells the routes apart: tokens and 9 partial maps on the GEMM route only
        assert (ws < _gemm_floor(1, t)) == banded, (W, ws, _gemm_floor(1, t))


def test_limits_of_batch_map_and_channels(L):
    t = (64, 16, 16, 3, 3)
    assert L.pt_iou_feat_ws_bytes(8, *t, *t) > 0 and L.pt_iou_feat_ws_bytes(9, *t, *t) == 0          # IOU_MAX_N
    assert L.pt_iou_feat_ws_bytes(1, 64, 16, 16, 64, 64, *t) > 0                                      # IOU_MAX_HW
    assert L.pt_iou_feat_ws_bytes(1, 64, 16, 16, 64, 65, *t) == 0 and L.pt_iou_feat_ws_bytes(1, *t, 64, 16, 16, 65, 64) == 0
    assert L.pt_iou_feat_ws_bytes(1, 64, 24, 16, 3, 3, *t) == 0 and L.pt_iou_feat_ws_bytes(1, *t, 64, 40, 16, 3, 3) == 0   # Cmid % 16
    assert L.pt_iou_feat_ws_bytes(1, 64, 48, 16, 3, 3, *t) > 0


def _cells(L):
    """Every named cell of the plan space -> the (case, tower, layer) entries that sit in it, new and existing cases together."""
    hit = {}

    def mark(cell, where):
        hit.setdefault(cell, []).append(where)
    both = dict(synth.IOU_FEAT_CASES)
    assert not set(both) & set(CT.CASES)
    both.update(CT.CASES)
    for name, (n, t3, t4) in both.items():
        routes = set()
        for tag, layer, *shape in CT.layers(n, t3, t4):
            where = (name, tag, layer)
            _, Ftot, C, H, W = shape
            p, Wp = CT.plan(L, *shape)
            routes.add(p is CT.GEMM)
            if p is CT.GEMM:
                mark("gemm", where)
                if n > 1:
                    mark("gemm n>1", where)
                if (H * W) % 4:
                    mark("gemm HW%4!=0", where)
                if C % 64:
                    mark("gemm Cin%64!=0", where)
                continue
            ks, br, npg, nb, last, vw, out_vec = p
            if nb > 1:
                mark(f"npg{npg} vw{vw} {'full' if last == br else 'partial'} last band, nb>1", where)
                if Wp - W == 1:
                    mark("Wp-W==1, nb>1", where)
                if n > 1 and ks > 1:
                    mark("n>1, nb>1, ks>1", where)
            if br == 1 and nb > 1:
                mark("br==1", where)
            mark(f"ks{ks}", where)
            if (C // 16) % ks:
                mark("ks does not divide nch", where)
            if out_vec:
                mark("vector stores", where)
        if len(routes) == 2:
            mark("both routes in one call", (name,))
    return hit


REQUIRED = ([f"npg{npg} vw{vw} {last} last band, nb>1" for npg in (4, 6) for vw in (4, 2) for last in ("full", "partial")]
            + ["npg4 vw1 full last band, nb>1", "npg4 vw1 partial last band, nb>1", "br==1", "Wp-W==1, nb>1",
               "ks1", "ks2", "ks4", "ks8", "ks does not divide nch", "n>1, nb>1, ks>1",
               "gemm n>1", "gemm HW%4!=0", "gemm Cin%64!=0", "both routes in one call"])


@pytest.mark.parametrize("cell", REQUIRED)
def test_cell_is_covered(L, cell):
    hit = _cells(L)
    print(f"\n{cell}: {hit.get(cell, [])}")
    assert hit.get(cell), f"no case runs the cell '{cell}'"


def test_new_cases_alone_run_every_banded_cell_as_full_maps(L):
    """The deployed-size goldens compare a sample of elements; every banded cell is also hit by a case whose whole map is compared."""
    full = dict(_cells(L))
    deployed = {"dimp50", "prdimp50", "atom18"}
    for cell in REQUIRED:
        assert [w for w in full.get(cell, []) if w[0] not in deployed], cell
