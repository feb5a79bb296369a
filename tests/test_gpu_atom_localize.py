"""ATOM's per-frame score localisation on the MI355X (csrc_loc/atom_localize.hip through the C ABI of include/pt_loc.h and through
pytracking_amd.atom_localize) against the float64 run of the numpy restatement (tests/atom_localize_np.py) on the whole case table
(tests/atom_localize_cases.py): no case is excluded -- tests/test_atom_localize_cpu.py asserts that every discrete decision keeps a margin of
16 x the bound below.

Bounds.  Discrete outputs (flag, scale_ind, both peaks' cells, which map is returned) equal the float64 restatement's.  Every float output
-- the (S, G_h, G_w) map the method returns, the map the first peak is found on, both peak values, the translation vector -- lies within
FACTOR x max(ref_err, 2^-23 max|want|) of float64: the bound of tests/f64_bound.py with its ulp_of_max floor, ref_err being the unmodified
reference's own fp32 distance from its float64 run on that case (`ref_fp32_err` of the golden).  The goldens' fp32 outputs are held at the
project's flat 1e-4 as well.  Figures are printed before they are asserted and, when ATOM_LOCALIZE_F64_OUT names a file, written there as
a table (profiles/atom_localize_f64.txt is the table of such a run)."""
import ctypes

import numpy as np
import pytest
import torch

import atom_localize_cases as C
import atom_localize_np as RN
import f64_bound
from f64_bound import dev
from pytracking_amd import _lib_loc as A
from pytracking_amd import atom_localize as AL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# worst ratio of a device output to max(ref_err, ulp of max) measured on the MI355X (profiles/atom_localize_f64.txt)
WORST_MEASURED = 0.56
FACTOR = f64_bound.raised_factor(WORST_MEASURED, C.F_MAX)
TABLE = f64_bound.Table("ATOM_LOCALIZE_F64_OUT",
                        "ATOM per-frame score localisation on the MI355X against float64 (tests/test_gpu_atom_localize.py):\n"
                        "per output max |out - float64| and its ratio to max(ref_err, 2^-23 max|want|) -- the unmodified reference's own fp32\n"
                        f"distance from its float64 run on that case, floored at one fp32 ulp of the output's range; bound = {FACTOR} x that.")
FILL = -7.0


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buffers:
    def __init__(self, case, rec=None):
        S, (Nh, Nw), (Gh, Gw) = len(case["scores"]), case["N"], case["G"]
        self.shape = (S, Nh, Nw, Gh, Gw)
        self.scores = dev(case["scores"])
        self.window = dev(case["window"])
        self.prm = A.LocAtomParams()
        assert A.lib().pt_loc_atom_constants_f32(ctypes.byref(C.state_block(case)), ctypes.byref(self.prm)) == 0
        self.maps = torch.full((S, 1, Gh, Gw), FILL, device=DEV)
        self.maps_hn = torch.full((S, 1, Gh, Gw), FILL, device=DEV) if (self.prm.advanced and self.prm.hn) else None
        self.rec = torch.full((A.PT_AL_REC_FLOATS,), FILL, device=DEV) if rec is None else rec
        self.ws = torch.zeros(A.lib().pt_loc_atom_ws_bytes(*self.shape), dtype=torch.uint8, device=DEV)

    def launch(self, seq=5.0, shape=None):
        p = lambda t: None if t is None else t.data_ptr()
        return A.lib().pt_loc_atom_f32(self.scores.data_ptr(), *(shape or self.shape), p(self.window), ctypes.byref(self.prm), self.maps.data_ptr(),
                                       p(self.maps_hn), self.rec.data_ptr(), seq, self.ws.data_ptr(), self.ws.numel(), stream())

    def outputs(self):
        r = self.rec.cpu().numpy().astype(np.float64)
        cell = lambda k: r[k:k + 2].astype(np.int64)
        which = int(r[A.PT_AL_R_WHICH])
        return dict(flag=int(r[A.PT_AL_R_FLAG]), scale_ind=int(r[A.PT_AL_R_SCALE]), peak1=cell(A.PT_AL_R_ROW1), peak2=cell(A.PT_AL_R_ROW2), which=which,
                    max1=r[A.PT_AL_R_MAX1], max2=r[A.PT_AL_R_MAX2], tv=r[A.PT_AL_R_TV:A.PT_AL_R_TV + 2], pick=int(r[A.PT_AL_R_PICK]), seq=r[A.PT_AL_R_SEQ],
                    map=(self.maps_hn if which else self.maps).cpu().numpy()[:, 0], map_first=self.maps.cpu().numpy()[:, 0])


def hold(name, got, w):
    errs = C.ref_errs(name)
    for q in RN.FLOAT_OUTPUTS + ("map_first",):
        want = np.atleast_1d(np.asarray(w[q], np.float64))
        f64_bound.held("atom_localize_" + name, {q: float(np.abs(np.asarray(got[q], np.float64).reshape(want.shape) - want).max())}, None,
                       errs["map" if q == "map_first" else q], factor=FACTOR, floor=f64_bound.ulp_of_max(want), table=TABLE)


@pytest.mark.parametrize("name", C.CASES)
def test_localisation_through_the_c_abi(name):
    case, w, g = C.CASES[name], C.run(name), C.golden(name)
    b = Buffers(case)
    assert b.launch() == 0
    torch.cuda.synchronize()
    got = b.outputs()
    for k in RN.DISCRETE_OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(w[k])), (name, k, got[k], w[k])
    assert got["seq"] == 5.0 and got["pick"] == (2 if w["branch"] == "hn_second" else 1)
    hold(name, got, w)
    # the unmodified reference's fp32 outputs at the project's flat bound
    si = got["scale_ind"]
    assert got["flag"] == int(g["flag"]) and si == int(g["scale_ind"])
    flat = {"tv": float(np.abs(got["tv"] - g["tv"]).max()), "max of the returned map": abs(float(got["map"][si].max()) - float(g["max1"]))}
    if "map" in g:
        flat["map"] = float(np.abs(got["map"][si] - g["map"]).max())
    print(f"atom_localize_{name}: against the reference's fp32 run " + "  ".join(f"{k} {v:.3e}" for k, v in flat.items()))
    assert max(flat.values()) <= 1e-4, flat
    # the same call again, and with the record in pinned host memory behind the polled wait: the same bits
    b2 = Buffers(case)
    assert b2.launch() == 0
    pinned = torch.zeros(A.PT_AL_REC_FLOATS).pin_memory()
    b3 = Buffers(case, rec=pinned)
    assert b3.launch() == 0 and A.lib().pt_loc_atom_wait_f32(pinned.data_ptr(), 5.0, stream()) == 0
    landed = pinned.numpy().copy()                                             # readable without a stream synchronisation
    torch.cuda.synchronize()
    assert torch.equal(b2.rec, b.rec) and torch.equal(b2.maps, b.maps) and np.array_equal(landed, b.rec.cpu().numpy())
    assert b.maps_hn is None or torch.equal(b2.maps_hn, b.maps_hn)


@pytest.mark.parametrize("name", C.CASES)
def test_localize_through_the_module_equals_the_c_abi(name):
    case, w = C.CASES[name], C.run(name)
    b = Buffers(case)
    assert b.launch() == 0
    torch.cuda.synchronize()
    got = b.outputs()
    r = AL.localize(dev(case["scores"]), C.state_block(case), dev(case["window"]))
    assert r.flag == RN.RETURN_FLAG[w["flag"]] and r.code == w["flag"] and int(r.scale_ind) == w["scale_ind"]
    assert not r.scale_ind.is_cuda and r.scale_ind.dtype == torch.int64 and r.scale_ind.dim() == 0
    assert not r.translation_vec.is_cuda and r.translation_vec.dtype == torch.float32 and r.translation_vec.shape == (2,)
    assert r.scores.is_cuda and r.scores.shape == (len(case["scores"]), 1) + case["G"]
    assert r.peak1 == list(w["peak1"]) and r.peak2 == list(w["peak2"]) and r.pick == got["pick"]
    assert np.array_equal(r.translation_vec.numpy().astype(np.float64), got["tv"]) and r.max1 == got["max1"] and r.max2 == got["max2"]
    assert np.array_equal(r.scores.cpu().numpy()[:, 0], got["map"])


def test_graph_replay_equals_the_eager_call():
    case = C.CASES["n5x6_k3_g40x24_hn"]
    eager = Buffers(case)
    assert eager.launch(seq=3.0) == 0
    torch.cuda.synchronize()
    b = Buffers(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert b.launch(seq=3.0) == 0                                          # warm-up: kernels loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    b.rec.fill_(FILL), b.maps.fill_(FILL), b.maps_hn.fill_(FILL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert b.launch(seq=3.0) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b.rec, eager.rec) and torch.equal(b.maps, eager.maps) and torch.equal(b.maps_hn, eager.maps_hn)


def test_refused_shapes_launch_nothing():
    case = C.CASES["deployed"]
    b = Buffers(case)
    big = torch.full((A.PT_AL_MAX_SCALES + 1, 1, 33, 33), 0.5, device=DEV)       # scores large enough for every refused series size
    b.scores = big
    for what, Nh, Nw, Gh, Gw, S in C.REFUSALS:
        assert b.launch(shape=(S, Nh, Nw, Gh, Gw)) == A.PT_AL_ERR_UNSUPPORTED, what
        assert not AL.covered_shape(S, Nh, Nw, Gh, Gw), what
    torch.cuda.synchronize()
    assert (b.rec == FILL).all() and (b.maps == FILL).all()
    with pytest.raises(NotImplementedError):
        AL.localize(torch.zeros(1, 1, 18, 18, device=DEV), C.state_block(dict(case, G=(19, 19))))
