"""Shared by tests/test_tamos_heads_cpu.py, tests/test_gpu_tamos_heads.py, tools/make_golden_tamos_heads.py and tools/bench_tamos_heads.py:
the shapes that put the TaMOs heads (pt_tamos_bbreg_f32 / pt_fpn2_f32 of pytracking_amd/csrc/tomp.hip, the FPN and DenseBoxRegressor of
pytracking_amd/tamos.py) on every loader mode of the direct 3x3 token convolution and on the sizes where it can go wrong -- a map inside
one 128-row tile with every pixel on the border, an odd width whose pixel count is no multiple of a tile, more than one row tile, a map one
row high, two images with different filters, 1 / 10 / 16 objects, every channel width from 64 to 512, a top-down resize that is no exact
doubling -- next to the workload's own size; with every case the ordered route list the library reports and the fp32 restatement's own
distance from float64 (tests/tamos_heads_f64.py).  Parameters are seeded as tests/tomp_cases.py seeds the regression tower (synth.tomp_params,
so the values in front of `exp` stay moderate); in every case with T >= 3 the middle object's filter is zero.  Reads nothing outside the
repository.  Test infrastructure only."""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from pytracking_amd import _lib, synth

import tamos_cases as TC

# name -> (n_img, T, D, H, W)
REG = OrderedDict([
    ("reg_d64_5x7_t3", (1, 3, 64, 5, 7)),                # the whole map inside one tile, every pixel on the border
    ("reg_d128_9x13_t1", (1, 1, 128, 9, 13)),            # odd width, HW = 117 no multiple of any tile
    ("reg_d128_9x13_t10", (1, 10, 128, 9, 13)),
    ("reg_d256_12x18_t16", (1, 16, 256, 12, 18)),        # two row tiles per image, the second ragged; the full object count
    ("reg_d512_6x6_t2", (1, 2, 512, 6, 6)),
    ("reg_d64_1x40_t2", (1, 2, 64, 1, 40)),              # a map one row high
    ("reg_d128_5x7_t3_n2", (2, 3, 128, 5, 7)),           # two images with different filters
    ("reg_deployed", (1, 10, 256, 48, 72)),              # the workload: 34 560 token rows per tower layer
])
# name -> (n, C_hi, C_lo, D, H3, W3, H2, W2)
FPN = OrderedDict([
    ("fpn_x2", (1, 128, 64, 64, 5, 7, 10, 14)),          # exact doubling
    ("fpn_odd", (2, 128, 64, 64, 5, 7, 9, 13)),          # not a multiple: the nearest index rule; two images
    ("fpn_d256", (1, 512, 256, 256, 6, 9, 12, 18)),
    ("fpn_deployed", (1, 512, 256, 256, 24, 36, 48, 72)),
])
# FPN -> regressor through the two Python classes: (FPN case, T)
CHAIN = OrderedDict([("chain_odd_t3", ("fpn_odd", 3))])
REG_DEPLOYED, FPN_DEPLOYED = "reg_deployed", "fpn_deployed"
SMALL_REG = [n for n in REG if n != REG_DEPLOYED]
SMALL_FPN = [n for n in FPN if n != FPN_DEPLOYED]
PARAM_SEED, INPUT_SEED = 9300, 9400               # + 10 x the case's position in its table
DEPLOYED_KEEP = {"ltrb": 7, "feat2": 37, "feat3": 11}      # the deployed cases' goldens keep every k-th element of the flattened output

R = _lib.TOMP_ROUTES
RT = _lib.HEADS_ROUTES
compress = TC.compress


def expand(text):
    """tests/tamos_cases.py's N*[ block ] notation over the shared launchers' and the heads' route names"""
    out, stack = [], []
    for tok in text.split():
        if tok.endswith("*["):
            stack.append((int(tok[:-2]), len(out)))
        elif tok == "]":
            n, at = stack.pop()
            out += out[at:] * (n - 1)
        else:
            assert tok in R or tok in RT, tok
            out.append(tok)
    assert not stack
    return tuple(out)


def route_name(v):
    if 0 < v < len(R):
        return R[v]
    assert _lib.HEADS_ROUTE_BASE <= v < _lib.HEADS_ROUTE_BASE + len(RT), v
    return RT[v - _lib.HEADS_ROUTE_BASE]

# The pinned routes, in launch order: written by `python tests/tamos_heads_f64.py` from pt_tamos_bbreg_routes / pt_fpn2_routes.
ROUTES_TEXT = {
    "reg_d64_5x7_t3": "HEADS_NCHW_TOKENS 2*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_d128_9x13_t1": "HEADS_NCHW_TOKENS 2*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_d128_9x13_t10": "HEADS_NCHW_TOKENS 2*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_d256_12x18_t16": "HEADS_NCHW_TOKENS 2*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_d512_6x6_t2": "HEADS_NCHW_TOKENS 2*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_d64_1x40_t2": "HEADS_NCHW_TOKENS 2*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_d128_5x7_t3_n2": "HEADS_NCHW_TOKENS 3*[ GEMM_T32 ] HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "reg_deployed": "HEADS_NCHW_TOKENS GEMM_T32 GEMM_T32_SWZ_PAD HEADS_CONV3_ROWSCALE 3*[ HEADS_CONV3_GN_FINISH HEADS_CONV3_GN ] HEADS_CONV3_GN_FINISH HEADS_REG_OUT",
    "fpn_x2": "2*[ HEADS_NCHW_TOKENS ] 2*[ GEMM_T32 ] HEADS_CONV3_UPADD HEADS_CONV3_PLAIN",
    "fpn_odd": "2*[ HEADS_NCHW_TOKENS ] 2*[ GEMM_T32 ] HEADS_CONV3_UPADD HEADS_CONV3_PLAIN",
    "fpn_d256": "2*[ HEADS_NCHW_TOKENS ] 2*[ GEMM_T32 ] HEADS_CONV3_UPADD HEADS_CONV3_PLAIN",
    "fpn_deployed": "2*[ HEADS_NCHW_TOKENS ] 2*[ GEMM_T32_SWZ_PAD ] HEADS_CONV3_UPADD HEADS_CONV3_PLAIN",
}
ROUTES = {name: expand(text) for name, text in ROUTES_TEXT.items()}

# max |fp32 restatement - float64 restatement| over the outputs of a case (tests/tamos_heads_f64.py), as measured on the CPU the table was
# written on
REF_ERR = {
    "reg_d64_5x7_t3": 6.239e-07,
    "reg_d128_9x13_t1": 4.902e-07,
    "reg_d128_9x13_t10": 7.676e-07,
    "reg_d256_12x18_t16": 1.570e-06,
    "reg_d512_6x6_t2": 1.138e-06,
    "reg_d64_1x40_t2": 2.827e-07,
    "reg_d128_5x7_t3_n2": 5.072e-07,
    "reg_deployed": 1.063e-06,
    "fpn_x2": 1.488e-06,
    "fpn_odd": 1.646e-06,
    "fpn_d256": 2.912e-06,
    "fpn_deployed": 3.410e-06,
    "chain_odd_t3": 1.646e-06,
}


def _query(fn, *args):
    cap = _lib.PT_TAMOS_MAX_ROUTES
    out = (ctypes.c_int * cap)(*([-1] * cap))
    n = ctypes.c_int(-1)
    rc = fn(*args, out, cap, ctypes.byref(n))
    if rc != 0:
        assert n.value == 0 and not any(out), (rc, n.value)
        return rc, ()
    assert 0 < n.value <= cap and not any(out[n.value:])
    return rc, tuple(route_name(v) for v in out[:n.value])


def reg_routes(L, n_img, T, D, H, W):
    return _query(L.pt_tamos_bbreg_routes, n_img, T, D, H, W)


def fpn_routes(L, n, C_hi, C_lo, D, H3, W3, H2, W2, want_feat3=1):
    return _query(L.pt_fpn2_routes, n, C_hi, C_lo, D, H2, W2, H3, W3, want_feat3)


def case_routes(L, name):
    return reg_routes(L, *REG[name]) if name in REG else fpn_routes(L, *FPN[name])


_CACHE = {}


def _freeze(*arrays):
    for v in arrays:
        v.setflags(write=False)


def reg_params(D, seed):
    return {q[4:]: v for q, v in synth.tomp_params(seed, dict(D=D, nhead=1, ff=64, n_enc=0, n_dec=0)).items() if q.startswith("reg.")}


def reg_case(name):
    """(params {reference key: fp32}, feat (n_img, D, H, W), filters (n_img, T, D)); the middle object's filter is zero when T >= 3."""
    if name not in _CACHE:
        n_img, T, D, H, W = REG[name]
        k = list(REG).index(name)
        params = reg_params(D, PARAM_SEED + 10 * k)
        rng = np.random.default_rng(INPUT_SEED + 10 * k)
        feat = rng.standard_normal((n_img, D, H, W), dtype=np.float32) * np.float32(4.0 / np.sqrt(D))
        filt = rng.standard_normal((n_img, T, D), dtype=np.float32)
        for a in TC.absent_objects(T):
            filt[:, a] = 0
        _freeze(feat, filt, *params.values())
        _CACHE[name] = (params, feat, filt)
    return _CACHE[name]


def fpn_case(name):
    """(params {'fpn.' + torchvision key: fp32}, feat_hi (n, C_hi, H2, W2), feat_lo (n, C_lo, H3, W3))"""
    if name not in _CACHE:
        n, C_hi, C_lo, D, H3, W3, H2, W2 = FPN[name]
        k = list(FPN).index(name)
        rng = np.random.default_rng(PARAM_SEED + 500 + 10 * k)
        g = lambda *s, scale: rng.standard_normal(s, dtype=np.float32) * np.float32(scale)
        params = OrderedDict()
        for i, C in enumerate((C_hi, C_lo)):
            params[f"fpn.inner_blocks.{i}.0.weight"] = g(D, C, 1, 1, scale=1 / np.sqrt(C))
            params[f"fpn.inner_blocks.{i}.0.bias"] = g(D, scale=0.1)
        for i in range(2):
            params[f"fpn.layer_blocks.{i}.0.weight"] = g(D, D, 3, 3, scale=1 / np.sqrt(9 * D))
            params[f"fpn.layer_blocks.{i}.0.bias"] = g(D, scale=0.1)
        rng = np.random.default_rng(INPUT_SEED + 500 + 10 * k)
        hi = rng.standard_normal((n, C_hi, H2, W2), dtype=np.float32)
        lo = rng.standard_normal((n, C_lo, H3, W3), dtype=np.float32)
        _freeze(hi, lo, *params.values())
        _CACHE[name] = (params, hi, lo)
    return _CACHE[name]


def chain_case(name):
    """(FPN case name, regressor params, filters (n, T, D)) of an FPN -> regressor chain"""
    if name not in _CACHE:
        fname, T = CHAIN[name]
        n, D = FPN[fname][0], FPN[fname][3]
        k = list(CHAIN).index(name)
        params = reg_params(D, PARAM_SEED + 800 + 10 * k)
        filt = np.random.default_rng(INPUT_SEED + 800 + 10 * k).standard_normal((n, T, D), dtype=np.float32) * np.float32(0.25)
        for a in TC.absent_objects(T):
            filt[:, a] = 0
        _freeze(filt, *params.values())
        _CACHE[name] = (fname, params, filt)
    return _CACHE[name]


def to_sd(params):
    return {k: torch.from_numpy(v.copy()) for k, v in params.items()}


def build_regressor(D, params, device):
    from pytracking_amd import tamos as TA
    reg = TA.DenseBoxRegressor(num_channels=D)
    reg.load_state_dict(to_sd(params), strict=True)
    return reg.to(device).eval()


def build_fpn(name, params, device):
    from pytracking_amd import tamos as TA
    _, C_hi, C_lo, D = FPN[name][:4]
    m = TA.FPN(output_dim=D, input_dims=(C_hi, C_lo))
    m.load_state_dict(to_sd(params), strict=True)
    return m.to(device).eval()
