"""Shared by tests/test_corr_tm_plans_cpu.py and tests/test_gpu_corr_tm_plans.py: shapes that put the banded tap-major 3x3 correlation
(k_mf_corr<9, VW, true, NPG>, pt_launch_mf_corr_tm) and the GEMM route of iou_feat.hip on every plan the host can pick -- band height,
8 or 12 waves, channel splits, staging width, store mode, partial last band -- each run through pytracking_amd.iou_feat.get_iou_feat on
iou_feat_cases.Towers.  Next to every case stands the plan its four convolutions must land on (pt_mf_corr_tm_plan), so that a change of
the cost model cannot move a case off the cell it is there for without the CPU suite saying so.  Test infrastructure only."""
import ctypes

import numpy as np
import torch

import iou_feat_cases as IC
from pytracking_amd import _lib, synth

GEMM = None                                   # a layer the banded kernel does not cover: iou_feat.hip's per-tap GEMM route

# name: (n, (Cin, Cmid, Cout, H, W) of tower 3, the same of tower 4).  Layer 1 of a tower is Cin -> Cmid, layer 2 Cmid -> Cout.
CASES = {
    "w170": (1, (64, 16, 16, 3, 170), (64, 16, 16, 24, 168)),         # the widest banded row: every row its own band
    "odd_bands": (1, (64, 16, 16, 9, 83), (64, 16, 16, 3, 127)),      # scalar staging, one zero dword between rows, several bands
    "max_map": (1, (64, 16, 16, 64, 64), (128, 16, 16, 10, 50)),      # H * W = 4096: 22 bands; 8 splits with a partial band
    "w12_vec4": (1, (64, 16, 256, 17, 128), (64, 16, 256, 18, 128)),  # layer 2: 12 waves, 16-byte staging, partial and full last band
    "w12_vec2": (3, (64, 16, 256, 11, 86), (64, 80, 32, 7, 23)),      # layer 2: 12 waves, 8-byte staging, n = 3; 5 chunks in 2 splits
    "w12_even": (2, (64, 16, 256, 18, 86), (64, 16, 16, 2, 6)),       # layer 2: 12 waves, 8-byte staging, full last band
    "pairs": (2, (64, 16, 16, 7, 62), (64, 16, 16, 2, 171)),          # n = 2 across bands and splits + a GEMM tower, H * W % 4 == 2
    "n5": (5, (64, 112, 16, 6, 10), (64, 16, 16, 13, 27)),            # 7 chunks in 4 splits; scalar staging, bands of 7 + 6, n = 5
    "n8": (8, (64, 16, 16, 3, 3), (64, 16, 16, 1, 200)),              # the largest batch on both routes
    "gemm_n3": (3, (64, 48, 16, 3, 171), (64, 64, 32, 2, 172)),       # GEMM route, n = 3: padded weights (Cin 48), odd H * W; Cin 64
}

# name: the plans of (tower 3 layer 1, tower 3 layer 2, tower 4 layer 1, tower 4 layer 2), each
# (ks, br, npg, nb, rows of the last band, vw, out_vec) or GEMM
PLANS = {
    "w170": ((4, 1, 4, 3, 1, 2, 0), (1, 1, 4, 3, 1, 2, 0), (4, 1, 4, 24, 1, 4, 1), (1, 1, 4, 24, 1, 4, 1)),
    "odd_bands": ((4, 3, 4, 3, 3, 1, 0), (1, 3, 4, 3, 3, 1, 0), (4, 2, 4, 2, 1, 1, 0), (1, 2, 4, 2, 1, 1, 0)),
    "max_map": ((4, 3, 4, 22, 1, 4, 1), (1, 3, 4, 22, 1, 4, 1), (8, 4, 4, 3, 2, 2, 0), (1, 4, 4, 3, 2, 2, 0)),
    "w12_vec4": ((4, 1, 4, 17, 1, 4, 1), (1, 2, 6, 9, 1, 4, 1), (4, 1, 4, 18, 1, 4, 1), (1, 2, 6, 9, 2, 4, 1)),
    "w12_vec2": ((4, 2, 4, 6, 1, 2, 0), (1, 3, 6, 4, 2, 2, 0), (4, 7, 4, 1, 7, 1, 0), (2, 7, 4, 1, 7, 1, 0)),
    "w12_even": ((4, 2, 4, 9, 2, 2, 0), (1, 3, 6, 6, 3, 2, 0), (4, 2, 4, 1, 2, 2, 0), (1, 2, 4, 1, 2, 2, 0)),
    "pairs": ((4, 4, 4, 2, 3, 2, 0), (1, 4, 4, 2, 3, 2, 0), GEMM, GEMM),
    "n5": ((4, 6, 4, 1, 6, 2, 0), (4, 6, 4, 1, 6, 2, 0), (4, 7, 4, 2, 6, 1, 0), (1, 7, 4, 2, 6, 1, 0)),
    "n8": ((4, 3, 4, 1, 3, 1, 0), (1, 3, 4, 1, 3, 1, 0), GEMM, GEMM),
    "gemm_n3": (GEMM, GEMM, GEMM, GEMM),
}
STATE_SEED, INPUT_SEED = 7100, 7200          # + the case's position in CASES
_CACHE = {}


def layers(n, t3, t4):
    """[(tower tag, layer, n, Cout, Cin, H, W)] of the four convolutions of a call, in PLANS order."""
    return [(tag, l + 1, n, t[l + 1], t[l], t[3], t[4]) for tag, t in (("3", t3), ("4", t4)) for l in range(2)]


def query(L, n, Ftot, C, H, W):
    """(status, [ks, br, npg, nb, last, Wp]) of pt_mf_corr_tm_plan."""
    out = (ctypes.c_int * 6)(*([-1] * 6))
    rc = L.pt_mf_corr_tm_plan(n, Ftot, C, H, W, out)
    return rc, list(out)


def plan(L, n, Ftot, C, H, W):
    """(ks, br, npg, nb, last, vw, out_vec) the launcher runs for 16-byte aligned contiguous operands, GEMM when the banded kernel does
    not cover the shape; Wp as the second value.  vw and out_vec as pt_launch_mf_corr_tm derives them (mf_vec_width)."""
    rc, (ks, br, npg, nb, last, Wp) = query(L, n, Ftot, C, H, W)
    if rc != 0:
        assert rc == _lib.PT_ERR_UNSUPPORTED and (ks, br, npg, nb, last, Wp) == (0,) * 6, (rc, ks, br, npg, nb, last, Wp)
        return GEMM, 0
    vw = 4 if W % 4 == 0 else 2 if W % 2 == 0 else 1
    return (ks, br, npg, nb, last, vw, int(vw == 4 and (H * W) % 4 == 0)), Wp


def case(name):
    """(n, tower3, tower4, state dict (numpy), (feat3, feat4) (numpy)), generated once per session."""
    key = ("case", name)
    if key not in _CACHE:
        n, t3, t4 = CASES[name]
        k = list(CASES).index(name)
        sd = synth.iou_feat_state(STATE_SEED + k, t3[0], t4[0], t3[1], t3[2], t4[1], t4[2])
        feats = synth.iou_feat_inputs(INPUT_SEED + k, n, t3[0], t3[3], t3[4], t4[0], t4[3], t4[4])
        _CACHE[key] = (n, t3, t4, sd, feats)
    return _CACHE[key]


def module(name, device="cpu", dtype=torch.float32):
    n, t3, t4, sd, _ = case(name)
    net = IC.Towers(t3, t4)
    net.load_state_dict(IC.state_tensors(sd))
    return net.to(device=device, dtype=dtype).eval()


def run_cpu(net, feats, dtype):
    with torch.no_grad():
        out = net.to(dtype).get_iou_feat([torch.from_numpy(np.ascontiguousarray(f)).to(dtype) for f in feats])
    return [o.double().numpy() for o in out]


def reference(name):
    """((c3, c4) of the float64 module on the CPU, max |fp32 CPU module - float64|), computed once per session and never written to."""
    key = ("ref", name)
    if key not in _CACHE:
        _, _, _, _, feats = case(name)
        ref = run_cpu(module(name), feats, torch.float64)
        f32 = run_cpu(module(name), feats, torch.float32)
        for r in ref:
            r.setflags(write=False)
        _CACHE[key] = (ref, max(float(np.abs(a - b).max()) for a, b in zip(f32, ref)))
    return _CACHE[key]


# ---- structured inputs: one-hot maps against weights whose taps are distinct powers of two (every value an exact small integer)
STRUCTURED_PLANS = {
    "banded": ((4, 3, 4, 3, 3, 1, 0), (1, 3, 4, 3, 3, 1, 0), (4, 2, 4, 9, 2, 2, 0), (1, 3, 6, 6, 3, 2, 0)),
    "gemm": (GEMM, GEMM, GEMM, GEMM),
}
STRUCTURED = {                                # one call per route, n = 2 so that the image index shows
    "banded": (2, (64, 16, 16, 9, 83), (64, 16, 256, 18, 86)),        # scalar staging, bands of 3, one zero dword; bands of 2, then of 3 on 12 waves
    "gemm": (2, (64, 48, 16, 3, 171), (64, 16, 16, 2, 172)),
}


def hot_spots(H, W, band_rows):
    """The four corners, and for every band height in `band_rows` the last row of a band and the first row of the next one (the boundary
    nearest the middle of the map) at the first, a middle and the last column."""
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for br in band_rows:
        nb = (H + br - 1) // br
        b = br * max(nb // 2, 1)                                        # first row of an interior band
        for y in (b - 1, b):
            if 0 <= y < H:
                pts += [(y, 0), (y, W // 2), (y, W - 1)]
    return list(dict.fromkeys(pts))


def structured_input(n, C, H, W, pts):
    """Channel c of image i is one-hot at pts[(c + 3 i) % len(pts)]."""
    x = np.zeros((n, C, H, W), np.float32)
    for i in range(n):
        for c in range(C):
            y, xx = pts[(c + 3 * i) % len(pts)]
            x[i, c, y, xx] = 1.0
    return x


def structured_module(t3, t4):
    """Towers whose blocks are exact: tap (u, v) of every live weight is 2^(3u + v), output channel o of a layer reads the input channels
    c with c % 16 == o % 16 in layer 1 (one per 16-channel chunk, so every channel split contributes) and the single channel o % Cmid in
    layer 2; bias 0 and BatchNorm the identity (eps = 2^-60: 1 + eps == 1 in float64, the scale is exactly 1).  A one-hot map meets one tap per position: layer 1 yields integers <= 4 * 256,
    layer 2 <= 9 * 256 * 1024 < 2^24, exact in fp32 in any summation order."""
    net = IC.Towers(t3, t4)
    taps = torch.tensor([[2.0 ** (3 * u + v) for v in range(3)] for u in range(3)])
    with torch.no_grad():
        for blk, first in ((net.conv3_1t, True), (net.conv3_2t, False), (net.conv4_1t, True), (net.conv4_2t, False)):
            conv, bn = blk[0], blk[1]
            conv.weight.zero_()
            conv.bias.zero_()
            for o in range(conv.out_channels):
                src = range(o % 16, conv.in_channels, 16) if first else [o % conv.in_channels]
                for c in src:
                    conv.weight[o, c] = taps
            bn.weight.fill_(1.0); bn.bias.zero_(); bn.running_mean.zero_(); bn.running_var.fill_(1.0)
            bn.eps = 2.0 ** -60
    return net.eval()
