"""Shared by tests/test_tomp_routes_cpu.py and tests/test_gpu_tomp_routes.py: configurations that put the ToMP model predictor
(pytracking_amd/csrc/tomp.hip, mfma_gemm.h, pytracking_amd/transformer.py) on every kernel route its launchers can pick -- launch_gemm,
launch_ln_rows, launch_gemv, the k_attn<HD> switch, the fused / unfused GroupNorm tower -- and on the shapes where its kernels change
path without the launcher knowing: more than two batch rows, fully masked leading key tiles, an empty mask range, odd split-K slices,
phantom row tiles, the LDS limit of k_dec_ctx and its long-row softmax, no encoder / no decoder.  Next to every case stands the ordered
route list the host-only queries (pt_tomp_predict_routes, pt_tomp_bbreg_routes, pt_tomp_linear_routes) report for it, and the fp32
oracle's own distance from float64 on it (tests/tomp_f64.py), so that a change of a dispatcher cannot move a case off the route it is
there for without the CPU suite saying so.  Reads nothing outside the repository.  Test infrastructure only."""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from pytracking_amd import _lib, synth

R = _lib.TOMP_ROUTES


def _p(D, nhead, ff, H, W, n_train, mode, n_seq=1, gth=0, n_enc=1, n_dec=1):
    """A predictor case: `mode` 'parallel' (predict_cls_bbreg_filters_parallel + classifier + box regressor, one sequence, memory
    frames [gth, n_train) masked for the bbreg row) or 'filter' (predict_filter on n_seq sequences)."""
    assert mode in ("parallel", "filter") and (mode == "filter" or n_seq == 1)
    return dict(D=D, nhead=nhead, ff=ff, n_enc=n_enc, n_dec=n_dec, H=H, W=W, feature_sz=max(H, W), n_train=n_train,
                num_gth_frames=gth, mode=mode, n_seq=n_seq)


# rows = batch rows x (n_train + 1) x H x W tokens; parallel = 2 batch rows
PREDICT = OrderedDict([
    # ---- the deployed size, both entry points (the only large cases)
    ("deployed_par", dict(synth.TOMP, mode="parallel", n_seq=1)),
    ("deployed_filter", dict(synth.TOMP, mode="filter", n_seq=1)),
    # ---- D x head width x dim_ff at 5x7 (210 rows: plain 32 x 32 tiles), two layers each so that the decoder's GEMVs run live
    ("d128_h16_ff256", _p(128, 8, 256, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d128_h32_ff320", _p(128, 4, 320, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d128_h64_ff768", _p(128, 2, 768, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d256_h16_ff320", _p(256, 16, 320, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d256_h32_ff768", _p(256, 8, 768, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d256_h64_ff256", _p(256, 4, 256, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d384_h32_ff256", _p(384, 12, 256, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d384_h64_ff768", _p(384, 6, 768, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d512_h32_ff320", _p(512, 16, 320, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    ("d512_h64_ff768", _p(512, 8, 768, 5, 7, 2, "parallel", gth=1, n_enc=2, n_dec=2)),
    # ---- more than two batch rows: blockIdx.z / y >= 2 of k_attn / k_dec_*, k_gemv<4> / k_gemv<1> with B > 2
    ("seq3_d256", _p(256, 8, 256, 5, 5, 1, "filter", n_seq=3, n_dec=2)),
    ("seq5_d256", _p(256, 8, 256, 5, 5, 1, "filter", n_seq=5, n_dec=2)),
    ("seq8_d256", _p(256, 8, 256, 5, 5, 1, "filter", n_seq=8, n_dec=2)),
    ("seq3_d128", _p(128, 4, 256, 5, 5, 1, "filter", n_seq=3, n_dec=2)),
    ("seq5_d128", _p(128, 4, 256, 5, 5, 1, "filter", n_seq=5, n_dec=2)),
    ("seq8_d128", _p(128, 4, 256, 5, 5, 1, "filter", n_seq=8, n_dec=2)),
    # ---- rows >= 1024 at D = 256: 16x16, one memory frame, parallel = 1024 rows exactly; split-K slices of 1, 3 and 4 stages, the
    #      fallback FFN2 with a K tail (ff 320), FFN1 on 128 x 64 tiles (ff >= 1024), rows that are no multiple of 128 (18x18: 1296)
    ("m1024_ff256", _p(256, 8, 256, 16, 16, 1, "parallel")),
    ("m1024_ff768", _p(256, 8, 768, 16, 16, 1, "parallel")),
    ("m1024_ff1024", _p(256, 8, 1024, 16, 16, 1, "parallel")),
    ("m1024_ff320", _p(256, 8, 320, 16, 16, 1, "parallel")),
    ("m1296_ff1280", _p(256, 8, 1280, 18, 18, 1, "parallel")),
    # ---- rows >= 1024 at D != 256: QKV on swizzled 32 x 32 tiles with "+pos" (D 128) or k_gemm_ps<2> (D 384 / 512), FFN2 + residual on
    #      32 x 32 tiles, the generic LayerNorm on many rows
    ("m1024_d128", _p(128, 4, 256, 16, 16, 1, "parallel")),
    ("m1024_d384", _p(384, 6, 768, 16, 16, 1, "parallel")),
    ("m1024_d512", _p(512, 8, 1024, 16, 16, 1, "parallel")),
    # ---- swizzled 32 x 32 tiles whose last group of 8 row tiles is partly phantom: 7x19, 532 rows = 17 row tiles
    ("swz_pad_532", _p(128, 4, 256, 7, 19, 1, "parallel")),
    # ---- masks over more than one 64-key tile (9x9: 81 keys per frame): the bbreg row's first key tiles fully masked (gth 0), the
    #      deployed pattern (gth 1), an empty mask range (gth = n_train); again at D = 256 on 16x16 maps (1536 rows)
    ("mask9_gth0", _p(128, 4, 256, 9, 9, 2, "parallel", gth=0)),
    ("mask9_gth1", _p(128, 4, 256, 9, 9, 2, "parallel", gth=1)),
    ("mask9_gth2", _p(128, 4, 256, 9, 9, 2, "parallel", gth=2)),
    ("mask16_gth0", _p(256, 8, 256, 16, 16, 2, "parallel", gth=0)),
    ("mask16_gth1", _p(256, 8, 256, 16, 16, 2, "parallel", gth=1)),
    ("mask16_gth2", _p(256, 8, 256, 16, 16, 2, "parallel", gth=2)),
    # ---- k_dec_ctx: on the LDS limit nhead (L + 4) <= 11000 with L % 16 != 0 (L = 1368), and rows of more than 1408 scores (two heads:
    #      the strided softmax passes instead of the register-resident one)
    ("lds_limit", _p(256, 8, 256, 18, 19, 3, "filter")),
    ("long_scores", _p(128, 2, 256, 22, 22, 2, "filter")),
    # ---- no encoder / no decoder / neither
    ("enc0_dec1", _p(128, 4, 256, 5, 7, 2, "parallel", gth=1, n_enc=0, n_dec=1)),
    ("enc1_dec0", _p(128, 4, 256, 5, 7, 2, "parallel", gth=1, n_enc=1, n_dec=0)),
    ("enc0_dec0", _p(128, 4, 256, 5, 7, 2, "parallel", gth=1, n_enc=0, n_dec=0)),
])
DEPLOYED = ("deployed_par", "deployed_filter")

# DenseBoxRegressor alone: name -> (n images, D, H, W).  HW < 32 and more than 256 GroupNorm slices per image (H W D > 262144) take the
# unfused tower (k_gn_apply)
BBREG = OrderedDict((f"reg_d{D}_{H}x{W}_n{n}", (n, D, H, W)) for D, H, W in
                    ((64, 6, 6), (128, 5, 5), (256, 5, 7), (384, 6, 6), (512, 6, 6), (512, 23, 23)) for n in (1, 3))

# pt_tomp_linear_f32 alone: name -> (B, N, K, bias, relu)
LINEAR = OrderedDict((f"lin_b{B}_n{N}_k{K}_{'b' if bias else 'nb'}{'_relu' if relu else ''}", (B, N, K, bias, relu))
                     for B, N, K in ((2, 258, 256), (3, 514, 512), (8, 130, 192), (1, 4, 64), (8, 2048, 768))
                     for bias in (False, True) for relu in (False, True))

PARAM_SEED, INPUT_SEED = 8100, 8200           # + 10 x the case's position in its table (+ the sequence)


# ------------------------------------------------------------------------------------------------------------------
# the pinned routes, in launch order.  "N*[a b]" stands for N repetitions of "a b" (encoder / decoder layers, tower layers).
# Written by `python tests/tomp_f64.py` from the queries, then read against the dispatchers: the comments say what each case is there for.
# ------------------------------------------------------------------------------------------------------------------
def expand(text):
    out, stack = [], []
    for tok in text.split():
        if tok.endswith("*["):
            stack.append((int(tok[:-2]), len(out)))
        elif tok == "]":
            n, at = stack.pop()
            out += out[at:] * (n - 1)
        else:
            assert tok in R, tok
            out.append(tok)
    assert not stack
    return tuple(out)


def compress(names):
    """The shortest-first greedy inverse of expand(): immediate repetitions of a block of up to 12 names become N*[block]."""
    names, out, i = list(names), [], 0
    while i < len(names):
        best = (1, 1)
        for w in range(1, 13):
            n = 1
            while names[i + n * w:i + (n + 1) * w] == names[i:i + w]:
                n += 1
            if n > 1 and n * w > best[0] * best[1]:
                best = (n, w)
        n, w = best
        out.append(names[i] if n == 1 else f"{n}*[ " + compress(names[i:i + w]) + " ]")
        i += n * w
    return " ".join(out)


ROUTES_TEXT = {
    "deployed_par": "TOKENS BOX1 2*[ GEMM_T32_SWZ_PAD ] 6*[ GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ_PAD LN256 GEMM_PS4_WIDE GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 ] DEC0_CONST 5*[ DEC_SCORES DEC_CTX 2*[ GEMV_DEC8 GEMV_DEC1 ] GEMV_DEC1 ] DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_DEC8 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "deployed_filter": "TOKENS BOX1 3*[ GEMM_T32_SWZ_PAD ] 5*[ ATTN32 2*[ GEMM_T32_SWZ_PAD LN256 GEMM_T32_SWZ_PAD ] ] ATTN32 GEMM_T32_SWZ_PAD LN256 2*[ GEMM_T32_SWZ_PAD ] LN256 DEC0_CONST 5*[ DEC_SCORES DEC_CTX 2*[ GEMV_DEC8 GEMV_DEC1 ] GEMV_DEC1 ] DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_DEC8 LN256_DOUBLE TO_NCHW",
    "d128_h16_ff256": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN16 2*[ GEMM_T32 LN128 GEMM_T32 ] ATTN16 GEMM_T32 LN128 2*[ GEMM_T32 ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d128_h32_ff320": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ATTN32 GEMM_T32 LN128 2*[ GEMM_T32 ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d128_h64_ff768": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN64 2*[ GEMM_T32 LN128 GEMM_T32 ] ATTN64 GEMM_T32 LN128 2*[ GEMM_T32 ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d256_h16_ff320": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN16 2*[ GEMM_T32 LN256 GEMM_T32 ] ATTN16 GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 DEC0_CONST DEC_SCORES DEC_CTX GEMV_V4 GEMV_DEC1 GEMV_V1 2*[ GEMV_DEC1 ] DEC_SCORES DEC_CTX GEMV_V4 GEMV_DEC1 GEMV_V1 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d256_h32_ff768": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 2*[ GEMM_T32 LN256 GEMM_T32 ] ATTN32 GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_V4 2*[ GEMV_DEC1 ] DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_V4 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d256_h64_ff256": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN64 2*[ GEMM_T32 LN256 GEMM_T32 ] ATTN64 GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC4 4*[ GEMV_DEC1 ] DEC_SCORES DEC_CTX GEMV_DEC4 2*[ GEMV_DEC1 ] LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d384_h32_ff256": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 2*[ GEMM_T32 LN_GENERIC GEMM_T32 ] ATTN32 GEMM_T32 LN_GENERIC 2*[ GEMM_T32 ] LN_GENERIC DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN_GENERIC ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d384_h64_ff768": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN64 2*[ GEMM_T32 LN_GENERIC GEMM_T32 ] ATTN64 GEMM_T32 LN_GENERIC 2*[ GEMM_T32 ] LN_GENERIC DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN_GENERIC ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d512_h32_ff320": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 2*[ GEMM_T32 LN_GENERIC GEMM_T32 ] ATTN32 GEMM_T32 LN_GENERIC 2*[ GEMM_T32 ] LN_GENERIC DEC0_CONST DEC_SCORES DEC_CTX GEMV_V4 GEMV_DEC2 GEMV_V1 2*[ GEMV_DEC2 ] DEC_SCORES DEC_CTX GEMV_V4 GEMV_DEC2 GEMV_V1 2*[ LN_GENERIC ] TO_NCHW 2*[ GEMV_DEC2 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "d512_h64_ff768": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN64 2*[ GEMM_T32 LN_GENERIC GEMM_T32 ] ATTN64 GEMM_T32 LN_GENERIC 2*[ GEMM_T32 ] LN_GENERIC DEC0_CONST DEC_SCORES DEC_CTX 2*[ GEMV_V4 GEMV_DEC2 ] GEMV_DEC2 DEC_SCORES DEC_CTX GEMV_V4 GEMV_DEC2 GEMV_V4 2*[ LN_GENERIC ] TO_NCHW 2*[ GEMV_DEC2 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "seq3_d256": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V4 ] DEC_SCORES DEC_CTX 3*[ GEMV_V4 ] LN256_DOUBLE TO_NCHW",
    "seq5_d256": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V4 ] DEC_SCORES DEC_CTX 3*[ GEMV_V4 ] LN256_DOUBLE TO_NCHW",
    "seq8_d256": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V4 ] DEC_SCORES DEC_CTX 3*[ GEMV_V4 ] LN256_DOUBLE TO_NCHW",
    "seq3_d128": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN128 2*[ GEMM_T32 ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW",
    "seq5_d128": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN128 2*[ GEMM_T32 ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW",
    "seq8_d128": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN128 2*[ GEMM_T32 ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 5*[ GEMV_V1 ] DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW",
    "m1024_ff256": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 GEMM_T32_SWZ GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 2*[ GEMV_DEC1 ] LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1024_ff768": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 GEMM_T32_SWZ GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_V4 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1024_ff1024": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 GEMM_PS4_WIDE GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_DEC4 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1024_ff320": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 2*[ GEMM_T32_SWZ ] LN256 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_V1 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1296_ff1280": "TOKENS BOX1 2*[ GEMM_T32_SWZ_PAD ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ_PAD LN256 GEMM_PS4_WIDE GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 GEMV_DEC1 GEMV_V4 LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1024_d128": "TOKENS BOX1 3*[ GEMM_T32_SWZ ] ATTN32 GEMM_T32_SWZ LN128 2*[ GEMM_T32_SWZ ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1024_d384": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN64 GEMM_T32_SWZ LN_GENERIC 2*[ GEMM_T32_SWZ ] LN_GENERIC DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN_GENERIC ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "m1024_d512": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN64 GEMM_T32_SWZ LN_GENERIC GEMM_PS4_WIDE GEMM_T32_SWZ LN_GENERIC DEC0_CONST DEC_SCORES DEC_CTX GEMV_V4 GEMV_DEC2 GEMV_DEC4 2*[ LN_GENERIC ] TO_NCHW 2*[ GEMV_DEC2 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "swz_pad_532": "TOKENS BOX1 2*[ GEMM_T32 ] GEMM_T32_SWZ_PAD ATTN32 GEMM_T32_SWZ_PAD LN128 2*[ GEMM_T32_SWZ_PAD ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "mask9_gth0": "TOKENS BOX1 2*[ GEMM_T32 ] GEMM_T32_SWZ ATTN32 GEMM_T32_SWZ LN128 2*[ GEMM_T32_SWZ ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "mask9_gth1": "TOKENS BOX1 2*[ GEMM_T32 ] GEMM_T32_SWZ ATTN32 GEMM_T32_SWZ LN128 2*[ GEMM_T32_SWZ ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "mask9_gth2": "TOKENS BOX1 2*[ GEMM_T32 ] GEMM_T32_SWZ ATTN32 GEMM_T32_SWZ LN128 2*[ GEMM_T32_SWZ ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "mask16_gth0": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 GEMM_T32_SWZ GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 2*[ GEMV_DEC1 ] LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "mask16_gth1": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 GEMM_T32_SWZ GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 2*[ GEMV_DEC1 ] LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "mask16_gth2": "TOKENS BOX1 2*[ GEMM_T32_SWZ ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ LN256 GEMM_T32_SWZ GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 2*[ GEMV_DEC1 ] LN256_DOUBLE TO_NCHW 2*[ GEMV_DEC1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "lds_limit": "TOKENS BOX1 2*[ GEMM_T32_SWZ_PAD ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ_PAD LN256 GEMM_T32_SWZ_PAD GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 DEC0_CONST DEC_SCORES DEC_CTX GEMV_DEC8 2*[ GEMV_DEC1 ] LN256_DOUBLE TO_NCHW",
    "long_scores": "TOKENS BOX1 3*[ GEMM_T32_SWZ_PAD ] ATTN64 GEMM_T32_SWZ_PAD LN128 2*[ GEMM_T32_SWZ_PAD ] LN128 DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW",
    "enc0_dec1": "TOKENS BOX1 2*[ GEMM_T32 ] DEC0_CONST DEC_SCORES DEC_CTX 3*[ GEMV_V1 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "enc1_dec0": "TOKENS BOX1 3*[ GEMM_T32 ] ATTN32 GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "enc0_dec0": "TOKENS BOX1 2*[ GEMM_T32 ] LN128 TO_NCHW 2*[ GEMV_V1 ] REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d64_6x6_n1": "GEMV_V1 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d64_6x6_n3": "GEMV_V1 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d128_5x5_n1": "GEMV_V1 REG_ATTEND 4*[ GEMM_CONV GN_REDUCE GN_APPLY ] GEMM_CONV REG_FINISH",
    "reg_d128_5x5_n3": "GEMV_V1 REG_ATTEND 4*[ GEMM_CONV GN_REDUCE GN_APPLY ] GEMM_CONV REG_FINISH",
    "reg_d256_5x7_n1": "GEMV_DEC1 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d256_5x7_n3": "GEMV_DEC1 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d384_6x6_n1": "GEMV_V1 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d384_6x6_n3": "GEMV_V1 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d512_6x6_n1": "GEMV_DEC2 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d512_6x6_n3": "GEMV_DEC2 REG_ATTEND GEMM_CONV 4*[ GN_REDUCE GEMM_CONV_GN ] REG_FINISH",
    "reg_d512_23x23_n1": "GEMV_DEC2 REG_ATTEND 4*[ GEMM_CONV GN_REDUCE GN_APPLY ] GEMM_CONV REG_FINISH",
    "reg_d512_23x23_n3": "GEMV_DEC2 REG_ATTEND 4*[ GEMM_CONV GN_REDUCE GN_APPLY ] GEMM_CONV REG_FINISH",
    "lin_b2_n258_k256_nb": "GEMV_DEC1",
    "lin_b2_n258_k256_nb_relu": "GEMV_DEC1",
    "lin_b2_n258_k256_b": "GEMV_DEC1",
    "lin_b2_n258_k256_b_relu": "GEMV_DEC1",
    "lin_b3_n514_k512_nb": "GEMV_V4",
    "lin_b3_n514_k512_nb_relu": "GEMV_V4",
    "lin_b3_n514_k512_b": "GEMV_V4",
    "lin_b3_n514_k512_b_relu": "GEMV_V4",
    "lin_b8_n130_k192_nb": "GEMV_V1",
    "lin_b8_n130_k192_nb_relu": "GEMV_V1",
    "lin_b8_n130_k192_b": "GEMV_V1",
    "lin_b8_n130_k192_b_relu": "GEMV_V1",
    "lin_b1_n4_k64_nb": "GEMV_V1",
    "lin_b1_n4_k64_nb_relu": "GEMV_V1",
    "lin_b1_n4_k64_b": "GEMV_V1",
    "lin_b1_n4_k64_b_relu": "GEMV_V1",
    "lin_b8_n2048_k768_nb": "GEMV_V4",
    "lin_b8_n2048_k768_nb_relu": "GEMV_V4",
    "lin_b8_n2048_k768_b": "GEMV_V4",
    "lin_b8_n2048_k768_b_relu": "GEMV_V4",
}

ROUTES = {name: expand(text) for name, text in ROUTES_TEXT.items()}

# max |fp32 oracle - float64 oracle| over the outputs of each case (tests/tomp_f64.py), as measured on the CPU the table was written on
REF_ERR = {
    "deployed_par": {"predictor": 2.205e-06, "scores": 2.716e-05, "ltrb": 4.260e-06},
    "deployed_filter": {"predictor": 1.590e-06},
    "d128_h16_ff256": {"predictor": 9.650e-07, "scores": 5.072e-06, "ltrb": 6.402e-07},
    "d128_h32_ff320": {"predictor": 8.536e-07, "scores": 8.138e-06, "ltrb": 9.704e-07},
    "d128_h64_ff768": {"predictor": 9.551e-07, "scores": 1.044e-05, "ltrb": 5.262e-07},
    "d256_h16_ff320": {"predictor": 9.077e-07, "scores": 1.026e-05, "ltrb": 7.395e-07},
    "d256_h32_ff768": {"predictor": 1.417e-06, "scores": 1.814e-05, "ltrb": 8.947e-07},
    "d256_h64_ff256": {"predictor": 8.208e-07, "scores": 8.405e-06, "ltrb": 5.795e-07},
    "d384_h32_ff256": {"predictor": 1.163e-06, "scores": 2.032e-05, "ltrb": 2.006e-06},
    "d384_h64_ff768": {"predictor": 1.535e-06, "scores": 1.475e-05, "ltrb": 5.368e-07},
    "d512_h32_ff320": {"predictor": 1.128e-06, "scores": 2.106e-05, "ltrb": 1.348e-06},
    "d512_h64_ff768": {"predictor": 1.458e-06, "scores": 1.786e-05, "ltrb": 5.728e-07},
    "seq3_d256": {"predictor": 9.222e-07},
    "seq5_d256": {"predictor": 1.741e-06},
    "seq8_d256": {"predictor": 2.479e-06},
    "seq3_d128": {"predictor": 7.278e-07},
    "seq5_d128": {"predictor": 8.883e-07},
    "seq8_d128": {"predictor": 9.396e-07},
    "m1024_ff256": {"predictor": 9.859e-07, "scores": 2.308e-05, "ltrb": 9.565e-07},
    "m1024_ff768": {"predictor": 1.347e-06, "scores": 1.620e-05, "ltrb": 1.056e-06},
    "m1024_ff1024": {"predictor": 1.282e-06, "scores": 2.036e-05, "ltrb": 7.313e-07},
    "m1024_ff320": {"predictor": 1.171e-06, "scores": 1.006e-05, "ltrb": 1.702e-06},
    "m1296_ff1280": {"predictor": 1.338e-06, "scores": 1.458e-05, "ltrb": 2.257e-06},
    "m1024_d128": {"predictor": 8.358e-07, "scores": 6.517e-06, "ltrb": 7.003e-07},
    "m1024_d384": {"predictor": 1.459e-06, "scores": 2.390e-05, "ltrb": 9.237e-07},
    "m1024_d512": {"predictor": 1.412e-06, "scores": 3.268e-05, "ltrb": 7.694e-07},
    "swz_pad_532": {"predictor": 9.410e-07, "scores": 4.975e-06, "ltrb": 4.027e-07},
    "mask9_gth0": {"predictor": 8.119e-07, "scores": 8.077e-06, "ltrb": 7.461e-07},
    "mask9_gth1": {"predictor": 8.422e-07, "scores": 7.419e-06, "ltrb": 6.731e-07},
    "mask9_gth2": {"predictor": 6.335e-07, "scores": 6.111e-06, "ltrb": 4.300e-07},
    "mask16_gth0": {"predictor": 1.120e-06, "scores": 8.863e-06, "ltrb": 1.043e-06},
    "mask16_gth1": {"predictor": 9.629e-07, "scores": 1.160e-05, "ltrb": 1.044e-06},
    "mask16_gth2": {"predictor": 9.964e-07, "scores": 9.845e-06, "ltrb": 7.617e-07},
    "lds_limit": {"predictor": 1.216e-06},
    "long_scores": {"predictor": 8.749e-07},
    "enc0_dec1": {"predictor": 7.293e-07, "scores": 4.331e-06, "ltrb": 2.789e-07},
    "enc1_dec0": {"predictor": 7.615e-07, "scores": 5.995e-07, "ltrb": 6.493e-07},
    "enc0_dec0": {"predictor": 1.192e-07, "scores": 5.320e-07, "ltrb": 7.525e-07},
    "reg_d64_6x6_n1": {"ltrb": 4.475e-07},
    "reg_d64_6x6_n3": {"ltrb": 4.586e-07},
    "reg_d128_5x5_n1": {"ltrb": 3.222e-07},
    "reg_d128_5x5_n3": {"ltrb": 3.870e-07},
    "reg_d256_5x7_n1": {"ltrb": 5.018e-07},
    "reg_d256_5x7_n3": {"ltrb": 5.351e-07},
    "reg_d384_6x6_n1": {"ltrb": 8.145e-07},
    "reg_d384_6x6_n3": {"ltrb": 1.286e-06},
    "reg_d512_6x6_n1": {"ltrb": 7.734e-07},
    "reg_d512_6x6_n3": {"ltrb": 6.663e-07},
    "reg_d512_23x23_n1": {"ltrb": 1.097e-06},
    "reg_d512_23x23_n3": {"ltrb": 1.101e-06},
    "lin_b2_n258_k256_nb": {"y": 3.428e-07},
    "lin_b2_n258_k256_nb_relu": {"y": 2.795e-07},
    "lin_b2_n258_k256_b": {"y": 2.819e-07},
    "lin_b2_n258_k256_b_relu": {"y": 3.750e-07},
    "lin_b3_n514_k512_nb": {"y": 1.419e-06},
    "lin_b3_n514_k512_nb_relu": {"y": 1.569e-06},
    "lin_b3_n514_k512_b": {"y": 1.269e-06},
    "lin_b3_n514_k512_b_relu": {"y": 1.356e-06},
    "lin_b8_n130_k192_nb": {"y": 3.034e-07},
    "lin_b8_n130_k192_nb_relu": {"y": 3.891e-07},
    "lin_b8_n130_k192_b": {"y": 4.287e-07},
    "lin_b8_n130_k192_b_relu": {"y": 4.088e-07},
    "lin_b1_n4_k64_nb": {"y": 7.536e-08},
    "lin_b1_n4_k64_nb_relu": {"y": 3.215e-08},
    "lin_b1_n4_k64_b": {"y": 8.209e-08},
    "lin_b1_n4_k64_b_relu": {"y": 4.388e-08},
    "lin_b8_n2048_k768_nb": {"y": 2.278e-06},
    "lin_b8_n2048_k768_nb_relu": {"y": 2.509e-06},
    "lin_b8_n2048_k768_b": {"y": 3.248e-06},
    "lin_b8_n2048_k768_b_relu": {"y": 1.733e-06},
}


def cfg_of(name):
    return PREDICT[name]


def dims(cfg):
    return _lib.TompDims(cfg["D"], cfg["nhead"], cfg["ff"], cfg["n_enc"], cfg["n_dec"], cfg["H"], cfg["W"], cfg["feature_sz"])


def _query(fn, *args):
    out = (ctypes.c_int * _lib.PT_TOMP_MAX_ROUTES)(*([-1] * _lib.PT_TOMP_MAX_ROUTES))
    n = ctypes.c_int(-1)
    rc = fn(*args, out, _lib.PT_TOMP_MAX_ROUTES, ctypes.byref(n))
    if rc != 0:
        assert n.value == 0 and not any(out), (rc, n.value)
        return rc, ()
    assert 0 < n.value <= _lib.PT_TOMP_MAX_ROUTES and not any(out[n.value:]) and all(0 < v < len(R) for v in out[:n.value])
    return rc, tuple(R[v] for v in out[:n.value])


def predict_routes(L, cfg, n_train=None, n_seq=None, parallel=None):
    """(status, route names) of pt_tomp_predict_routes for a case's configuration (or the overrides)."""
    d = dims(cfg)
    return _query(L.pt_tomp_predict_routes, ctypes.byref(d), cfg["n_train"] if n_train is None else n_train,
                  cfg["n_seq"] if n_seq is None else n_seq, int(cfg["mode"] == "parallel") if parallel is None else parallel)


def bbreg_routes(L, n, D, H, W):
    return _query(L.pt_tomp_bbreg_routes, n, D, H, W)


def linear_routes(L, B, N, K):
    return _query(L.pt_tomp_linear_routes, B, N, K)


def case_routes(L, name):
    """(status, route names) the query reports for a case of PREDICT; for a 'parallel' case the classifier's projection (pt_tomp_linear_f32,
    B = 1, N = K = D) and the box regressor on the (1, D, H, W) encoded features follow, as the test runs them."""
    cfg = PREDICT[name]
    rc, r = predict_routes(L, cfg)
    if rc == 0 and cfg["mode"] == "parallel":
        rc1, r1 = linear_routes(L, 1, cfg["D"], cfg["D"])
        rc2, r2 = bbreg_routes(L, 1, cfg["D"], cfg["H"], cfg["W"])
        assert rc1 == 0 and rc2 == 0, (rc1, rc2)
        r = r + r1 + r2
    return rc, r


# ------------------------------------------------------------------------------------------------------------------
# parameters, inputs, modules
# ------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def predict_case(name):
    """(cfg, parameters {reference key: fp32 numpy}, (train, test, label, ltrb) fp32 numpy with n_seq sequences on axis 1), generated once
    per session."""
    if ("predict", name) not in _CACHE:
        cfg = PREDICT[name]
        k = list(PREDICT).index(name)
        params = synth.tomp_params(PARAM_SEED + 10 * k, cfg)
        seqs = [synth.tomp_inputs(INPUT_SEED + 10 * k + s, cfg) for s in range(cfg["n_seq"])]
        inputs = tuple(np.concatenate([s[i] for s in seqs], axis=1) for i in range(4))
        _CACHE[("predict", name)] = (cfg, params, inputs)
    return _CACHE[("predict", name)]


def bbreg_case(name):
    """(n, D, H, W, 'reg.' parameters, feat (n, 1, D, H, W), filter (D,)): features scaled as synth.tomp_inputs scales them, the filter at
    the size of a predicted one."""
    if ("bbreg", name) not in _CACHE:
        n, D, H, W = BBREG[name]
        k = list(BBREG).index(name)
        cfg = dict(D=D, nhead=1, ff=64, n_enc=0, n_dec=0)
        params = {q: v for q, v in synth.tomp_params(PARAM_SEED + 1000 + 10 * k, cfg).items() if q.startswith("reg.")}
        rng = np.random.default_rng(INPUT_SEED + 1000 + 10 * k)
        feat = rng.standard_normal((n, 1, D, H, W), dtype=np.float32) * np.float32(4.0 / np.sqrt(D))
        filt = rng.standard_normal(D, dtype=np.float32)
        _CACHE[("bbreg", name)] = (n, D, H, W, params, feat, filt)
    return _CACHE[("bbreg", name)]


def linear_case(name):
    """(B, N, K, bias flag, relu flag, weight (N, K), bias (N) or None, x (B, K))"""
    if ("linear", name) not in _CACHE:
        B, N, K, bias, relu = LINEAR[name]
        rng = np.random.default_rng(INPUT_SEED + 2000 + list(LINEAR).index(name))
        w = (rng.standard_normal((N, K), dtype=np.float32) / np.float32(np.sqrt(K))).astype(np.float32)
        b = rng.standard_normal(N, dtype=np.float32) if bias else None
        x = rng.standard_normal((B, K), dtype=np.float32)
        _CACHE[("linear", name)] = (B, N, K, bias, relu, w, b, x)
    return _CACHE[("linear", name)]


def build_tomp_modules(cfg, params, device):
    """The mirrored FilterPredictor / LinearFilterClassifier / DenseBoxRegressor carrying the seeded parameters,
    loaded through `load_state_dict(strict=True)` with the reference's key names."""
    from pytracking_amd import transformer as TM
    D = cfg["D"]
    tr = TM.Transformer(d_model=D, nhead=cfg["nhead"], num_encoder_layers=cfg["n_enc"],
                        num_decoder_layers=cfg["n_dec"], dim_feedforward=cfg["ff"])
    pred = TM.FilterPredictor(tr, feature_sz=cfg["feature_sz"], use_test_frame_encoding=True)
    cls = TM.LinearFilterClassifier(num_channels=D)
    reg = TM.DenseBoxRegressor(num_channels=D)
    for mod, pre in ((pred, "fp."), (cls, "cls."), (reg, "reg.")):
        sd = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith(pre)}
        if pre == "fp.":
            sd["query_embed_fg_decoder.weight"] = sd["query_embed_fg.weight"]
            for idx in (1, 4):
                sd[f"box_encoding.{idx}.num_batches_tracked"] = torch.tensor(0)
        mod.load_state_dict(sd, strict=True)
        mod.to(device).eval()
    return pred, cls, reg


def build_regressor(D, params, device):
    from pytracking_amd import transformer as TM
    reg = TM.DenseBoxRegressor(num_channels=D)
    reg.load_state_dict({k[4:]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith("reg.")}, strict=True)
    return reg.to(device).eval()
