// IoU feature extraction: AtomIoUNet.get_iou_feat (ltr/models/bbreg/atom_iou_net.py:172-179) in one call.
//
//   c3_t = conv3_2t(conv3_1t(layer2)),  c4_t = conv4_2t(conv4_1t(layer3)),  every block = Conv2d(3x3, pad 1, bias) -> BatchNorm2d (eval)
//   -> ReLU (atom_iou_net.py:7-12).  DiMP, PrDiMP, DiMPSimple, KeepTrack, KYS and ATOM run it once per frame in front of the box
//   refinement (iou_refine.hip).
//
// Per layer and tower the 3x3 convolution is the banded MFMA correlation of mf_kernels.hip (pt_launch_mf_corr_tm: 16 output channels
// per workgroup, tap-major weights, the input channels split `ks` ways into partial maps part[s][n][Cout][H][W]); k_iou_epilogue sums
// the splits in fixed order, applies y = relu(sum * scale[c] + shift[c]) (bias and eval BatchNorm as ONE per-channel affine behind the
// split sum: the weights stay the module's own values) and writes (n, C, H, W), which the second layer's correlation reads as it is --
// no token layout between the layers.  The epilogue serves BOTH towers in one launch (grid.y = tower).  The correlation kernel takes its
// band geometry as one by-value plan per launch, so the two towers (unrelated H, W, C) are two correlation launches per layer:
//   banded route: corr(3) corr(4) epilogue(3+4) | corr(3) corr(4) epilogue(3+4)  = 6 launches per call.
// A layer the banded kernel does not cover (rows wider than 170, pt_mf_corr_tm_splits() == 0) takes the per-tap split-K GEMM route of
// the classification head (tomp.hip: pt_clf_head_impl): NCHW -> tokens (channels zero-padded to a multiple of 64, k_iou_tokens; the
// weights padded alike by k_iou_padw when Cin % 64 != 0), 9 per-tap partial GEMMs written straight as NCHW partial maps (GemmArgs.nchw),
// then the SAME epilogue with 9 partials.
#include <algorithm>
#include "common.h"
#include "pt_internal.h"
#include "mfma_gemm.h"
#include "conv_tokens.h"     // k_iou_tokens, k_iou_padw

namespace {

constexpr int IOU_MAX_N = 8, IOU_MAX_HW = 4096, IOU_MAX_C = 4096;
enum { ROUTE_BANDED = 1, ROUTE_GEMM = 2 };

struct IouLayer { int route, parts, Cin, Cout, Cpad; size_t w_off, s_off, b_off; };      // offsets into the pack, floats
struct IouTower { int n, H, W, HW; IouLayer l[2]; size_t part, mid, tok, wpad; };         // offsets into the workspace, floats
struct IouPlan { IouTower t[2]; size_t ws_floats, pack_floats; };

// one tower's partial maps of one layer: y[e] = relu((sum_s part[s * count + e]) * scale[c] + shift[c]),  c = (e / HW) % C
struct IouEpi { const float* part; float* out; const float* scale; const float* shift; long count; int parts, C, HW, vec; };
struct IouEpi2 { IouEpi t[2]; };

// grid (ceil(max count / 1024), 2 towers), 256 threads, 4 consecutive elements per thread.  vec (HW % 4 == 0: the four share a channel
// and every partial map is 16-byte aligned): 16-byte loads and one 16-byte store; else the scalar path with its own bounds.
__global__ __launch_bounds__(256) void k_iou_epilogue(IouEpi2 a) {
    const IouEpi t = a.t[blockIdx.y];
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= t.count) return;
    if (t.vec) {
        f32x4 s = *(const f32x4*)(t.part + e);
        for (int k = 1; k < t.parts; ++k) s += *(const f32x4*)(t.part + (long)k * t.count + e);     // fixed order
        const int c = (int)((e / t.HW) % t.C);
        const float sc = t.scale[c], sh = t.shift[c];
        f32x4 y;
#pragma unroll
        for (int u = 0; u < 4; ++u) y[u] = fmaxf(fmaf(s[u], sc, sh), 0.f);
        *(f32x4*)(t.out + e) = y;
    } else {
        for (int u = 0; u < 4; ++u) {
            const long i = e + u;
            if (i >= t.count) break;
            float s = t.part[i];
            for (int k = 1; k < t.parts; ++k) s += t.part[(long)k * t.count + i];                   // fixed order
            const int c = (int)((i / t.HW) % t.C);
            t.out[i] = fmaxf(fmaf(s, t.scale[c], t.shift[c]), 0.f);
        }
    }
}

int iou_plan(int n, const int ch[2][3], const int hw[2][2], IouPlan* out) {
    for (int t = 0; t < 2; ++t)
        if (n <= 0 || ch[t][0] <= 0 || ch[t][1] <= 0 || ch[t][2] <= 0 || hw[t][0] <= 0 || hw[t][1] <= 0) return PT_ERR_SHAPE;
    IouPlan p{};
    size_t pk = 0, ws = 0;
    auto take = [&](size_t k) { size_t r = ws; ws += pt_align_floats(k); return r; };
    for (int t = 0; t < 2; ++t) {
        IouTower& T = p.t[t];
        T.n = n; T.H = hw[t][0]; T.W = hw[t][1];
        if (n > IOU_MAX_N || (long)T.H * T.W > IOU_MAX_HW) return PT_ERR_UNSUPPORTED;
        T.HW = T.H * T.W;
        if (ch[t][0] % 64 || ch[t][1] % 16 || ch[t][2] % 16) return PT_ERR_UNSUPPORTED;
        if (ch[t][0] > IOU_MAX_C || ch[t][1] > IOU_MAX_C || ch[t][2] > IOU_MAX_C) return PT_ERR_UNSUPPORTED;
        size_t part = 0, tok = 0, wpad = 0;
        for (int l = 0; l < 2; ++l) {
            IouLayer& L = T.l[l];
            L.Cin = ch[t][l]; L.Cout = ch[t][l + 1]; L.Cpad = (L.Cin + 63) / 64 * 64;
            L.w_off = pk; pk += (size_t)L.Cout * 9 * L.Cin;
            L.s_off = pk; pk += L.Cout;
            L.b_off = pk; pk += L.Cout;
            const int ks = pt_mf_corr_tm_splits(n, L.Cout, L.Cin, T.H, T.W);
            const size_t map = (size_t)n * L.Cout * T.HW;
            if (ks >= 1 && ks <= 8) {
                L.route = ROUTE_BANDED; L.parts = ks;
            } else {
                L.route = ROUTE_GEMM; L.parts = 9;
                // what launch_gemm's 32-bit byte offsets must hold: the 9 NCHW partial maps, the token matrix, the weight matrix
                if (9 * map * 4 >= 0xFFFFFFE0ull || (size_t)n * T.HW * L.Cpad * 4 > 0xFFFFFFE0ull ||
                    (size_t)L.Cout * 9 * L.Cpad * 4 > 0xFFFFFFE0ull)
                    return PT_ERR_UNSUPPORTED;
                tok = std::max(tok, (size_t)n * T.HW * L.Cpad);
                if (L.Cpad != L.Cin) wpad = std::max(wpad, (size_t)L.Cout * 9 * L.Cpad);
            }
            part = std::max(part, (size_t)L.parts * map);
        }
        T.part = take(part);
        T.mid = take((size_t)n * ch[t][1] * T.HW);
        T.tok = take(tok);
        T.wpad = take(wpad);
    }
    p.ws_floats = ws; p.pack_floats = pk;
    if (out) *out = p;
    return PT_OK;
}

int iou_conv(const IouTower& T, const IouLayer& L, const float* in, const float* pack, float* base, hipStream_t st) {
    float* part = base + T.part;
    if (L.route == ROUTE_BANDED)
        return pt_launch_mf_corr_tm(in, (long)L.Cin * T.HW, pack + L.w_off, part, T.n, L.Cout, L.Cin, T.H, T.W, L.parts, st);
    const int M = T.n * T.HW;
    float* X = base + T.tok;
    hipLaunchKernelGGL(k_iou_tokens, dim3((T.HW + 31) / 32, L.Cpad / 32, T.n), dim3(256), 0, st, in, X, L.Cin, L.Cpad, T.HW);
    PT_CHECK_LAUNCH();
    const float* w = pack + L.w_off;
    if (L.Cpad != L.Cin) {
        const long total = (long)L.Cout * 9 * L.Cpad;
        hipLaunchKernelGGL(k_iou_padw, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, base + T.wpad, L.Cin, L.Cpad, total);
        PT_CHECK_LAUNCH();
        w = base + T.wpad;
    }
    GemmArgs g = gemm_args(X, L.Cpad, M, w, M, L.Cout, 9 * L.Cpad, nullptr, part, L.Cout);
    g.H = T.H; g.Wd = T.W; g.Cin = L.Cpad; g.HW = T.HW; g.ksteps = L.Cpad / 64; g.c_zstride = (long)M * L.Cout; g.nchw = 1;
    return launch_gemm(g, st, true);
}

}  // namespace

extern "C" size_t pt_iou_feat_pack_floats(int Cin3, int Cmid3, int Cout3, int Cin4, int Cmid4, int Cout4) {
    const int ch[2][3] = {{Cin3, Cmid3, Cout3}, {Cin4, Cmid4, Cout4}}, hw[2][2] = {{1, 1}, {1, 1}};
    IouPlan p;
    return iou_plan(1, ch, hw, &p) == PT_OK ? p.pack_floats : 0;
}

extern "C" size_t pt_iou_feat_ws_bytes(int n, int Cin3, int Cmid3, int Cout3, int H3, int W3, int Cin4, int Cmid4, int Cout4, int H4,
                                       int W4) {
    const int ch[2][3] = {{Cin3, Cmid3, Cout3}, {Cin4, Cmid4, Cout4}}, hw[2][2] = {{H3, W3}, {H4, W4}};
    IouPlan p;
    return iou_plan(n, ch, hw, &p) == PT_OK ? p.ws_floats * sizeof(float) : 0;
}

extern "C" int pt_iou_feat_f32(const float* feat3, const float* feat4, const float* pack, float* c3_out, float* c4_out, int n, int Cin3,
                               int Cmid3, int Cout3, int H3, int W3, int Cin4, int Cmid4, int Cout4, int H4, int W4, void* ws,
                               size_t ws_bytes, void* stream) {
    if (!feat3 || !feat4 || !pack || !c3_out || !c4_out || !ws) return PT_ERR_NULL;
    const int ch[2][3] = {{Cin3, Cmid3, Cout3}, {Cin4, Cmid4, Cout4}}, hw[2][2] = {{H3, W3}, {H4, W4}};
    IouPlan p;
    int rc = iou_plan(n, ch, hw, &p);
    if (rc) return rc;
    // 16-byte loads and stores on every operand (the staging width of the banded kernel is chosen from the pointers)
    for (const void* q : {(const void*)feat3, (const void*)feat4, (const void*)pack, (const void*)c3_out, (const void*)c4_out})
        if ((uintptr_t)q % 16) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < p.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    const float* in[2] = {feat3, feat4};
    float* outp[2] = {c3_out, c4_out};
    for (int l = 0; l < 2; ++l) {
        IouEpi2 e{};
        long most = 0;
        for (int t = 0; t < 2; ++t) {
            const IouTower& T = p.t[t];
            const IouLayer& L = T.l[l];
            if ((rc = iou_conv(T, L, l == 0 ? in[t] : base + T.mid, pack, base, st))) return rc;
            IouEpi& E = e.t[t];
            E.part = base + T.part; E.out = l == 0 ? base + T.mid : outp[t];
            E.scale = pack + L.s_off; E.shift = pack + L.b_off;
            E.count = (long)T.n * L.Cout * T.HW; E.parts = L.parts; E.C = L.Cout; E.HW = T.HW; E.vec = (T.HW % 4) == 0;
            most = std::max(most, E.count);
        }
        hipLaunchKernelGGL(k_iou_epilogue, dim3((unsigned)((most + 1023) / 1024), 2), dim3(256), 0, st, e);
        PT_CHECK_LAUNCH();
    }
    return PT_OK;
}
