// RTS instance-score encoder and learners fusion: the stock-PyTorch stretch of RTS.track() between the classifier and the decoder.
//
//   ResidualDS16SW_Clf.forward (ltr/models/rts/label_encoder.py:57-103), six launches:
//   s (n,1,H,W) -> conv3x3 s1 p1 (1->C0) [+BN] + ReLU -> maxpool3x3 s1 p1                                          k_se_stem
//               -> BasicBlock(C0->C1, s1): relu(bn2(conv2(relu(bn1(conv1 x)))) + downsample(x))                     k_se_conv x 2
//               -> BasicBlock(C1->C2, s1)                                                                           k_se_conv x 2
//               -> label_pred = relu([bn](conv3x3(C2->F)))  ;  samp_w_pred = conv3x3(C2->F)                         k_se_conv x 1
//   RTSNet.segment_target's interpolate + LearnersFusion (rts_net.py:227-230, learners_fusion.py:24-38), one launch:
//   'add'    seg + bilinear(clf)                                                                                    k_fuse_add
//   'concat' Conv2d(2F->F, 3, padding 1, bias)(cat(seg, bilinear(clf)))                                             k_se_conv<., true>
//
// Every stride is 1 and the deployed map is 16 x 27 (rts50.py): the whole problem is a few hundred pixels, so the tiles are small.
//
// k_se_stem (VALU): one workgroup of 64 threads = a 4 x 16 tile of pooled outputs of one map x 4 channels.  The 8 x 20 score tile with a
//   halo of 2 is staged in LDS (zero filled outside the map = the convolution's padding); a thread holds its 5 x 5 patch in registers,
//   computes per channel the nine convolution outputs of its pooling window, applies scale / shift / ReLU and takes the maximum over the
//   window positions that exist (pooling padding = positions IGNORED, as nn.MaxPool2d's -inf; the centre always exists).  The
//   convolution output never goes to memory.
//
// k_se_conv<WV, FUSE> (exact fp32 MFMA 16x16x4, implicit GEMM): pixels of a map are numbered linearly (p = y * W + x); one workgroup of WV
//   waves = 16 consecutive pixels x 16 WV output channels, wave w owns channel tile w.  Per chunk of up to 64 input channels the im2col
//   patch [channel][tap][pixel] of the 16 pixels is staged in LDS (zero outside the map); per tap and 16 channels a lane loads ONE 16-byte
//   piece of the tap-major weights (w[co][tap][ci0 + 4*(l>>4) .. + 3]) and reads 4 patch values: k-step s pairs lane group l>>4 with
//   input channel ci0 + 4*(l>>4) + s on both operands, as k_le_conv does.  A channel's 144 patch floats are padded to 148 (4 mod 8): the
//   two 16-lane groups of a ds_read_b32 half (4 channels apart) then sit 16 banks apart.  FUSE: input channels >= Cin1 do not exist in
//   memory; the staging samples them bilinearly (align_corners=False, no antialiasing) from the second input as it fills LDS.
//   Epilogue: y = acc * scale[co] + shift[co] (+ residual[co]) (ReLU for co < relu_n), written to out0 (co < csplit) or out1.
//   Sums run in one fixed order whatever WV is; no atomics, no split accumulation: repeated calls are bit-identical.
//
// k_fuse_add<V> (VALU): V = 4 consecutive pixels of a row per thread with 16-byte accesses when Wt % 4 == 0 and the pointers allow.
#include <algorithm>
#include <math.h>
#include "common.h"
#include "pt_internal.h"
#include "ds16_enc.h"

namespace {

constexpr int SE_MAX_C = 64, SE_MAX_DIM = 1024, SE_MAX_N = 1024;
constexpr Ds16Limits SE_LIMITS{SE_MAX_C, SE_MAX_DIM, SE_MAX_N};
constexpr int SS_TH = 4, SS_TW = 16, SS_THREADS = SS_TH * SS_TW, SS_CG = 4;
constexpr int SS_LR = SS_TH + 4, SS_LC = SS_TW + 4;                      // LDS tile: origin row y0 - 2, origin column x0 - 2
constexpr int SE_CHUNK = 64, SE_CS = 148;                                // channels staged at once; floats per channel (144, padded)

// grid (ceil(W/16), ceil(H/4) * (C0/4), n), 64 threads
__global__ __launch_bounds__(SS_THREADS) void k_se_stem(const float* __restrict__ scores, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ out, int C0, int H, int W) {
    __shared__ float tile[SS_LR * SS_LC];
    const int groups = C0 / SS_CG;
    const int img = blockIdx.z, cg = blockIdx.y % groups, y0 = (blockIdx.y / groups) * SS_TH, x0 = blockIdx.x * SS_TW;
    const float* src = scores + (long)img * H * W;
    for (int e = threadIdx.x; e < SS_LR * SS_LC; e += SS_THREADS) {
        const int r = e / SS_LC, c = e - r * SS_LC, iy = y0 - 2 + r, ix = x0 - 2 + c;
        tile[e] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? src[(long)iy * W + ix] : 0.f;
    }
    __syncthreads();
    const int lx = threadIdx.x % SS_TW, ly = threadIdx.x / SS_TW, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) return;                                        // behind the only barrier
    float p[5][5];                                                       // p[r][c] = score(y - 2 + r, x - 2 + c)
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int c = 0; c < 5; ++c) p[r][c] = tile[(ly + r) * SS_LC + lx + c];
    bool ok[3][3];                                                       // does convolution output (y - 1 + a, x - 1 + b) exist
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int cy = y - 1 + a, cx = x - 1 + b;
            ok[a][b] = cy >= 0 && cy < H && cx >= 0 && cx < W;
        }
    const long plane = (long)H * W;
    float* o = out + (long)img * C0 * plane + (long)y * W + x;
    for (int c = cg * SS_CG; c < (cg + 1) * SS_CG; ++c) {
        float wk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k] = w[c * 9 + k];
        const float sc = scale[c], sh = shift[c];
        float m = -INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                float v = 0.f;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) v = fmaf(wk[ky * 3 + kx], p[a + ky][b + kx], v);
                v = fmaxf(fmaf(v, sc, sh), 0.f);
                m = ok[a][b] ? fmaxf(m, v) : m;                          // the centre (a = b = 1) always exists
            }
        o[c * plane] = m;
    }
}

// F.interpolate(mode='bilinear', align_corners=False) with an explicit size, one output value: src = (dst + 0.5) * (in / out) - 0.5
// clamped below at 0, i0 = floor(src), i1 = min(i0 + 1, in - 1), weight src - i0.  `same`: equal sizes, the reference skips the resize.
struct SeResize { int Hs, Ws, same; float sy, sx; };

__device__ __forceinline__ void se_axis(float scale, int dst, int in, int& i0, int& i1, float& l1) {
    const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = min((int)s, in - 1);
    i1 = min(i0 + 1, in - 1);
    l1 = s - (float)i0;
}

__device__ __forceinline__ float se_bilinear(const float* __restrict__ src, const SeResize& r, int y, int x) {
    if (r.same) return src[y * r.Ws + x];
    int y0, y1, x0, x1;
    float ly, lx;
    se_axis(r.sy, y, r.Hs, y0, y1, ly);
    se_axis(r.sx, x, r.Ws, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * src[y0 * r.Ws + x0] + lx * src[y0 * r.Ws + x1]) + ly * (hx * src[y1 * r.Ws + x0] + lx * src[y1 * r.Ws + x1]);
}

struct SeConv {
    const float* in; long in_img;                // input (n, >= Cin1, H, W) view: image stride in floats, channel stride H * W
    const float* in2; long in2_img; int Cin1;    // FUSE: input channels >= Cin1 are the resize of in2 (n, Cin - Cin1, Hs, Ws) to H x W
    SeResize rs;
    const float* w; const float* scale; const float* shift;      // (Cout, 3, 3, Cin), (Cout) or null = 1, (Cout)
    const float* res; long res_img;              // optional residual (n, Cout, H, W) view
    float* out0; long out0_img; float* out1; long out1_img;      // channels < csplit -> out0[co], the others -> out1[co - csplit]
    int csplit, Cin, Cout, H, W, relu_n;
};

// grid (ceil(H*W/16), Cout / (16 WV), n), 64 WV threads
template <int WV, bool FUSE>
__global__ __launch_bounds__(64 * WV) void k_se_conv(SeConv a) {
    __shared__ float tile[SE_CHUNK * SE_CS];
    const int img = blockIdx.z, p0 = blockIdx.x * 16, HW = a.H * a.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, j = lane & 15;
    const int cot = blockIdx.y * WV + wave;                              // this wave's tile of 16 output channels
    const float* src = a.in + (long)img * a.in_img;
    const float* src2 = FUSE ? a.in2 + (long)img * a.in2_img : nullptr;
    // the staging loop strides by a multiple of 16, so a thread always fills the same pixel of the patch
    const int sp = p0 + j, sy = sp / a.W, sx = sp - sy * a.W;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wl = a.w + ((long)(cot * 16 + j) * 9) * a.Cin + 4 * kq;                 // + tap * Cin + ci
    for (int cb = 0; cb < a.Cin; cb += SE_CHUNK) {
        const int nc = min(SE_CHUNK, a.Cin - cb);
        if (cb) __syncthreads();
        for (int e = threadIdx.x; e < nc * 144; e += 64 * WV) {
            const int c = e / 144, rem = e - c * 144, tap = rem >> 4, ky = tap / 3, kx = tap - 3 * ky;
            const int iy = sy + ky - 1, ix = sx + kx - 1, ci = cb + c;
            float v = 0.f;
            if (sp < HW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                if (!FUSE || ci < a.Cin1) v = src[(long)ci * HW + iy * a.W + ix];
                else v = se_bilinear(src2 + (long)(ci - a.Cin1) * a.rs.Hs * a.rs.Ws, a.rs, iy, ix);
            }
            tile[c * SE_CS + rem] = v;
        }
        __syncthreads();
        for (int ci0 = 0; ci0 < nc; ci0 += 16) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const f32x4 wv = *(const f32x4*)(wl + (long)tap * a.Cin + cb + ci0);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = mfma16(wv[s], tile[(ci0 + 4 * kq + s) * SE_CS + tap * 16 + j], acc);
            }
        }
    }
    if (sp >= HW) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = cot * 16 + 4 * kq + r;
        float v = a.scale ? fmaf(acc[r], a.scale[co], a.shift[co]) : acc[r] + a.shift[co];   // no scale: a plain bias
        if (a.res) v += a.res[(long)img * a.res_img + (long)co * HW + sp];
        if (co < a.relu_n) v = fmaxf(v, 0.f);
        if (co < a.csplit) a.out0[(long)img * a.out0_img + (long)co * HW + sp] = v;
        else a.out1[(long)img * a.out1_img + (long)(co - a.csplit) * HW + sp] = v;
    }
}

// grid (ceil(planes * Ht * (Wt / V) / 256)), 256 threads; planes = n * F
template <int V>
__global__ __launch_bounds__(256) void k_fuse_add(const float* __restrict__ seg, const float* __restrict__ clf, float* __restrict__ out,
                                                  int planes, int Ht, int Wt, SeResize rs) {
    const int wq = Wt / V;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)planes * Ht * wq) return;
    const int x = (int)(idx % wq) * V;
    const long t = idx / wq;
    const int y = (int)(t % Ht);
    const long pl = t / Ht, at = (pl * Ht + y) * Wt + x;
    const float* src = clf + pl * rs.Hs * rs.Ws;
    if (V == 4) {
        const f32x4 s = *(const f32x4*)(seg + at);
        f32x4 o;
        if (rs.same) {
            o = s + *(const f32x4*)(src + y * rs.Ws + x);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) o[u] = s[u] + se_bilinear(src, rs, y, x + u);
        }
        *(f32x4*)(out + at) = o;
    } else {
        out[at] = seg[at] + se_bilinear(src, rs, y, x);
    }
}

// Tile choice from the shape alone: waves (= tiles of 16 output channels) per workgroup.  A workgroup stages its pixels' patch once for
// all its waves, so more waves mean less staging -- but the deployed problem is 27 pixel tiles of one map, and the chip has 256 CUs: the
// largest count that still gives about a hundred workgroups, else one wave per workgroup (the most workgroups there are).
int se_waves(int n, int H, int W, int Cout) {
    const int ct = Cout / 16;
    const long ptiles = (long)pt_ceil_div(H * W, 16) * n;
    for (int wv : {4, 2})
        if (ct % wv == 0 && ptiles * (ct / wv) >= 96) return wv;
    return 1;
}

template <bool FUSE>
int se_conv(const SeConv& a, int n, hipStream_t st) {
    const int wv = se_waves(n, a.H, a.W, a.Cout);
    const dim3 grid(pt_ceil_div(a.H * a.W, 16), a.Cout / (16 * wv), n);                  // x <= 65536, y <= 8, z <= SE_MAX_N
    switch (wv) {
        case 4: hipLaunchKernelGGL((k_se_conv<4, FUSE>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_se_conv<2, FUSE>), grid, dim3(128), 0, st, a); break;
        default: hipLaunchKernelGGL((k_se_conv<1, FUSE>), grid, dim3(64), 0, st, a); break;
    }
    PT_CHECK_LAUNCH();
    return PT_OK;
}

}  // namespace

size_t pt_score_enc_pack_floats_impl(int c0, int c1, int c2, int f) { return ds16_pack_floats(1, SE_LIMITS, c0, c1, c2, f); }

size_t pt_score_enc_ws_bytes_impl(int n, int H, int W, int c0, int c1, int c2, int f) {
    return ds16_ws_bytes(1, SE_LIMITS, n, H, W, c0, c1, c2, f);
}

int pt_score_enc_impl(const float* scores, const float* pack, float* label_enc, float* sample_w, int n, int H, int W, int c0, int c1,
                      int c2, int f, void* ws, size_t ws_bytes, hipStream_t st) {
    auto stem = [&](const Ds16Plan& p, const float* pk, float* out) -> int {
        hipLaunchKernelGGL(k_se_stem, dim3(pt_ceil_div(W, SS_TW), pt_ceil_div(H, SS_TH) * (c0 / SS_CG), n), dim3(SS_THREADS), 0, st, scores,
                           pk + p.stem.w_off, pk + p.stem.s_off, pk + p.stem.b_off, out, c0, H, W);
        PT_CHECK_LAUNCH();
        return PT_OK;
    };
    auto conv = [&](const Ds16Conv& c, int images) {
        SeConv a{};
        a.in = c.in; a.in_img = c.in_img; a.Cin1 = c.Cin;
        a.w = c.w; a.scale = c.scale; a.shift = c.shift;
        a.res = c.res; a.res_img = c.res_img;
        a.out0 = c.out0; a.out0_img = c.out0_img; a.out1 = c.out1; a.out1_img = c.out1_img;
        a.csplit = c.csplit; a.Cin = c.Cin; a.Cout = c.Cout; a.H = c.Ho; a.W = c.Wo; a.relu_n = c.relu_n;
        return se_conv<false>(a, images, st);
    };
    // sample_w may be null: that half of the heads is skipped
    return ds16_encode(1, SE_LIMITS, true, scores, pack, label_enc, sample_w, n, H, W, c0, c1, c2, f, ws, ws_bytes, stem, conv);
}

size_t pt_learners_fuse_pack_floats_impl(int f) {
    return (f > 0 && f % 16 == 0 && f <= SE_MAX_C) ? (size_t)f * 9 * 2 * f + f : 0;
}

int pt_learners_fuse_impl(const float* seg_enc, const float* clf_enc, const float* pack, float* out, int n, int f, int Hs, int Ws, int Ht,
                          int Wt, int mode, hipStream_t st) {
    if (!seg_enc || !clf_enc || !out) return PT_ERR_NULL;
    if (mode != PT_FUSE_ADD && mode != PT_FUSE_CONCAT) return PT_ERR_UNSUPPORTED;
    if (mode == PT_FUSE_CONCAT && !pack) return PT_ERR_NULL;
    if (n <= 0 || f <= 0 || Hs <= 0 || Ws <= 0 || Ht <= 0 || Wt <= 0) return PT_ERR_SHAPE;
    if (f > SE_MAX_C || (mode == PT_FUSE_CONCAT && f % 16)) return PT_ERR_UNSUPPORTED;
    if (n > SE_MAX_N || std::max({Hs, Ws, Ht, Wt}) > SE_MAX_DIM) return PT_ERR_UNSUPPORTED;
    for (const void* q : {(const void*)seg_enc, (const void*)clf_enc, (const void*)out})
        if ((uintptr_t)q % 4) return PT_ERR_UNSUPPORTED;
    SeResize rs{Hs, Ws, Hs == Ht && Ws == Wt, (float)Hs / (float)Ht, (float)Ws / (float)Wt};
    if (mode == PT_FUSE_ADD) {
        const bool wide = Wt % 4 == 0 && ((uintptr_t)seg_enc | (uintptr_t)out | (rs.same ? (uintptr_t)clf_enc : 0)) % 16 == 0;
        const long threads = (long)n * f * Ht * (wide ? Wt / 4 : Wt);                    // <= 2^36: below 2^31 blocks
        const dim3 grid((unsigned)((threads + 255) / 256));
        if (wide) hipLaunchKernelGGL(k_fuse_add<4>, grid, dim3(256), 0, st, seg_enc, clf_enc, out, n * f, Ht, Wt, rs);
        else hipLaunchKernelGGL(k_fuse_add<1>, grid, dim3(256), 0, st, seg_enc, clf_enc, out, n * f, Ht, Wt, rs);
        PT_CHECK_LAUNCH();
        return PT_OK;
    }
    if ((uintptr_t)pack % 16) return PT_ERR_UNSUPPORTED;                 // 16-byte weight loads
    const long hw = (long)Ht * Wt;
    SeConv a{};
    a.in = seg_enc; a.in_img = f * hw; a.in2 = clf_enc; a.in2_img = (long)f * Hs * Ws; a.Cin1 = f; a.rs = rs;
    a.w = pack; a.shift = pack + (size_t)f * 9 * 2 * f; a.scale = nullptr;
    a.Cin = 2 * f; a.Cout = f; a.H = Ht; a.W = Wt; a.csplit = f; a.out0 = out; a.out0_img = f * hw;
    return se_conv<true>(a, n, st);
}
