// LWL / RTS segmentation decoder: LWTLDecoder.forward (ltr/models/lwl/decoder.py:130-160) = RTSDecoder.forward
// (ltr/models/rts/decoder.py, the same code) in one asynchronous call, fp32, eval mode, num_objects = None.
//
// Levels run deepest first (decoder.py:140; layer4 -> layer1, or layer3 -> layer1), oc = {1,2,2,4} * mdim for layer1..4 (decoder.py:104):
//   s   = bilinear(scores -> ft size)            decoder.py:143, utils.py:11-14 (align_corners=False)          k_dec_resize
//   x   = relu(conv1x1(x_prev))                  decoder.py:145, proj[L] (every level but the first)           k_dec_conv1
//   TSE (decoder.py:27-32): h = conv1x1(relu(conv1x1(ft)))                                                     k_dec_conv1 x 2
//       hpool = mean(h) on the first level, else x (a map)   decoder.py:29                                     k_dec_mean
//       h = cat(h, s); 3 x relu(conv3x3(h) + bias)           decoder.py:30-31, utils.py:5-8                    conv3 + k_dec_epilogue
//       (the second 1x1 and the resize write the two channel slices of the concatenated map: no copy)
//   RRB (decoder.py:67-69): h = conv1x1(x); relu(h + conv3x3_nobias(relu(BN(conv3x3(h) + bias))))               k_dec_conv1, conv3 x 2
//       bias and eval BatchNorm are ONE per-channel scale / shift behind the split sum (folded in float64 by the caller)
//   CAB (decoder.py:42-54): g = sigmoid(conv1x1(relu(conv1x1(cat(mean(shallower), deeper_pool)))))              k_dec_mean, k_dec_cab
//       out = shallower * g + bilinear(deeper -> shallower size)  (deepest level: deeper is the pooled vector)  k_dec_gate
//   Upsampler (decoder.py:79-84): bicubic x2, relu(conv3x3 mdim -> mdim/2), bicubic -> image size, conv3x3 -> 1 channel
//       bicubic: A = -0.75, align_corners=False, source coordinate NOT clamped, tap indices clamped      k_dec_resize, conv3, k_dec_conv_out
//
// conv3 = the banded tap-major MFMA correlation (pt_launch_mf_corr_tm) wherever pt_mf_corr_tm_splits() > 0, else the per-tap split-K
// GEMM route of iou_feat.hip (tokens, 9 partial products written as NCHW partial maps); k_dec_epilogue sums the partial maps in fixed
// order, applies scale / shift, the optional residual and ReLU and writes a plain map or a channel slice of a wider one.
// k_dec_conv1 is a 1x1 convolution on the exact fp32 MFMA reading NCHW as it is: D[channel][position], 16 output channels x 16 T
// positions per workgroup, the four waves split the input channels in chunks of 16 and their accumulators are summed through LDS in wave
// order.  No atomics anywhere: two calls return the same bits.
#include <algorithm>
#include <math.h>
#include "common.h"
#include "pt_internal.h"
#include "mfma_gemm.h"
#include "conv_tokens.h"

namespace {

constexpr int DEC_MAX_N = 8, DEC_MAX_MDIM = 256, DEC_MAX_IC = 256, DEC_MAX_FC = 8192, DEC_MAX_OUT_CIN = 128;
constexpr size_t DEC_MAX_BYTES = 0xFFFFFFE0ull;          // what the launchers' 32-bit byte offsets hold
enum { ROUTE_BANDED = 1, ROUTE_GEMM = 2 };

struct DecConv3 { int route, parts, Cin, Cout, Cpad; size_t w, s, b; };                      // pack offsets, floats
struct DecRRB { size_t w1, b1; DecConv3 a, b; };
struct DecLevel {
    int fc, oc, nc, H, W, HW;
    size_t proj_w, proj_b, red0_w, red0_b, red1_w, red1_b, cab_w1, cab_b1, cab_w2, cab_b2;
    DecConv3 tr[3];
    DecRRB r1, r2;
};
struct DecPlan {
    int n, levels, ic, mdim, SH, SW, H2, W2, IH, IW;
    DecLevel L[4];
    DecConv3 up1;
    size_t up2_w, up2_b;
    size_t cat0, cat1, r, s, t, xa, xb, xp, part, tok, wpad, u0, u1, u2, vec;               // workspace offsets, floats
    size_t ws_floats, pack_floats;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// 1x1 convolution on NCHW: out[img][co][p] = act(sum_ci w[co][ci] * in[img][ci][p] + bias[co]).  grid (ceil(HW / (16 T)), Cout / 16, n),
// 256 threads.  Per 16-channel chunk a lane loads ONE 16-byte piece of the weight row (w[co0 + (l & 15)][ci0 + 4 * (l >> 4) .. + 3]) and
// 4 T input values; k-step s pairs lane group l >> 4 with input channel ci0 + 4 * (l >> 4) + s on both operands.  Wave w owns the chunks
// w, w + 4, ...; the three other accumulators go through LDS and wave 0 adds them in wave order.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void k_dec_conv1(const float* __restrict__ in, long in_sn, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out, long out_sn, int Cin, int HW,
                                                   int relu) {
    __shared__ f32x4 red[3][T][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, j = lane & 15;
    const int p0 = blockIdx.x * (16 * T), co0 = blockIdx.y * 16, img = blockIdx.z;
    const float* src = in + (long)img * in_sn;
    const float* wl = w + (long)(co0 + j) * Cin + 4 * kq;
    int pp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) pp[t] = min(p0 + 16 * t + j, HW - 1);          // columns past the map are computed and dropped
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ci0 = wave * 16; ci0 < Cin; ci0 += 64) {
        const f32x4 a = *(const f32x4*)(wl + ci0);
        const float* b = src + (long)(ci0 + 4 * kq) * HW;
        float bv[4][T];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < T; ++t) bv[s][t] = b[(long)s * HW + pp[t]];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = mfma16(a[s], bv[s][t], acc[t]);
    }
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) red[wave - 1][t][lane] = acc[t];
    }
    __syncthreads();
    if (wave > 0) return;
    float* dst = out + (long)img * out_sn;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const f32x4 v = ((acc[t] + red[0][t][lane]) + red[1][t][lane]) + red[2][t][lane];
        const int p = p0 + 16 * t + j;
        if (p < HW) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 4 * kq + r;
                float y = v[r] + bias[co];
                if (relu) y = fmaxf(y, 0.f);
                dst[(long)co * HW + p] = y;
            }
        }
    }
}

// partial maps part[s][img][C][HW] -> out[img * out_sn + c * HW + p] = act((sum_s part[s]) * scale[c] + shift[c] (+ res[img][c][p]))
struct DecEpi {
    const float* part; const float* scale; const float* shift; const float* res; float* out;
    long count, out_sn; int parts, C, HW, relu, vec;
};
// grid ceil(count / 1024), 256 threads, 4 consecutive elements per thread (vec: HW % 4 == 0, every operand 16-byte aligned)
__global__ __launch_bounds__(256) void k_dec_epilogue(DecEpi t) {
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= t.count) return;
    const long chw = (long)t.C * t.HW;
    if (t.vec) {
        f32x4 s = *(const f32x4*)(t.part + e);
        for (int k = 1; k < t.parts; ++k) s += *(const f32x4*)(t.part + (long)k * t.count + e);     // fixed order
        const long img = e / chw, rem = e - img * chw;
        const int c = (int)(rem / t.HW);
        const float sc = t.scale[c], sh = t.shift[c];
        f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t.res) r = *(const f32x4*)(t.res + e);
        f32x4 y;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            y[u] = fmaf(s[u], sc, sh) + r[u];
            if (t.relu) y[u] = fmaxf(y[u], 0.f);
        }
        *(f32x4*)(t.out + img * t.out_sn + rem) = y;
    } else {
        for (int u = 0; u < 4; ++u) {
            const long i = e + u;
            if (i >= t.count) break;
            float s = t.part[i];
            for (int k = 1; k < t.parts; ++k) s += t.part[(long)k * t.count + i];                   // fixed order
            const long img = i / chw, rem = i - img * chw;
            const int c = (int)(rem / t.HW);
            float y = fmaf(s, t.scale[c], t.shift[c]) + (t.res ? t.res[i] : 0.f);
            if (t.relu) y = fmaxf(y, 0.f);
            t.out[img * t.out_sn + rem] = y;
        }
    }
}

// out[img * C + c] = mean over HW of in[img * in_sn + c * HW + p].  grid (C, n), 256 threads; strided partial sums, then the block sum
__global__ __launch_bounds__(256) void k_dec_mean(const float* __restrict__ in, long in_sn, float* __restrict__ out, int C, int HW) {
    __shared__ float scratch[4];
    const float* src = in + (long)blockIdx.y * in_sn + (long)blockIdx.x * HW;
    float a = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) a += src[p];
    const float tot = block_sum(a, scratch, 256);
    if (threadIdx.x == 0) out[(long)blockIdx.y * C + blockIdx.x] = tot / (float)HW;
}

// CAB gate of one sample per workgroup: g = sigmoid(W2 relu(W1 [ms | dp] + b1) + b2), W1 (oc, 2 oc), W2 (oc, oc).  A wave per row.
__global__ __launch_bounds__(256) void k_dec_cab(const float* __restrict__ ms, const float* __restrict__ dp, const float* __restrict__ w1,
                                                 const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                 float* __restrict__ gate, int oc) {
    __shared__ float v[2 * 4 * DEC_MAX_MDIM], hid[4 * DEC_MAX_MDIM];
    const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < oc; k += 256) { v[k] = ms[(long)img * oc + k]; v[oc + k] = dp[(long)img * oc + k]; }
    __syncthreads();
    for (int r = wave; r < oc; r += 4) {
        const float* row = w1 + (long)r * 2 * oc;
        float a = 0.f;
        for (int k = lane; k < 2 * oc; k += 64) a = fmaf(row[k], v[k], a);
        a = wave_sum(a);
        if (lane == 0) hid[r] = fmaxf(a + b1[r], 0.f);
    }
    __syncthreads();
    for (int r = wave; r < oc; r += 4) {
        const float* row = w2 + (long)r * oc;
        float a = 0.f;
        for (int k = lane; k < oc; k += 64) a = fmaf(row[k], hid[k], a);
        a = wave_sum(a);
        if (lane == 0) gate[(long)img * oc + r] = 1.f / (1.f + expf(-(a + b2[r])));
    }
}

// PyTorch's align_corners=False source coordinate: scale * (d + 0.5) - 0.5 with scale = in / out in float
__device__ __forceinline__ float dec_src(int d, float scale) { return scale * ((float)d + 0.5f) - 0.5f; }

__device__ __forceinline__ float dec_bilinear(const float* __restrict__ pl, int Hi, int Wi, int y, int x, float sy, float sx) {
    const float fy = fmaxf(dec_src(y, sy), 0.f), fx = fmaxf(dec_src(x, sx), 0.f);
    const int y0 = min((int)fy, Hi - 1), x0 = min((int)fx, Wi - 1);
    const int y1 = y0 + (y0 < Hi - 1 ? 1 : 0), x1 = x0 + (x0 < Wi - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * pl[(long)y0 * Wi + x0] + lx * pl[(long)y0 * Wi + x1]) + ly * (hx * pl[(long)y1 * Wi + x0] + lx * pl[(long)y1 * Wi + x1]);
}

__device__ __forceinline__ void dec_cubic(float t, float (&w)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// in (n, C, Hi, Wi) dense -> out[img * out_sn + c * Ho * Wo + y * Wo + x]; bicubic = 0: bilinear.  grid (ceil(Ho*Wo / 256), C, n)
__global__ __launch_bounds__(256) void k_dec_resize(const float* __restrict__ in, float* __restrict__ out, long out_sn, int C, int Hi, int Wi,
                                                    int Ho, int Wo, float sy, float sx, int bicubic) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Ho * Wo) return;
    const int y = e / Wo, x = e - y * Wo, c = blockIdx.y, img = blockIdx.z;
    const float* pl = in + ((long)img * C + c) * Hi * Wi;
    float v;
    if (!bicubic) {
        v = dec_bilinear(pl, Hi, Wi, y, x, sy, sx);
    } else {
        const float fy = dec_src(y, sy), fx = dec_src(x, sx);
        const float yf = floorf(fy), xf = floorf(fx);
        const int iy = (int)yf, ix = (int)xf;
        float wy[4], wx[4];
        dec_cubic(fy - yf, wy);
        dec_cubic(fx - xf, wx);
        v = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float* row = pl + (long)min(max(iy - 1 + a, 0), Hi - 1) * Wi;
            float r = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) r += row[min(max(ix - 1 + b, 0), Wi - 1)] * wx[b];
            v += r * wy[a];
        }
    }
    out[(long)img * out_sn + (long)c * Ho * Wo + e] = v;
}

// out[img][c][p] = sh[img][c][p] * gate[img][c] + (deep_map ? bilinear(deep_map[img][c] (Hd, Wd) -> (H, W))[p] : deep_vec[img][c])
// grid (ceil(H*W / 256), n * C)
__global__ __launch_bounds__(256) void k_dec_gate(const float* __restrict__ sh, const float* __restrict__ gate, const float* __restrict__ deep_vec,
                                                  const float* __restrict__ deep_map, float* __restrict__ out, int H, int W, int Hd, int Wd,
                                                  float sy, float sx) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= H * W) return;
    const long pl = blockIdx.y;
    float d;
    if (deep_map) {
        const int y = e / W, x = e - y * W;
        d = dec_bilinear(deep_map + pl * Hd * Wd, Hd, Wd, y, x, sy, sx);
    } else {
        d = deep_vec[pl];
    }
    out[pl * H * W + e] = sh[pl * H * W + e] * gate[pl] + d;
}

// the last convolution, Cin -> 1 channel (nothing for the 16-filter bank): out[img][y][x] = bias + sum_{tap, ci} w[tap][ci] * in[img][ci][..]
// grid (ceil(W / 64), ceil(H / 4), n), 256 threads = 4 rows x 64 columns; the 9 * Cin weights in LDS
__global__ __launch_bounds__(256) void k_dec_conv_out(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int Cin, int H, int W) {
    __shared__ float wl[9 * DEC_MAX_OUT_CIN];
    for (int k = threadIdx.x; k < 9 * Cin; k += 256) wl[k] = w[k];
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), img = blockIdx.z;
    if (x >= W || y >= H) return;                                          // behind the only barrier
    const long plane = (long)H * W;
    const float* src = in + (long)img * Cin * plane;
    float acc = bias[0];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x + kx - 1;
            if (ix < 0 || ix >= W) continue;
            const float* q = src + (long)iy * W + ix;
            const float* wt = wl + (ky * 3 + kx) * Cin;
            for (int ci = 0; ci < Cin; ++ci) acc = fmaf(wt[ci], q[(long)ci * plane], acc);
        }
    }
    out[(long)img * plane + (long)y * W + x] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------------------------------------
struct DecSizes { size_t part, tok, wpad; bool ok; };

void dec_conv3_plan(DecConv3& c, int n, int Cin, int Cout, int H, int W, size_t& pk, DecSizes& z) {
    c.Cin = Cin; c.Cout = Cout; c.Cpad = (Cin + 63) / 64 * 64;
    c.w = pk; pk += (size_t)Cout * 9 * Cin;
    c.s = pk; pk += Cout;
    c.b = pk; pk += Cout;
    const size_t HW = (size_t)H * W, map = (size_t)n * Cout * HW;
    const int ks = pt_mf_corr_tm_splits(n, Cout, Cin, H, W);
    if (ks >= 1 && ks <= 8) {
        c.route = ROUTE_BANDED; c.parts = ks;
    } else {
        c.route = ROUTE_GEMM; c.parts = 9;
        // what launch_gemm's 32-bit byte offsets must hold: the 9 NCHW partial maps, the token matrix, the weight matrix
        if (9 * map * 4 >= DEC_MAX_BYTES || (size_t)n * HW * c.Cpad * 4 > DEC_MAX_BYTES || (size_t)Cout * 9 * c.Cpad * 4 > DEC_MAX_BYTES) z.ok = false;
        z.tok = std::max(z.tok, (size_t)n * HW * c.Cpad);
        if (c.Cpad != Cin) z.wpad = std::max(z.wpad, (size_t)Cout * 9 * c.Cpad);
    }
    if ((size_t)c.parts * map * 4 >= DEC_MAX_BYTES || (size_t)n * Cin * HW * 4 >= DEC_MAX_BYTES) z.ok = false;
    z.part = std::max(z.part, (size_t)c.parts * map);
}

void dec_rrb_plan(DecRRB& r, int n, int oc, int H, int W, size_t& pk, DecSizes& z) {
    r.w1 = pk; pk += (size_t)oc * oc;
    r.b1 = pk; pk += oc;
    dec_conv3_plan(r.a, n, oc, oc, H, W, pk, z);
    dec_conv3_plan(r.b, n, oc, oc, H, W, pk, z);
}

// fc / hw in execution order (deepest level first)
int dec_plan(int n, int levels, const int* fc, const int* hw, const int* score_hw, const int* image_hw, int ic, int mdim, DecPlan* out) {
    if (!fc || !hw || !score_hw || !image_hw) return PT_ERR_NULL;
    if (n <= 0 || ic <= 0 || mdim <= 0 || score_hw[0] <= 0 || score_hw[1] <= 0 || image_hw[0] <= 0 || image_hw[1] <= 0) return PT_ERR_SHAPE;
    if (levels != 3 && levels != 4) return PT_ERR_UNSUPPORTED;
    if (n > DEC_MAX_N || ic % 16 || mdim % 32 || ic > DEC_MAX_IC || mdim > DEC_MAX_MDIM || mdim / 2 > DEC_MAX_OUT_CIN) return PT_ERR_UNSUPPORTED;
    static const int mult4[4] = {4, 2, 2, 1}, mult3[3] = {2, 2, 1};
    DecPlan p{};
    p.n = n; p.levels = levels; p.ic = ic; p.mdim = mdim;
    p.SH = score_hw[0]; p.SW = score_hw[1]; p.IH = image_hw[0]; p.IW = image_hw[1];
    if ((size_t)n * ic * p.SH * p.SW * 4 >= DEC_MAX_BYTES) return PT_ERR_UNSUPPORTED;
    size_t pk = 0, cat = 0, omap = 0, xp = 0;
    DecSizes z{0, 0, 0, true};
    for (int l = 0; l < levels; ++l) {
        DecLevel& L = p.L[l];
        L.fc = fc[l]; L.H = hw[2 * l]; L.W = hw[2 * l + 1];
        if (L.fc <= 0 || L.H <= 0 || L.W <= 0) return PT_ERR_SHAPE;
        if (L.fc % 16 || L.fc > DEC_MAX_FC || (size_t)L.H * L.W >= (1u << 24)) return PT_ERR_UNSUPPORTED;
        L.HW = L.H * L.W;
        L.oc = (levels == 4 ? mult4[l] : mult3[l]) * mdim;
        L.nc = L.oc + ic;
        if ((size_t)n * L.fc * L.HW * 4 >= DEC_MAX_BYTES || (size_t)n * L.nc * L.HW * 4 >= DEC_MAX_BYTES) return PT_ERR_UNSUPPORTED;
        if (l > 0) {
            const DecLevel& P = p.L[l - 1];
            L.proj_w = pk; pk += (size_t)L.oc * P.oc;
            L.proj_b = pk; pk += L.oc;
            if ((size_t)n * std::max(L.oc, P.oc) * P.HW * 4 >= DEC_MAX_BYTES) return PT_ERR_UNSUPPORTED;
            xp = std::max(xp, (size_t)n * L.oc * P.HW);
        }
        L.red0_w = pk; pk += (size_t)L.oc * L.fc;
        L.red0_b = pk; pk += L.oc;
        L.red1_w = pk; pk += (size_t)L.oc * L.oc;
        L.red1_b = pk; pk += L.oc;
        dec_conv3_plan(L.tr[0], n, L.nc, L.nc, L.H, L.W, pk, z);
        dec_conv3_plan(L.tr[1], n, L.nc, L.nc, L.H, L.W, pk, z);
        dec_conv3_plan(L.tr[2], n, L.nc, L.oc, L.H, L.W, pk, z);
        dec_rrb_plan(L.r1, n, L.oc, L.H, L.W, pk, z);
        L.cab_w1 = pk; pk += (size_t)L.oc * 2 * L.oc;
        L.cab_b1 = pk; pk += L.oc;
        L.cab_w2 = pk; pk += (size_t)L.oc * L.oc;
        L.cab_b2 = pk; pk += L.oc;
        dec_rrb_plan(L.r2, n, L.oc, L.H, L.W, pk, z);
        cat = std::max(cat, (size_t)n * L.nc * L.HW);
        omap = std::max(omap, (size_t)n * L.oc * L.HW);
    }
    const DecLevel& last = p.L[levels - 1];
    if (last.H > (1 << 14) || last.W > (1 << 14) || p.IH > (1 << 15) || p.IW > (1 << 15)) return PT_ERR_UNSUPPORTED;
    p.H2 = 2 * last.H; p.W2 = 2 * last.W;
    const size_t hw2 = (size_t)p.H2 * p.W2, ihw = (size_t)p.IH * p.IW;
    if (hw2 >= (1u << 24) || ihw >= (1u << 26)) return PT_ERR_UNSUPPORTED;
    if ((size_t)n * mdim * hw2 * 4 >= DEC_MAX_BYTES || (size_t)n * (mdim / 2) * ihw * 4 >= DEC_MAX_BYTES) return PT_ERR_UNSUPPORTED;
    dec_conv3_plan(p.up1, n, mdim, mdim / 2, p.H2, p.W2, pk, z);
    p.up2_w = pk; pk += (size_t)9 * (mdim / 2);
    p.up2_b = pk; pk += 1;
    if (!z.ok) return PT_ERR_UNSUPPORTED;
    size_t ws = 0;
    auto take = [&](size_t k) { size_t r = ws; ws += pt_align_floats(k); return r; };
    p.cat0 = take(cat); p.cat1 = take(cat);
    p.r = take(omap); p.s = take(omap); p.t = take(omap); p.xa = take(omap); p.xb = take(omap);
    p.xp = take(xp);
    p.part = take(z.part); p.tok = take(z.tok); p.wpad = take(z.wpad);
    p.u0 = take((size_t)n * mdim * hw2); p.u1 = take((size_t)n * (mdim / 2) * hw2); p.u2 = take((size_t)n * (mdim / 2) * ihw);
    p.vec = take((size_t)4 * n * 4 * mdim);
    p.ws_floats = ws; p.pack_floats = pk;
    if (out) *out = p;
    return PT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------------------
int dec_conv1(const float* in, long in_sn, const float* w, const float* bias, float* out, long out_sn, int n, int Cin, int Cout, int HW,
              int relu, hipStream_t st) {
    // enough workgroups for the chip with 64 positions each, else 16 positions each (layer4: 2048 -> 256 on 390 positions)
    const bool wide = (long)((HW + 63) / 64) * (Cout / 16) * n >= 512;
    if (wide) hipLaunchKernelGGL(k_dec_conv1<4>, dim3((HW + 63) / 64, Cout / 16, n), dim3(256), 0, st, in, in_sn, w, bias, out, out_sn, Cin, HW, relu);
    else hipLaunchKernelGGL(k_dec_conv1<1>, dim3((HW + 15) / 16, Cout / 16, n), dim3(256), 0, st, in, in_sn, w, bias, out, out_sn, Cin, HW, relu);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// 3x3 convolution of the dense map `in` (n, Cin, H, W): partial maps at base + P.part
int dec_conv3(const DecPlan& P, const DecConv3& c, const float* in, const float* pack, float* base, int H, int W, hipStream_t st) {
    const int HW = H * W;
    float* part = base + P.part;
    if (c.route == ROUTE_BANDED)
        return pt_launch_mf_corr_tm(in, (long)c.Cin * HW, pack + c.w, part, P.n, c.Cout, c.Cin, H, W, c.parts, st);
    const int M = P.n * HW;
    float* X = base + P.tok;
    hipLaunchKernelGGL(k_iou_tokens, dim3((HW + 31) / 32, c.Cpad / 32, P.n), dim3(256), 0, st, in, X, c.Cin, c.Cpad, HW);
    PT_CHECK_LAUNCH();
    const float* w = pack + c.w;
    if (c.Cpad != c.Cin) {
        const long total = (long)c.Cout * 9 * c.Cpad;
        hipLaunchKernelGGL(k_iou_padw, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, base + P.wpad, c.Cin, c.Cpad, total);
        PT_CHECK_LAUNCH();
        w = base + P.wpad;
    }
    GemmArgs g = gemm_args(X, c.Cpad, M, w, M, c.Cout, 9 * c.Cpad, nullptr, part, c.Cout);
    g.H = H; g.Wd = W; g.Cin = c.Cpad; g.HW = HW; g.ksteps = c.Cpad / 64; g.c_zstride = (long)M * c.Cout; g.nchw = 1;
    return launch_gemm(g, st, true);
}

int dec_epi(const DecPlan& P, const DecConv3& c, const float* pack, const float* base, const float* res, int relu, float* out, long out_sn,
            int HW, hipStream_t st) {
    DecEpi e{};
    e.part = base + P.part; e.scale = pack + c.s; e.shift = pack + c.b; e.res = res; e.out = out;
    e.count = (long)P.n * c.Cout * HW; e.out_sn = out_sn; e.parts = c.parts; e.C = c.Cout; e.HW = HW; e.relu = relu;
    e.vec = (HW % 4) == 0 && (out_sn % 4) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)res % 16) == 0;
    hipLaunchKernelGGL(k_dec_epilogue, dim3((unsigned)((e.count + 1023) / 1024)), dim3(256), 0, st, e);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// relu(h + conv3x3_nobias(relu(affine(conv3x3(h))))), h = conv1x1(in): h and mid are scratch maps, out may be `in`
int dec_rrb(const DecPlan& P, const DecRRB& r, const float* in, float* h, float* mid, float* out, const float* pack, float* base, int oc,
            int H, int W, hipStream_t st) {
    const int HW = H * W;
    const long sn = (long)oc * HW;
    int rc;
    if ((rc = dec_conv1(in, sn, pack + r.w1, pack + r.b1, h, sn, P.n, oc, oc, HW, 0, st))) return rc;
    if ((rc = dec_conv3(P, r.a, h, pack, base, H, W, st))) return rc;
    if ((rc = dec_epi(P, r.a, pack, base, nullptr, 1, mid, sn, HW, st))) return rc;
    if ((rc = dec_conv3(P, r.b, mid, pack, base, H, W, st))) return rc;
    return dec_epi(P, r.b, pack, base, h, 1, out, sn, HW, st);
}

int dec_resize(const float* in, float* out, long out_sn, int n, int C, int Hi, int Wi, int Ho, int Wo, int bicubic, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_resize, dim3((Ho * Wo + 255) / 256, C, n), dim3(256), 0, st, in, out, out_sn, C, Hi, Wi, Ho, Wo,
                       (float)Hi / (float)Ho, (float)Wi / (float)Wo, bicubic);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

int dec_mean(const float* in, long in_sn, float* out, int n, int C, int HW, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_mean, dim3(C, n), dim3(256), 0, st, in, in_sn, out, C, HW);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

}  // namespace

extern "C" size_t pt_lwl_decoder_pack_floats(int levels, const int* fc, int ic, int mdim, int use_bn) {
    (void)use_bn;                                    // scale / shift are stored for every 3x3 convolution either way
    const int hw[8] = {1, 1, 1, 1, 1, 1, 1, 1}, one[2] = {1, 1};
    DecPlan p;
    return dec_plan(1, levels, fc, hw, one, one, ic, mdim, &p) == PT_OK ? p.pack_floats : 0;
}

extern "C" size_t pt_lwl_decoder_ws_bytes(int n, int levels, const int* fc, const int* hw, const int* score_hw, const int* image_hw, int ic,
                                          int mdim) {
    DecPlan p;
    return dec_plan(n, levels, fc, hw, score_hw, image_hw, ic, mdim, &p) == PT_OK ? p.ws_floats * sizeof(float) : 0;
}

extern "C" int pt_lwl_decoder_f32(const float* scores, const float* const* feats, const float* pack, float* mask_out, float* const* dec_out,
                                  int n, int levels, const int* fc, const int* hw, const int* score_hw, const int* image_hw, int ic, int mdim,
                                  void* ws, size_t ws_bytes, void* stream) {
    if (!scores || !feats || !pack || !mask_out || !ws) return PT_ERR_NULL;
    DecPlan P;
    int rc = dec_plan(n, levels, fc, hw, score_hw, image_hw, ic, mdim, &P);
    if (rc) return rc;
    for (int l = 0; l < levels; ++l) {
        if (!feats[l]) return PT_ERR_NULL;
        if (((uintptr_t)feats[l] % 4) || (dec_out && dec_out[l] && ((uintptr_t)dec_out[l] % 16))) return PT_ERR_UNSUPPORTED;
    }
    if (((uintptr_t)pack % 16) || ((uintptr_t)scores % 4) || ((uintptr_t)mask_out % 4)) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < P.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    float *CAT0 = base + P.cat0, *CAT1 = base + P.cat1, *R = base + P.r, *S = base + P.s, *T = base + P.t, *XP = base + P.xp;
    const int vs = n * 4 * mdim;
    float *hp = base + P.vec, *ms = hp + vs, *dp = ms + vs, *gate = dp + vs;
    const float* xprev = nullptr;
    for (int l = 0; l < levels; ++l) {
        const DecLevel& L = P.L[l];
        const int HW = L.HW, oc = L.oc, nc = L.nc;
        const long sn = (long)oc * HW, csn = (long)nc * HW;
        if (l > 0) {
            const DecLevel& Q = P.L[l - 1];
            if ((rc = dec_conv1(xprev, (long)Q.oc * Q.HW, pack + L.proj_w, pack + L.proj_b, XP, (long)oc * Q.HW, n, Q.oc, oc, Q.HW, 1, st))) return rc;
        }
        // TSE: reduce, concatenation with the resized scores, transform
        if ((rc = dec_conv1(feats[l], (long)L.fc * HW, pack + L.red0_w, pack + L.red0_b, R, sn, n, L.fc, oc, HW, 1, st))) return rc;
        if ((rc = dec_conv1(R, sn, pack + L.red1_w, pack + L.red1_b, CAT0, csn, n, oc, oc, HW, 0, st))) return rc;
        if ((rc = dec_resize(scores, CAT0 + sn, csn, n, ic, P.SH, P.SW, L.H, L.W, 0, st))) return rc;
        if (l == 0 && (rc = dec_mean(CAT0, csn, hp, n, oc, HW, st))) return rc;
        if ((rc = dec_conv3(P, L.tr[0], CAT0, pack, base, L.H, L.W, st))) return rc;
        if ((rc = dec_epi(P, L.tr[0], pack, base, nullptr, 1, CAT1, csn, HW, st))) return rc;
        if ((rc = dec_conv3(P, L.tr[1], CAT1, pack, base, L.H, L.W, st))) return rc;
        if ((rc = dec_epi(P, L.tr[1], pack, base, nullptr, 1, CAT0, csn, HW, st))) return rc;
        if ((rc = dec_conv3(P, L.tr[2], CAT0, pack, base, L.H, L.W, st))) return rc;
        if ((rc = dec_epi(P, L.tr[2], pack, base, nullptr, 1, R, sn, HW, st))) return rc;
        if ((rc = dec_rrb(P, L.r1, R, S, T, R, pack, base, oc, L.H, L.W, st))) return rc;
        // CAB
        if ((rc = dec_mean(R, sn, ms, n, oc, HW, st))) return rc;
        const DecLevel& Q = P.L[l > 0 ? l - 1 : 0];
        if (l > 0 && (rc = dec_mean(XP, (long)oc * Q.HW, dp, n, oc, Q.HW, st))) return rc;
        hipLaunchKernelGGL(k_dec_cab, dim3(n), dim3(256), 0, st, ms, l == 0 ? hp : dp, pack + L.cab_w1, pack + L.cab_b1, pack + L.cab_w2,
                           pack + L.cab_b2, gate, oc);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_dec_gate, dim3((HW + 255) / 256, n * oc), dim3(256), 0, st, R, gate, hp, l == 0 ? nullptr : XP, T, L.H, L.W, Q.H,
                           Q.W, (float)Q.H / (float)L.H, (float)Q.W / (float)L.W);
        PT_CHECK_LAUNCH();
        float* xout = (dec_out && dec_out[l]) ? dec_out[l] : base + ((l & 1) ? P.xb : P.xa);
        if ((rc = dec_rrb(P, L.r2, T, S, R, xout, pack, base, oc, L.H, L.W, st))) return rc;
        xprev = xout;
    }
    // Upsampler
    const DecLevel& L = P.L[levels - 1];
    float *U0 = base + P.u0, *U1 = base + P.u1, *U2 = base + P.u2;
    const int HW2 = P.H2 * P.W2, half = mdim / 2;
    if ((rc = dec_resize(xprev, U0, (long)mdim * HW2, n, mdim, L.H, L.W, P.H2, P.W2, 1, st))) return rc;
    if ((rc = dec_conv3(P, P.up1, U0, pack, base, P.H2, P.W2, st))) return rc;
    if ((rc = dec_epi(P, P.up1, pack, base, nullptr, 1, U1, (long)half * HW2, HW2, st))) return rc;
    if ((rc = dec_resize(U1, U2, (long)half * P.IH * P.IW, n, half, P.H2, P.W2, P.IH, P.IW, 1, st))) return rc;
    hipLaunchKernelGGL(k_dec_conv_out, dim3((P.IW + 63) / 64, (P.IH + 3) / 4, n), dim3(256), 0, st, U2, pack + P.up2_w, pack + P.up2_b, mask_out,
                       half, P.IH, P.IW);
    PT_CHECK_LAUNCH();
    return PT_OK;
}
