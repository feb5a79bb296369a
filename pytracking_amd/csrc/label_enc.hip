// Mask label encoder: ResidualDS16SW.forward (ltr/models/lwl/label_encoder.py:9-55 = ltr/models/rts/label_encoder.py:9-55) in six launches.
//
//   x (n,1,H,W) -> conv3x3 s2 p1 (1->C0) [+BN] + ReLU -> maxpool3x3 s2 p1                                        k_le_stem
//               -> BasicBlock(C0->C1, s2): relu(bn2(conv2(relu(bn1(conv1 x)))) + downsample(x))                  k_le_conv x 2
//               -> BasicBlock(C1->C2, s2)                                                                        k_le_conv x 2
//               -> label_pred = relu([bn](conv3x3(C2->F)))  ;  samp_w_pred = conv3x3(C2->F)                      k_le_conv x 1
//
// LWL and RTS call it on every stored mask on every frame (lwl.py:560-564, rts.py:688): up to 32 masks of 480 x 832.
//
// k_le_stem (VALU: Cin = 1 is nine MACs per output, nothing for the matrix pipe): one workgroup = a 4 x 32 tile of POOLED outputs of one
//   mask, all C0 channels.  The 19 x 132 mask tile with its halo is staged in LDS (10 KB, zero filled outside the mask = the convolution's
//   padding); a thread reads its 7 x 7 patch as two 16-byte LDS reads per row, and per channel computes the nine convolution outputs of
//   its pooling window in registers, applies scale / shift / ReLU and takes the maximum over the window positions that exist (pooling
//   padding = positions ignored, as nn.MaxPool2d's -inf).  The convolution output never goes to memory.
//
// k_le_conv<S, M, T> (exact fp32 MFMA 16x16x4, implicit GEMM): one workgroup of 4 waves = 4M output rows x 16 output columns of one image
//   x 16T output channels.  Per 16 input channels the input tile with its halo is staged in LDS (zero filled outside the map); wave w
//   owns rows w*M .. w*M + M - 1 and holds M x T accumulator tiles D[channel][pixel].  Per tap and 16-channel chunk a lane loads ONE
//   16-byte piece of the tap-major weights per channel tile (w[co][tap][ci0 + 4*(l>>4) .. + 3]) and reads M x 4 input values from LDS:
//   k-step s of the chunk pairs lane group l>>4 with input channel ci0 + 4*(l>>4) + s on both operands (the order of a sum's terms is
//   free as long as A and B agree).  T + 4M loads per 4MT MFMAs.  The channel planes in LDS are padded to 8 mod 16 floats: the two
//   16-lane groups a ds_read_b32 half serves then sit 32 banks apart (stride-1 and stride-2 columns both conflict free).
//   Epilogue: y = acc * scale[co] + shift[co] (+ residual[co]) (ReLU for co < relu_n), written to out0 (co < csplit) or out1.
//   No atomics, no split accumulation: repeated calls are bit-identical.
#include <algorithm>
#include <math.h>
#include "common.h"
#include "pt_internal.h"

namespace {

constexpr int LE_MAX_C = 64, LE_MAX_DIM = 8192, LE_MAX_N = 65535;
constexpr int ST_TH = 4, ST_TW = 32, ST_THREADS = ST_TH * ST_TW;
constexpr int ST_LR = 4 * ST_TH + 3, ST_LC = 4 * ST_TW + 4;              // LDS tile: origin row 4*py0 - 3, origin column 4*px0 - 4

// grid (ceil(W2/32), ceil(H2/4), n), 128 threads
__global__ __launch_bounds__(ST_THREADS) void k_le_stem(const float* __restrict__ mask, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ out, int C0, int H, int W, int H1, int W1, int H2, int W2) {
    __shared__ __attribute__((aligned(16))) float tile[ST_LR * ST_LC];
    const int img = blockIdx.z, py0 = blockIdx.y * ST_TH, px0 = blockIdx.x * ST_TW;
    const float* src = mask + (long)img * H * W;
    const int r0 = 4 * py0 - 3, c0 = 4 * px0 - 4;
    for (int e = threadIdx.x; e < ST_LR * ST_LC; e += ST_THREADS) {
        const int r = e / ST_LC, c = e - r * ST_LC, iy = r0 + r, ix = c0 + c;
        tile[e] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? src[(long)iy * W + ix] : 0.f;
    }
    __syncthreads();
    const int lx = threadIdx.x % ST_TW, ly = threadIdx.x / ST_TW, py = py0 + ly, px = px0 + lx;
    if (py >= H2 || px >= W2) return;                                    // behind the only barrier
    float p[7][8];                                                       // p[ry][q + 1] = mask(4*py - 3 + ry, 4*px - 3 + q)
#pragma unroll
    for (int ry = 0; ry < 7; ++ry) {
        const f32x4 lo = *(const f32x4*)&tile[(4 * ly + ry) * ST_LC + 4 * lx], hi = *(const f32x4*)&tile[(4 * ly + ry) * ST_LC + 4 * lx + 4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { p[ry][u] = lo[u]; p[ry][4 + u] = hi[u]; }
    }
    bool ok[3][3];                                                       // does convolution output (2*py - 1 + a, 2*px - 1 + b) exist
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int cy = 2 * py - 1 + a, cx = 2 * px - 1 + b;
            ok[a][b] = cy >= 0 && cy < H1 && cx >= 0 && cx < W1;
        }
    const long plane = (long)H2 * W2;
    float* o = out + (long)img * C0 * plane + (long)py * W2 + px;
    for (int c = 0; c < C0; ++c) {
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
                    for (int kx = 0; kx < 3; ++kx) v = fmaf(wk[ky * 3 + kx], p[2 * a + ky][2 * b + kx + 1], v);
                v = fmaxf(fmaf(v, sc, sh), 0.f);
                m = ok[a][b] ? fmaxf(m, v) : m;                          // the centre (a = b = 1) always exists
            }
        o[c * plane] = m;
    }
}

struct LeConv {
    const float* in; long in_img;                // input (n, Cin, Hi, Wi) view: image stride in floats, channel stride Hi * Wi
    const float* w; const float* scale; const float* shift;      // (Cout, 3, 3, Cin), (Cout), (Cout)
    const float* res; long res_img;              // optional residual (n, Cout, Ho, Wo) view
    float* out0; long out0_img; float* out1; long out1_img;      // channels < csplit -> out0[co], the others -> out1[co - csplit]
    int csplit, Cin, Cout, Hi, Wi, Ho, Wo, relu_n, groups;
};

constexpr int le_plane(int S, int M) {           // floats per channel plane of the LDS tile, padded to 8 mod 16
    const int raw = ((4 * M - 1) * S + 3) * (15 * S + 3);
    return raw + ((8 - raw % 16) + 16) % 16;
}

// grid (ceil(Wo/16), ceil(Ho/(4M)) * groups, n), 256 threads; groups = Cout / (16 T)
template <int S, int M, int T>
__global__ __launch_bounds__(256) void k_le_conv(LeConv a) {
    constexpr int TRI = (4 * M - 1) * S + 3, TCI = 15 * S + 3, PL = le_plane(S, M);
    __shared__ float tile[16 * PL];
    const int img = blockIdx.z, g = blockIdx.y % a.groups, oy0 = (blockIdx.y / a.groups) * (4 * M), ox0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, j = lane & 15;
    const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    const long cstride = (long)a.Hi * a.Wi;
    const float* src = a.in + (long)img * a.in_img;
    f32x4 acc[M][T];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int t = 0; t < T; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wl = a.w + ((long)(g * T * 16 + j) * 9) * a.Cin + 4 * kq;           // + (t * 16 * 9 + tap) * Cin + ci0
    for (int ci0 = 0; ci0 < a.Cin; ci0 += 16) {
        if (ci0) __syncthreads();
        for (int e = threadIdx.x; e < 16 * TRI * TCI; e += 256) {
            const int c = e / (TRI * TCI), rem = e - c * (TRI * TCI), r = rem / TCI, col = rem - r * TCI, iy = iy0 + r, ix = ix0 + col;
            tile[c * PL + rem] = (iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) ? src[(ci0 + c) * cstride + (long)iy * a.Wi + ix] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            f32x4 wv[T];
#pragma unroll
            for (int t = 0; t < T; ++t) wv[t] = *(const f32x4*)(wl + ((long)t * 16 * 9 + tap) * a.Cin + ci0);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float b = tile[(4 * kq + s) * PL + ((wave * M + m) * S + ky) * TCI + j * S + kx];
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[m][t] = mfma16(wv[t][s], b, acc[m][t]);
                }
        }
    }
    const long oplane = (long)a.Ho * a.Wo;
    const int ox = ox0 + j;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int oy = oy0 + wave * M + m;
        if (oy >= a.Ho || ox >= a.Wo) continue;
        const long pix = (long)oy * a.Wo + ox;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = (g * T + t) * 16 + 4 * kq + r;
                float v = fmaf(acc[m][t][r], a.scale[co], a.shift[co]);
                if (a.res) v += a.res[(long)img * a.res_img + co * oplane + pix];
                if (co < a.relu_n) v = fmaxf(v, 0.f);
                if (co < a.csplit) a.out0[(long)img * a.out0_img + co * oplane + pix] = v;
                else a.out1[(long)img * a.out1_img + (co - a.csplit) * oplane + pix] = v;
            }
    }
}

struct LeLayer { int Cin, Cout; size_t w_off, s_off, b_off; };           // offsets into the pack, floats
struct LePlan {
    int n, C[4], H[5], W[5];                     // H[0] mask, H[1] stem conv, H[2] pool, H[3] block 1, H[4] block 2 and the heads
    LeLayer stem, conv[5];                       // conv: res1.conv1|downsample, res1.conv2, res2.conv1|downsample, res2.conv2, heads
    size_t s0, t1, r1, t2, r2, ws_floats, pack_floats;                   // workspace offsets, floats
};

int le_plan(int n, int H, int W, int c0, int c1, int c2, int f, LePlan* out) {
    if (n <= 0 || H <= 0 || W <= 0 || c0 <= 0 || c1 <= 0 || c2 <= 0 || f <= 0) return PT_ERR_SHAPE;
    for (int c : {c0, c1, c2, f})
        if (c % 16 || c > LE_MAX_C) return PT_ERR_UNSUPPORTED;
    if (n > LE_MAX_N || H > LE_MAX_DIM || W > LE_MAX_DIM) return PT_ERR_UNSUPPORTED;
    LePlan p{};
    p.n = n; p.C[0] = c0; p.C[1] = c1; p.C[2] = c2; p.C[3] = f;
    p.H[0] = H; p.W[0] = W;
    for (int k = 1; k < 5; ++k) { p.H[k] = (p.H[k - 1] - 1) / 2 + 1; p.W[k] = (p.W[k - 1] - 1) / 2 + 1; }
    size_t pk = 0;
    auto layer = [&](LeLayer& L, int cin, int cout) {
        L.Cin = cin; L.Cout = cout;
        L.w_off = pk; pk += (size_t)cout * 9 * cin;
        L.s_off = pk; pk += cout;
        L.b_off = pk; pk += cout;
    };
    layer(p.stem, 1, c0);
    layer(p.conv[0], c0, 2 * c1); layer(p.conv[1], c1, c1);
    layer(p.conv[2], c1, 2 * c2); layer(p.conv[3], c2, c2);
    layer(p.conv[4], c2, 2 * f);
    p.pack_floats = pk;
    size_t ws = 0;
    auto take = [&](size_t k) { size_t r = ws; ws += pt_align_floats(k); return r; };
    const size_t hw2 = (size_t)p.H[2] * p.W[2], hw3 = (size_t)p.H[3] * p.W[3], hw4 = (size_t)p.H[4] * p.W[4];
    p.s0 = take((size_t)n * c0 * hw2);
    p.t1 = take((size_t)n * 2 * c1 * hw3);
    p.r1 = take((size_t)n * c1 * hw3);
    p.t2 = take((size_t)n * 2 * c2 * hw4);
    p.r2 = take((size_t)n * c2 * hw4);
    p.ws_floats = ws;
    if (out) *out = p;
    return PT_OK;
}

template <int S, int M>
int le_launch_t(const LeConv& a, int T, dim3 grid, hipStream_t st) {
    switch (T) {
        case 4: hipLaunchKernelGGL((k_le_conv<S, M, 4>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_le_conv<S, M, 2>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_le_conv<S, M, 1>), grid, dim3(256), 0, st, a); break;
    }
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// Tile choice from the shape alone: the largest (rows per wave M, channel tiles per workgroup T) that still gives two workgroups per CU;
// below that the smallest tile (most workgroups) -- the late layers of a single mask have fewer than 256 tiles in any case.
int le_conv(LeConv a, int S, int n, hipStream_t st) {
    const int ct = a.Cout / 16, tmax = ct % 4 == 0 ? 4 : (ct % 2 == 0 ? 2 : 1);
    int M = 1, T = 1;
    const int cand[4][2] = {{2, tmax}, {1, tmax}, {1, tmax >= 2 ? tmax / 2 : 1}, {1, 1}};
    for (const auto& c : cand) {
        M = c[0]; T = c[1];
        const long wgs = (long)pt_ceil_div(a.Wo, 16) * pt_ceil_div(a.Ho, 4 * M) * (ct / T) * n;
        if (wgs >= 512) break;
    }
    a.groups = ct / T;
    const dim3 grid(pt_ceil_div(a.Wo, 16), pt_ceil_div(a.Ho, 4 * M) * a.groups, n);      // y <= 512 * 8 (LE_MAX_DIM), z <= LE_MAX_N
    if (S == 2) return M == 2 ? le_launch_t<2, 2>(a, T, grid, st) : le_launch_t<2, 1>(a, T, grid, st);
    return M == 2 ? le_launch_t<1, 2>(a, T, grid, st) : le_launch_t<1, 1>(a, T, grid, st);
}

}  // namespace

size_t pt_label_enc_pack_floats_impl(int c0, int c1, int c2, int f) {
    LePlan p;
    return le_plan(1, 1, 1, c0, c1, c2, f, &p) == PT_OK ? p.pack_floats : 0;
}

size_t pt_label_enc_ws_bytes_impl(int n, int H, int W, int c0, int c1, int c2, int f) {
    LePlan p;
    return le_plan(n, H, W, c0, c1, c2, f, &p) == PT_OK ? p.ws_floats * sizeof(float) : 0;
}

int pt_label_enc_impl(const float* masks, const float* pack, float* label_enc, float* sample_w, int n, int H, int W, int c0, int c1,
                      int c2, int f, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!masks || !pack || !label_enc || !sample_w || !ws) return PT_ERR_NULL;
    LePlan p;
    int rc = le_plan(n, H, W, c0, c1, c2, f, &p);
    if (rc) return rc;
    if ((uintptr_t)pack % 16) return PT_ERR_UNSUPPORTED;                 // 16-byte weight loads
    for (const void* q : {(const void*)masks, (const void*)label_enc, (const void*)sample_w})
        if ((uintptr_t)q % 4) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < p.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    const long hw3 = (long)p.H[3] * p.W[3], hw4 = (long)p.H[4] * p.W[4];
    hipLaunchKernelGGL(k_le_stem, dim3(pt_ceil_div(p.W[2], ST_TW), pt_ceil_div(p.H[2], ST_TH), n), dim3(ST_THREADS), 0, st, masks,
                       pack + p.stem.w_off, pack + p.stem.s_off, pack + p.stem.b_off, base + p.s0, c0, H, W, p.H[1], p.W[1], p.H[2],
                       p.W[2]);
    PT_CHECK_LAUNCH();
    auto conv = [&](int k, const float* in, long in_img, int Hi, int Wi, int Ho, int Wo) {
        const LeLayer& L = p.conv[k];
        LeConv a{};
        a.in = in; a.in_img = in_img;
        a.w = pack + L.w_off; a.scale = pack + L.s_off; a.shift = pack + L.b_off;
        a.Cin = L.Cin; a.Cout = L.Cout; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
        a.csplit = L.Cout; a.out0_img = (long)L.Cout * Ho * Wo;
        return a;
    };
    // block 1: conv1 | downsample as one convolution with 2 C1 outputs (ReLU on the conv1 half), then conv2 + residual + ReLU
    LeConv a = conv(0, base + p.s0, (long)c0 * p.H[2] * p.W[2], p.H[2], p.W[2], p.H[3], p.W[3]);
    a.out0 = base + p.t1; a.relu_n = c1;
    if ((rc = le_conv(a, 2, n, st))) return rc;
    a = conv(1, base + p.t1, 2 * c1 * hw3, p.H[3], p.W[3], p.H[3], p.W[3]);
    a.res = base + p.t1 + c1 * hw3; a.res_img = 2 * c1 * hw3; a.out0 = base + p.r1; a.relu_n = c1;
    if ((rc = le_conv(a, 1, n, st))) return rc;
    // block 2
    a = conv(2, base + p.r1, c1 * hw3, p.H[3], p.W[3], p.H[4], p.W[4]);
    a.out0 = base + p.t2; a.relu_n = c2;
    if ((rc = le_conv(a, 2, n, st))) return rc;
    a = conv(3, base + p.t2, 2 * c2 * hw4, p.H[4], p.W[4], p.H[4], p.W[4]);
    a.res = base + p.t2 + c2 * hw4; a.res_img = 2 * c2 * hw4; a.out0 = base + p.r2; a.relu_n = c2;
    if ((rc = le_conv(a, 1, n, st))) return rc;
    // heads: label_pred | samp_w_pred as one convolution with 2 F outputs, ReLU on label_pred's half, written to the two results
    a = conv(4, base + p.r2, c2 * hw4, p.H[4], p.W[4], p.H[4], p.W[4]);
    a.csplit = f; a.out0 = label_enc; a.out0_img = f * hw4; a.out1 = sample_w; a.out1_img = f * hw4; a.relu_n = f;
    return le_conv(a, 1, n, st);
}
