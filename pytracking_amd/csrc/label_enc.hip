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
#include "ds16_enc.h"
#include "box_slice.h"

namespace {

constexpr int LE_MAX_C = 64, LE_MAX_DIM = 8192, LE_MAX_N = 65535;
constexpr Ds16Limits LE_LIMITS{LE_MAX_C, LE_MAX_DIM, LE_MAX_N};
constexpr int ST_TH = 4, ST_TW = 32, ST_THREADS = ST_TH * ST_TW;
constexpr int ST_LR = 4 * ST_TH + 3, ST_LC = 4 * ST_TW + 4;              // LDS tile: origin row 4*py0 - 3, origin column 4*px0 - 4

// grid (ceil(W2/32), ceil(H2/4), n), 128 threads.  BOX: `mask` holds n boxes (x, y, w, h) instead of n masks and the tile is filled with
// the binary mask ResidualDS16FeatSWBox.bbox_to_mask writes (box_slice.h; starts clamped at 0); nothing of image size is loaded or stored.
template <bool BOX>
__global__ __launch_bounds__(ST_THREADS) void k_le_stem(const float* __restrict__ mask, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ out, int C0, int H, int W, int H1, int W1, int H2, int W2) {
    __shared__ __attribute__((aligned(16))) float tile[ST_LR * ST_LC];
    const int img = blockIdx.z, py0 = blockIdx.y * ST_TH, px0 = blockIdx.x * ST_TW;
    const int r0 = 4 * py0 - 3, c0 = 4 * px0 - 4;
    if constexpr (BOX) {
        const PtBoxRect box = pt_box_rect(mask + 4 * (long)img, H, W, true);         // inside [0, W] x [0, H]
        for (int e = threadIdx.x; e < ST_LR * ST_LC; e += ST_THREADS) {
            const int r = e / ST_LC, c = e - r * ST_LC, iy = r0 + r, ix = c0 + c;
            tile[e] = (iy >= box.y0 && iy < box.y1 && ix >= box.x0 && ix < box.x1) ? 1.f : 0.f;
        }
    } else {
        const float* src = mask + (long)img * H * W;
        for (int e = threadIdx.x; e < ST_LR * ST_LC; e += ST_THREADS) {
            const int r = e / ST_LC, c = e - r * ST_LC, iy = r0 + r, ix = c0 + c;
            tile[e] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? src[(long)iy * W + ix] : 0.f;
        }
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

size_t pt_label_enc_pack_floats_impl(int c0, int c1, int c2, int f) { return ds16_pack_floats(2, LE_LIMITS, c0, c1, c2, f); }

size_t pt_label_enc_ws_bytes_impl(int n, int H, int W, int c0, int c1, int c2, int f) {
    return ds16_ws_bytes(2, LE_LIMITS, n, H, W, c0, c1, c2, f);
}

namespace {

template <bool BOX>
int le_stem(const float* in, const Ds16Plan& p, const float* pk, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_le_stem<BOX>, dim3(pt_ceil_div(p.W[2], ST_TW), pt_ceil_div(p.H[2], ST_TH), p.n), dim3(ST_THREADS), 0, st, in,
                       pk + p.stem.w_off, pk + p.stem.s_off, pk + p.stem.b_off, out, p.C[0], p.H[0], p.W[0], p.H[1], p.W[1], p.H[2], p.W[2]);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

int le_conv_ds16(const Ds16Conv& c, int images, hipStream_t st) {
    LeConv a{};
    a.in = c.in; a.in_img = c.in_img;
    a.w = c.w; a.scale = c.scale; a.shift = c.shift;
    a.res = c.res; a.res_img = c.res_img;
    a.out0 = c.out0; a.out0_img = c.out0_img; a.out1 = c.out1; a.out1_img = c.out1_img;
    a.csplit = c.csplit; a.Cin = c.Cin; a.Cout = c.Cout; a.Hi = c.Hi; a.Wi = c.Wi; a.Ho = c.Ho; a.Wo = c.Wo; a.relu_n = c.relu_n;
    return le_conv(a, c.stride, images, st);
}

}  // namespace

int pt_label_enc_impl(const float* masks, const float* pack, float* label_enc, float* sample_w, int n, int H, int W, int c0, int c1,
                      int c2, int f, void* ws, size_t ws_bytes, hipStream_t st) {
    auto stem = [&](const Ds16Plan& p, const float* pk, float* out) { return le_stem<false>(masks, p, pk, out, st); };
    auto conv = [&](const Ds16Conv& c, int images) { return le_conv_ds16(c, images, st); };
    return ds16_encode(2, LE_LIMITS, false, masks, pack, label_enc, sample_w, n, H, W, c0, c1, c2, f, ws, ws_bytes, stem, conv);
}

// The mask trunk of ResidualDS16FeatSWBox for box_enc.hip: the plan of the (c0, c1, c2) trunk on n H x W images (the heads' slot of the
// plan is filled with c2 and not used), and the five launches from the boxes; `ws` holds p.ws_floats floats, the trunk output
// (n, c2, H[4], W[4]) ends at ws + p.r2.  The caller has checked its arguments.
int pt_le_box_trunk_plan(int n, int H, int W, int c0, int c1, int c2, Ds16Plan* p) {
    return ds16_plan(2, LE_LIMITS, n, H, W, c0, c1, c2, c2, p);
}

int pt_le_box_trunk_launch(const float* boxes, const float* pack, const Ds16Plan& p, float* ws, hipStream_t st) {
    auto stem = [&](const Ds16Plan& q, const float* pk, float* out) { return le_stem<true>(boxes, q, pk, out, st); };
    auto conv = [&](const Ds16Conv& c, int images) { return le_conv_ds16(c, images, st); };
    return ds16_trunk(2, p, pack, ws, stem, conv);
}
