// Segmentation read-out of LWL / RTS: what the trackers run on the CPU between the decoder's raw score map and the next frame's label
// encoder (pytracking/tracker/lwl/lwl.py:210-359, pytracking/tracker/rts/rts.py:340-493, pytracking/features/preprocessing.py:131-146).
//
//   pt_seg_readout_f32        convert_scores_crop_to_image + `> 0` + sigmoid + the sums of get_target_state / masks_to_bboxes   k_seg_readout, k_seg_finish
//   pt_seg_state_f32          the same statistics of a probability image that already exists                                   k_seg_state,   k_seg_finish
//   pt_seg_merge_f32          merge_results' soft aggregation, arg-max and the per-object statistics                           k_seg_merge<N>, k_seg_finish
//   pt_sample_mask_patch_f32  sample_patch(is_mask=True): strided view, zero padding, legacy nearest resize                    k_mask_patch
//
// Every image kernel works on tiles of ST_TH x ST_TW = 16 x 64 pixels, one workgroup of 256 threads per tile, a thread = 4 consecutive
// pixels of a row (16-byte loads and stores when the row length is a multiple of 4 and the pointer allows, scalar otherwise).
//
// Statistics: the reference sums rows and columns first and centres on e_y / e_x afterwards; so do we.  `tile_partials` leaves, per tile,
// the 16 row sums (over the tile's 64 columns) and the 64 column sums (over its 16 rows) of three quantities -- p, max(p, 0), mask -- in
// the workspace: row partials [q][tile column][H], column partials [q][tile row][W].  k_seg_finish (one workgroup of 1024 threads per
// statistics block) adds the partials of a row / column in tile order, then reduces prob_sum, the first moments, and -- with e_y, e_x
// known -- the centred second moments, the mask count and the mask's extent.  Every sum has one fixed order (serial inside a thread, then
// a wave shuffle tree, then the waves in order); no atomics: repeated calls are bit-identical, and pt_seg_state_f32 on the read-out's own
// prob_im / mask_im repeats the read-out's statistics bit for bit.
//
// k_seg_merge<N>: the N + 1 scores of a pixel (background first) stay in registers; the loop over the output index i is rolled (the
// score s_i is picked by a chain of uniform selects), the sum over j is unrolled and runs in the reference's order j = 0 .. N:
// out_i = 1 / sum_j exp(s_j - s_i).  exp overflows to inf exactly where the reference's does (1 / inf = 0) and no difference of two
// finite scores is NaN.
#include <math.h>
#include "common.h"
#include "pt_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned char u8x4 __attribute__((ext_vector_type(4)));

constexpr int ST_TH = 16, ST_TW = 64, ST_THREADS = 256, ST_LD = ST_TW + 1;
constexpr int FIN_THREADS = 1024, FIN_WAVES = FIN_THREADS / 64;
constexpr int NQ = 3;                                                    // p, max(p, 0), mask

static inline int tiles_x(int W) { return (W + ST_TW - 1) / ST_TW; }
static inline int tiles_y(int H) { return (H + ST_TH - 1) / ST_TH; }

// workspace of ONE statistics block, in floats: row partials | column partials | row sums | column sums
struct StatWs {
    float *rowp, *colp, *rowf, *colf;
    int H, W, TX, TY;
};
static inline size_t stat_ws_floats(int H, int W) {
    return pt_align_floats((size_t)NQ * tiles_x(W) * H) + pt_align_floats((size_t)NQ * tiles_y(H) * W) + pt_align_floats((size_t)NQ * H) +
           pt_align_floats((size_t)NQ * W);
}
__host__ __device__ inline StatWs stat_ws(float* base, int H, int W, int TX, int TY) {
    StatWs s;
    s.H = H; s.W = W; s.TX = TX; s.TY = TY;
    s.rowp = base;
    s.colp = s.rowp + (((size_t)NQ * TX * H + 63) & ~(size_t)63);
    s.rowf = s.colp + (((size_t)NQ * TY * W + 63) & ~(size_t)63);
    s.colf = s.rowf + (((size_t)NQ * H + 63) & ~(size_t)63);
    return s;
}

__device__ inline float sigmoidf(float s) { return 1.f / (1.f + expf(-s)); }

// The tile's partial sums of p, max(p, 0) and m.  Called by all 256 threads of the workgroup (two barriers); pixels outside the image
// carry p = m = 0.  Thread t holds row t >> 4, columns 4 (t & 15) .. + 3 of the tile.
__device__ inline void tile_partials(float (*sh)[ST_TH][ST_LD], const float p[4], const float m[4], const StatWs& ws) {
    const int t = threadIdx.x, ly = t >> 4, lx = (t & 15) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sh[0][ly][lx + k] = p[k];
        sh[1][ly][lx + k] = fmaxf(p[k], 0.f);
        sh[2][ly][lx + k] = m[k];
    }
    __syncthreads();
    if (t < ST_TW) {                                                     // wave 0: one column each, rows top to bottom
        const int x = blockIdx.x * ST_TW + t;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < ST_TH; ++r) s += sh[q][r][t];
            if (x < ws.W) ws.colp[((size_t)q * ws.TY + blockIdx.y) * ws.W + x] = s;
        }
    } else if (t < 2 * ST_TW) {                                          // wave 1: four lanes per row, 16 columns each, left to right
        const int r = (t - ST_TW) >> 2, qd = (t - ST_TW) & 3, y = blockIdx.y * ST_TH + r;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) s += sh[q][r][qd * 16 + c];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (qd == 0 && y < ws.H) ws.rowp[((size_t)q * ws.TX + blockIdx.x) * ws.H + y] = s;
        }
    }
    __syncthreads();
}

// ---- crop scores -> image scores / probability / mask -------------------------------------------------------------------------------
struct ReadoutArgs {
    const float* scores;
    float *scores_im, *prob_im, *mask_im, *wsbase;
    int Hc, Wc, Hr, Wr, r1, c1, Hi, Wi, vec;
    float rscale;
};

// grid (ceil(Wi/64), ceil(Hi/16)), 256 threads
__global__ __launch_bounds__(ST_THREADS) void k_seg_readout(ReadoutArgs a) {
    __shared__ float sh[NQ][ST_TH][ST_LD];
    const int t = threadIdx.x, y = blockIdx.y * ST_TH + (t >> 4), x0 = blockIdx.x * ST_TW + (t & 15) * 4;
    const bool rowin = y < a.Hi;
    const int ry = y - a.r1;
    const bool yin = rowin && ry >= 0 && ry < a.Hr;
    // F.interpolate(scale_factor=s, mode='bilinear'): src = (dst + 0.5) / s - 0.5 clamped below at 0
    float fy = __fmaf_rn(a.rscale, (float)ry + 0.5f, -0.5f);
    fy = fy < 0.f ? 0.f : fy;
    const int y0 = min((int)fy, a.Hc - 1), y1 = min(y0 + 1, a.Hc - 1);
    const float wy1 = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), wy0 = 1.f - wy1;
    float s[4], p[4], m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k, rx = x - a.c1;
        const bool in = rowin && x < a.Wi;
        float v = -100.f;
        if (yin && in && rx >= 0 && rx < a.Wr) {
            float fx = __fmaf_rn(a.rscale, (float)rx + 0.5f, -0.5f);
            fx = fx < 0.f ? 0.f : fx;
            const int xa = min((int)fx, a.Wc - 1), xb = min(xa + 1, a.Wc - 1);
            const float wx1 = fminf(fmaxf(fx - (float)xa, 0.f), 1.f), wx0 = 1.f - wx1;
            const float* r0 = a.scores + (size_t)y0 * a.Wc;
            const float* r1 = a.scores + (size_t)y1 * a.Wc;
            const float top = r0[xa] * wx0 + r0[xb] * wx1, bot = r1[xa] * wx0 + r1[xb] * wx1;
            v = top * wy0 + bot * wy1;
        }
        s[k] = v;
        p[k] = in ? sigmoidf(v) : 0.f;
        m[k] = (in && v > 0.f) ? 1.f : 0.f;
    }
    if (rowin && x0 < a.Wi) {
        const size_t o = (size_t)y * a.Wi + x0;
        if (a.vec) {                                                     // Wi % 4 == 0: x0 + 3 < Wi
            if (a.scores_im) *(f32x4*)(a.scores_im + o) = f32x4{s[0], s[1], s[2], s[3]};
            if (a.prob_im) *(f32x4*)(a.prob_im + o) = f32x4{p[0], p[1], p[2], p[3]};
            if (a.mask_im) *(f32x4*)(a.mask_im + o) = f32x4{m[0], m[1], m[2], m[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < a.Wi) {
                    if (a.scores_im) a.scores_im[o + k] = s[k];
                    if (a.prob_im) a.prob_im[o + k] = p[k];
                    if (a.mask_im) a.mask_im[o + k] = m[k];
                }
        }
    }
    tile_partials(sh, p, m, stat_ws(a.wsbase, a.Hi, a.Wi, gridDim.x, gridDim.y));
}

// ---- statistics of an existing probability image ---------------------------------------------------------------------------------
// mask: pixels of `mask` > 0 when given, prob > 0.5 otherwise.  grid (ceil(W/64), ceil(H/16)), 256 threads
__global__ __launch_bounds__(ST_THREADS) void k_seg_state(const float* __restrict__ prob, const float* __restrict__ mask, float* wsbase,
                                                          int H, int W, int vec) {
    __shared__ float sh[NQ][ST_TH][ST_LD];
    const int t = threadIdx.x, y = blockIdx.y * ST_TH + (t >> 4), x0 = blockIdx.x * ST_TW + (t & 15) * 4;
    float p[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f}, mk[4] = {0.f, 0.f, 0.f, 0.f};
    if (y < H && x0 < W) {
        const size_t o = (size_t)y * W + x0;
        if (vec) {
            const f32x4 v = *(const f32x4*)(prob + o);
            p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
            if (mask) {
                const f32x4 u = *(const f32x4*)(mask + o);
                mk[0] = u[0]; mk[1] = u[1]; mk[2] = u[2]; mk[3] = u[3];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W) {
                    p[k] = prob[o + k];
                    if (mask) mk[k] = mask[o + k];
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = (x0 + k < W && (mask ? mk[k] > 0.f : p[k] > 0.5f)) ? 1.f : 0.f;
    }
    tile_partials(sh, p, m, stat_ws(wsbase, H, W, gridDim.x, gridDim.y));
}

// ---- the second kernel of every statistics block ---------------------------------------------------------------------------------
// K sums at once, the total to every thread: serial per thread (done by the caller), shuffle tree per wave, the 16 waves in order
template <int K>
__device__ inline void block_sums(float (&v)[K], float (*sh)[FIN_WAVES]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = v[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
        if (lane == 0) sh[k][wv] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < FIN_WAVES; ++w) s += sh[k][w];
        v[k] = s;
    }
    __syncthreads();
}

// grid (blocks of statistics), 1024 threads.  Block b: workspace wsbase + b * ws_stride, result stats + 16 b.
__global__ __launch_bounds__(FIN_THREADS) void k_seg_finish(float* wsbase, size_t ws_stride, float* stats, int H, int W, int TX, int TY) {
    __shared__ float sh[8][FIN_WAVES];
    const StatWs ws = stat_ws(wsbase + blockIdx.x * ws_stride, H, W, TX, TY);
    const int t = threadIdx.x;
    // sums of rows and columns; a thread reads back below only what it wrote itself
    for (int y = t; y < H; y += FIN_THREADS)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s = 0.f;
            for (int tx = 0; tx < TX; ++tx) s += ws.rowp[((size_t)q * TX + tx) * H + y];
            ws.rowf[(size_t)q * H + y] = s;
        }
    for (int x = t; x < W; x += FIN_THREADS)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s = 0.f;
            for (int ty = 0; ty < TY; ++ty) s += ws.colp[((size_t)q * TY + ty) * W + x];
            ws.colf[(size_t)q * W + x] = s;
        }
    // v: prob_sum, sum p y, sum p x, the same of max(p, 0), mask count
    float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float lo_y = INFINITY, hi_y = -1.f, lo_x = INFINITY, hi_x = -1.f;
    for (int y = t; y < H; y += FIN_THREADS) {
        const float r0 = ws.rowf[y], r1 = ws.rowf[(size_t)H + y], rm = ws.rowf[(size_t)2 * H + y];
        v[0] += r0; v[1] += r0 * (float)y;
        v[3] += r1; v[4] += r1 * (float)y;
        v[6] += rm;
        if (rm > 0.f) { lo_y = fminf(lo_y, (float)y); hi_y = fmaxf(hi_y, (float)y); }
    }
    for (int x = t; x < W; x += FIN_THREADS) {
        const float c0 = ws.colf[x], c1 = ws.colf[(size_t)W + x], cm = ws.colf[(size_t)2 * W + x];
        v[2] += c0 * (float)x;
        v[5] += c1 * (float)x;
        if (cm > 0.f) { lo_x = fminf(lo_x, (float)x); hi_x = fmaxf(hi_x, (float)x); }
    }
    block_sums<7>(v, sh);
    const float ey = v[1] / v[0], ex = v[2] / v[0], eyc = v[4] / v[3], exc = v[5] / v[3];
    float u[4] = {0.f, 0.f, 0.f, 0.f};
    for (int y = t; y < H; y += FIN_THREADS) {
        const float d0 = (float)y - ey, d1 = (float)y - eyc;
        u[0] += ws.rowf[y] * (d0 * d0);
        u[2] += ws.rowf[(size_t)H + y] * (d1 * d1);
    }
    for (int x = t; x < W; x += FIN_THREADS) {
        const float d0 = (float)x - ex, d1 = (float)x - exc;
        u[1] += ws.colf[x] * (d0 * d0);
        u[3] += ws.colf[(size_t)W + x] * (d1 * d1);
    }
    block_sums<4>(u, sh);
    // extent of the mask: min / max are exact and order-free
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo_y = fminf(lo_y, __shfl_down(lo_y, d)); hi_y = fmaxf(hi_y, __shfl_down(hi_y, d));
        lo_x = fminf(lo_x, __shfl_down(lo_x, d)); hi_x = fmaxf(hi_x, __shfl_down(hi_x, d));
    }
    if (lane == 0) { sh[0][wv] = lo_y; sh[1][wv] = hi_y; sh[2][wv] = lo_x; sh[3][wv] = hi_x; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < FIN_WAVES; ++w) {
            lo_y = fminf(lo_y, sh[0][w]); hi_y = fmaxf(hi_y, sh[1][w]);
            lo_x = fminf(lo_x, sh[2][w]); hi_x = fmaxf(hi_x, sh[3][w]);
        }
        const bool any = hi_y >= 0.f && hi_x >= 0.f;                      // masks_to_bboxes: an empty mask gives [0, 0, 0, 0]
        float* o = stats + (size_t)blockIdx.x * PT_SEG_STATS_FLOATS;
        o[0] = v[0]; o[1] = ey; o[2] = ex; o[3] = u[0] / v[0]; o[4] = u[1] / v[0];
        o[5] = v[3]; o[6] = eyc; o[7] = exc; o[8] = u[2] / v[3]; o[9] = u[3] / v[3];
        o[10] = v[6];
        o[11] = any ? lo_x : 0.f; o[12] = any ? lo_y : 0.f; o[13] = any ? hi_x : 0.f; o[14] = any ? hi_y : 0.f;
        o[15] = 0.f;
    }
}

// ---- soft aggregation of N objects ------------------------------------------------------------------------------------------------
// grid (ceil(W/64), ceil(H/16)), 256 threads
template <int N>
__global__ __launch_bounds__(ST_THREADS) void k_seg_merge(const float* __restrict__ scores, float* __restrict__ prob,
                                                          unsigned char* __restrict__ labels, float* wsbase, size_t ws_stride, int H, int W,
                                                          int vec) {
    __shared__ float sh[NQ][ST_TH][ST_LD];
    const int t = threadIdx.x, y = blockIdx.y * ST_TH + (t >> 4), x0 = blockIdx.x * ST_TW + (t & 15) * 4;
    const size_t plane = (size_t)H * W, o = (size_t)y * W + x0;
    const bool rowin = y < H && x0 < W;
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = rowin && x0 + k < W;
    float s[N + 1][4], out[N + 1][4] = {};
#pragma unroll
    for (int i = 1; i <= N; ++i) {
        const float* src = scores + (size_t)(i - 1) * plane + o;
        if (rowin && vec) {
            const f32x4 v = *(const f32x4*)src;
            s[i][0] = v[0]; s[i][1] = v[1]; s[i][2] = v[2]; s[i][3] = v[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[i][k] = in[k] ? src[k] : 0.f;
        }
    }
    const float eps = 1e-7f, one_m_eps = (float)(1.0 - 1e-7);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float bg = 1.f;
#pragma unroll
        for (int i = 1; i <= N; ++i) bg *= 1.f - sigmoidf(s[i][k]);
        bg = fminf(fmaxf(bg, eps), one_m_eps);
        s[0][k] = logf(bg / (1.f - bg));
    }
    float best[4] = {-1.f, -1.f, -1.f, -1.f};
    int idx[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int i = 0; i <= N; ++i) {
        float si[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) si[k] = s[0][k];
#pragma unroll
        for (int j = 1; j <= N; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) si[k] = (i == j) ? s[j][k] : si[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j <= N; ++j) sum += expf(s[j][k] - si[k]);
            r[k] = 1.f / sum;
            if (r[k] > best[k]) { best[k] = r[k]; idx[k] = i; }           // the first maximum wins, as numpy.argmax
        }
#pragma unroll
        for (int j = 0; j <= N; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) out[j][k] = (i == j) ? r[k] : out[j][k];
        if (rowin) {
            float* dst = prob + (size_t)i * plane + o;
            if (vec) {
                *(f32x4*)dst = f32x4{r[0], r[1], r[2], r[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (in[k]) dst[k] = r[k];
            }
        }
    }
    if (rowin) {
        if (vec) {
            *(u8x4*)(labels + o) = u8x4{(unsigned char)idx[0], (unsigned char)idx[1], (unsigned char)idx[2], (unsigned char)idx[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k]) labels[o + k] = (unsigned char)idx[k];
        }
    }
#pragma unroll 1
    for (int i = 1; i <= N; ++i) {
        float p[4], m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = out[1][k];
#pragma unroll
        for (int j = 2; j <= N; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = (i == j) ? out[j][k] : p[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p[k] = in[k] ? p[k] : 0.f;
            m[k] = (in[k] && idx[k] == i) ? 1.f : 0.f;
        }
        tile_partials(sh, p, m, stat_ws(wsbase + (size_t)(i - 1) * ws_stride, H, W, gridDim.x, gridDim.y));
    }
}

template <int N>
void launch_merge(dim3 grid, hipStream_t st, const float* scores, float* prob, unsigned char* labels, float* ws, size_t stride, int H, int W,
                  int vec) {
    hipLaunchKernelGGL(k_seg_merge<N>, grid, dim3(ST_THREADS), 0, st, scores, prob, labels, ws, stride, H, W, vec);
}

// ---- mask patch -------------------------------------------------------------------------------------------------------------------
struct MaskPatchArgs {
    const float* im;
    float* out;
    int C, H, W, OH, OW, vec;
    pt_patch_geom g;
};

// a thread = 4 consecutive output pixels of a row; grid-stride over C * OH * ceil(OW/4) quads
__global__ __launch_bounds__(256) void k_mask_patch(MaskPatchArgs a) {
    const pt_patch_geom g = a.g;
    const int QW = (a.OW + 3) / 4;
    const long total = (long)a.C * a.OH * QW;
    // legacy 'nearest' of ATen: scale = (float)in / (float)out, index = min((int)floorf(dst * scale), in - 1), in fp32
    const float sh = (float)g.crop_h / (float)a.OH, sw = (float)g.crop_w / (float)a.OW;
    const int h2 = (a.H - g.os0 + g.df - 1) / g.df, w2 = (a.W - g.os1 + g.df - 1) / g.df;   // the strided view im[os0::df, os1::df]
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int q = (int)(e % QW);
        long r = e / QW;
        const int y = (int)(r % a.OH), c = (int)(r / a.OH);
        const int vy = g.tl0 + min((int)floorf((float)y * sh), g.crop_h - 1);
        const bool yin = vy >= 0 && vy < h2;
        const float* row = a.im + ((size_t)c * a.H + (size_t)(g.os0 + g.df * (yin ? vy : 0))) * a.W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = 4 * q + k;
            const int vx = g.tl1 + min((int)floorf((float)x * sw), g.crop_w - 1);
            v[k] = (x < a.OW && yin && vx >= 0 && vx < w2) ? row[g.os1 + g.df * vx] : 0.f;   // F.pad: zeros outside the view
        }
        float* dst = a.out + ((size_t)c * a.OH + y) * a.OW + 4 * q;
        if (a.vec) {
            *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < a.OW) dst[k] = v[k];
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
inline bool dims_ok(int H, int W) { return H <= PT_SEG_MAX_DIM && W <= PT_SEG_MAX_DIM; }

int launch_finish(float* ws, size_t stride, float* stats, int blocks, int H, int W, hipStream_t st) {
    hipLaunchKernelGGL(k_seg_finish, dim3(blocks), dim3(FIN_THREADS), 0, st, ws, stride, stats, H, W, tiles_x(W), tiles_y(H));
    PT_CHECK_LAUNCH();
    return PT_OK;
}

}  // namespace

size_t pt_seg_stats_ws_bytes_impl(int blocks, int H, int W) {
    if (blocks <= 0 || blocks > PT_SEG_MAX_OBJECTS || H <= 0 || W <= 0 || !dims_ok(H, W)) return 0;
    return (size_t)blocks * stat_ws_floats(H, W) * sizeof(float);
}

int pt_seg_readout_impl(const float* scores, int Hc, int Wc, double scale, int Hr, int Wr, int r1, int c1, int Hi, int Wi, float* scores_im,
                        float* prob_im, float* mask_im, float* stats, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!scores || !stats || !ws) return PT_ERR_NULL;
    if (Hc <= 0 || Wc <= 0 || Hr <= 0 || Wr <= 0 || Hi <= 0 || Wi <= 0 || !(scale > 0.0)) return PT_ERR_SHAPE;
    if (!dims_ok(Hc, Wc) || !dims_ok(Hi, Wi) || !dims_ok(Hr, Wr) || r1 < -PT_SEG_MAX_DIM || r1 > PT_SEG_MAX_DIM || c1 < -PT_SEG_MAX_DIM ||
        c1 > PT_SEG_MAX_DIM)
        return PT_ERR_UNSUPPORTED;
    if (ws_bytes < pt_seg_stats_ws_bytes_impl(1, Hi, Wi) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    ReadoutArgs a;
    a.scores = scores; a.scores_im = scores_im; a.prob_im = prob_im; a.mask_im = mask_im; a.wsbase = (float*)ws;
    a.Hc = Hc; a.Wc = Wc; a.Hr = Hr; a.Wr = Wr; a.r1 = r1; a.c1 = c1; a.Hi = Hi; a.Wi = Wi;
    a.vec = (Wi % 4 == 0 && aligned16(scores_im) && aligned16(prob_im) && aligned16(mask_im)) ? 1 : 0;
    a.rscale = (float)(1.0 / scale);
    hipLaunchKernelGGL(k_seg_readout, dim3(tiles_x(Wi), tiles_y(Hi)), dim3(ST_THREADS), 0, st, a);
    PT_CHECK_LAUNCH();
    return launch_finish((float*)ws, 0, stats, 1, Hi, Wi, st);
}

int pt_seg_state_impl(const float* prob, const float* mask, int H, int W, float* stats, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!prob || !stats || !ws) return PT_ERR_NULL;
    if (H <= 0 || W <= 0) return PT_ERR_SHAPE;
    if (!dims_ok(H, W)) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < pt_seg_stats_ws_bytes_impl(1, H, W) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    const int vec = (W % 4 == 0 && aligned16(prob) && aligned16(mask)) ? 1 : 0;
    hipLaunchKernelGGL(k_seg_state, dim3(tiles_x(W), tiles_y(H)), dim3(ST_THREADS), 0, st, prob, mask, (float*)ws, H, W, vec);
    PT_CHECK_LAUNCH();
    return launch_finish((float*)ws, 0, stats, 1, H, W, st);
}

int pt_seg_merge_impl(const float* scores, int N, int H, int W, float* prob, unsigned char* labels, float* stats, void* ws, size_t ws_bytes,
                      hipStream_t st) {
    if (!scores || !prob || !labels || !stats || !ws) return PT_ERR_NULL;
    if (N <= 0 || H <= 0 || W <= 0) return PT_ERR_SHAPE;
    if (N > PT_SEG_MAX_OBJECTS || !dims_ok(H, W)) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < pt_seg_stats_ws_bytes_impl(N, H, W) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    // W % 4 == 0 keeps every plane and every row 16-byte aligned relative to its base (and the label rows 4-byte aligned)
    const int vec = (W % 4 == 0 && aligned16(scores) && aligned16(prob) && ((uintptr_t)labels % 4) == 0) ? 1 : 0;
    const dim3 grid(tiles_x(W), tiles_y(H));
    const size_t stride = stat_ws_floats(H, W);
    float* w = (float*)ws;
    switch (N) {
#define PT_SEG_MERGE_CASE(n) case n: launch_merge<n>(grid, st, scores, prob, labels, w, stride, H, W, vec); break;
        PT_SEG_MERGE_CASE(1) PT_SEG_MERGE_CASE(2) PT_SEG_MERGE_CASE(3) PT_SEG_MERGE_CASE(4) PT_SEG_MERGE_CASE(5) PT_SEG_MERGE_CASE(6)
        PT_SEG_MERGE_CASE(7) PT_SEG_MERGE_CASE(8) PT_SEG_MERGE_CASE(9) PT_SEG_MERGE_CASE(10) PT_SEG_MERGE_CASE(11) PT_SEG_MERGE_CASE(12)
        PT_SEG_MERGE_CASE(13) PT_SEG_MERGE_CASE(14) PT_SEG_MERGE_CASE(15) PT_SEG_MERGE_CASE(16)
#undef PT_SEG_MERGE_CASE
    }
    PT_CHECK_LAUNCH();
    return launch_finish(w, stride, stats, N, H, W, st);
}

int pt_sample_mask_patch_impl(const float* im, int C, int H, int W, const pt_patch_geom* geom, float* out, int OH, int OW, hipStream_t st) {
    if (!im || !geom || !out) return PT_ERR_NULL;
    if (C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return PT_ERR_SHAPE;
    const pt_patch_geom& g = *geom;
    if (g.df < 1 || g.crop_h < 1 || g.crop_w < 1 || g.os0 < 0 || g.os1 < 0 || g.os0 >= g.df || g.os1 >= g.df || g.os0 >= H || g.os1 >= W)
        return PT_ERR_SHAPE;
    if (!dims_ok(H, W) || !dims_ok(OH, OW) || !dims_ok(g.crop_h, g.crop_w) || C > 1024) return PT_ERR_UNSUPPORTED;
    MaskPatchArgs a;
    a.im = im; a.out = out; a.C = C; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.g = g;
    a.vec = (OW % 4 == 0 && aligned16(out)) ? 1 : 0;
    const long total = (long)C * OH * ((OW + 3) / 4);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_mask_patch, dim3(blocks), dim3(256), 0, st, a);
    PT_CHECK_LAUNCH();
    return PT_OK;
}
