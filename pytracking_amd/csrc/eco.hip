// ECO's Fourier-domain per-frame path (pytracking/tracker/eco/eco.py:181-245, 293-309, 339-343; pytracking/libs/fourier.py; dcf.py:97-103):
//
//   pt_eco_sample_f32        project_sample + window + real 2-D DFT + rfftshift2 + interpolate_dft (+ shift_fs)     k_eco_sample
//   pt_eco_shift_f32         fourier.shift_fs of a half spectrum                                                       k_eco_shift
//   pt_eco_apply_filter_f32  sum_c hf * xf per frequency bin                                                           k_eco_apply_filter
//   pt_eco_localize_f32      sum_fs + sample_fs on an (Oh, Ow) grid + dcf.max2d                                        k_eco_twiddles, k_eco_series_rows,
//                                                                                                                      k_eco_series_cols, k_max2d (localize.hip)
//   pt_eco_insert_f32        shift_fs + the transposed store into slot `ind` of the sample memory                     k_eco_insert
//   pt_eco_filter_update_f32 FilterOptim.run, all blocks (second half of this file)                                    k_eco_fu_*
//
// Complex numbers are a trailing dimension of 2 (the reference's layout), loaded and stored as float2.  The transforms are dense: the
// maps are at most 64 x 64 and the score grid a few hundred points wide, so a pass is a sum of <= 64 twiddle products per output.  Twiddle
// phases are reduced in integers ((k n) mod N, carried incrementally) and looked up in tables of cos / sin(2 pi j / N) that are evaluated
// in double precision, so the accuracy of a term does not depend on k n.  Inputs, outputs and everything in memory are fp32; the sums
// themselves (<= 256 channels, <= 64 samples of a row or column, <= 129 rows of a series) run in double-precision registers and are
// rounded to fp32 once: a sequential fp32 sum of 60 terms would sit at the float64 bound the tests hold these outputs to (4 x the error
// of an fp32 FFT), and the fp64 FMA costs nothing at these sizes.  Every sum runs in one fixed order inside one thread: no atomics,
// repeated calls give the same bits.
#include <math.h>
#include "common.h"
#include "pt_internal.h"

namespace {

constexpr int EC_THREADS = 256;
constexpr int EC_F = PT_ECO_MAX_FEAT, EC_WH = PT_ECO_MAX_FEAT / 2 + 1;

__device__ inline float2 cmul(float2 a, float2 b) {          // complex.mult: (ar br - ai bi, ar bi + ai br)
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ inline double2 unit(int j, int N) {                // (cos, sin)(2 pi j / N), 0 <= j < N
    double s, c;
    sincospi(2.0 * (double)j / (double)N, &s, &c);
    return make_double2(c, s);
}
__device__ inline float2 expi(float ang) {                    // complex.exp_imag
    float s, c;
    sincosf(ang, &s, &c);
    return make_float2(c, s);
}

// ---- sample transform ----------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    const float *x, *P, *win;
    const float2 *iy, *ix;
    float2* out;
    int Cin, c, H, W, Hf, Wh, has_shift;
    float s0, s1;
};

// grid (c, S), 256 threads: one workgroup = one projected channel of one sample, the whole map in LDS
__global__ __launch_bounds__(EC_THREADS) void k_eco_sample(SampleArgs a) {
    __shared__ float y[EC_F * EC_F];
    __shared__ double2 T[EC_F * EC_WH];
    __shared__ double2 twW[EC_F], twH[EC_F];
    const int k = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    const int H = a.H, W = a.W, HW = H * W, Hf = a.Hf, Wh = a.Wh;
    if (t < W) twW[t] = unit(t, W);
    if (t >= 64 && t - 64 < H) twH[t - 64] = unit(t - 64, H);
    const float* xs = a.x + (size_t)s * a.Cin * HW;
    for (int p = t; p < HW; p += EC_THREADS) {
        float v;
        if (a.P) {
            double acc = 0.0;
            for (int ci = 0; ci < a.Cin; ++ci) acc = fma((double)xs[(size_t)ci * HW + p], (double)a.P[(size_t)ci * a.c + k], acc);
            v = (float)acc;
        } else {
            v = xs[(size_t)k * HW + p];
        }
        y[p] = a.win ? v * a.win[p] : v;
    }
    __syncthreads();
    for (int q = t; q < H * Wh; q += EC_THREADS) {             // rows: T[h][kx] = sum_w y[h][w] e^{-2 pi i kx w / W}
        const int h = q / Wh, kx = q - h * Wh;
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int w = 0; w < W; ++w) {
            const double2 tw = twW[idx];
            const double v = (double)y[h * W + w];
            re = fma(v, tw.x, re);
            im = fma(-v, tw.y, im);
            idx += kx;
            if (idx >= W) idx -= W;
        }
        T[q] = make_double2(re, im);
    }
    __syncthreads();
    const int mid = (Hf - 1) / 2;
    float2* o = a.out + ((size_t)s * a.c + k) * Hf * Wh;
    for (int q = t; q < Hf * Wh; q += EC_THREADS) {            // columns, centred: row r carries frequency r - mid (Nyquist at both ends)
        const int r = q / Wh, kx = q - r * Wh, f = r - mid;
        const int fm = ((f % H) + H) % H;
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int h = 0; h < H; ++h) {
            const double2 tw = twH[idx], v = T[h * Wh + kx];
            re = fma(v.x, tw.x, fma(v.y, tw.y, re));
            im = fma(v.y, tw.x, fma(-v.x, tw.y, im));
            idx += fm;
            if (idx >= H) idx -= H;
        }
        float2 v = make_float2((float)re, (float)im);
        if (a.iy) v = cmul(cmul(v, a.iy[r]), a.ix[kx]);
        if (a.has_shift) v = cmul(cmul(v, expi(a.s0 * (float)f)), expi(a.s1 * (float)kx));
        o[q] = v;
    }
}

// ---- shift_fs ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EC_THREADS) void k_eco_shift(const float2* in, float2* out, long total, int Hf, int Wh, float s0, float s1) {
    const long i = (long)blockIdx.x * EC_THREADS + threadIdx.x;
    if (i >= total) return;
    const int kx = (int)(i % Wh), r = (int)((i / Wh) % Hf);
    out[i] = cmul(cmul(in[i], expi(s0 * (float)(r - (Hf - 1) / 2))), expi(s1 * (float)kx));
}

// ---- filter response -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EC_THREADS) void k_eco_apply_filter(const float2* hf, const float2* xf, float2* sf, int S, int c, int bins) {
    const long i = (long)blockIdx.x * EC_THREADS + threadIdx.x;
    if (i >= (long)S * bins) return;
    const int s = (int)(i / bins), b = (int)(i - (long)s * bins);
    const float2* xs = xf + (size_t)s * c * bins + b;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < c; ++k) {
        const float2 h = hf[(size_t)k * bins + b], x = xs[(size_t)k * bins];
        re = fma((double)h.x, (double)x.x, fma(-(double)h.y, (double)x.y, re));
        im = fma((double)h.x, (double)x.y, fma((double)h.y, (double)x.x, im));
    }
    sf[i] = make_float2((float)re, (float)im);
}

// ---- memory insert -------------------------------------------------------------------------------------------------------------------
// thread = (bin, channel), channel fastest: the store into samples (Hf, Wh, n, c, 2) is contiguous per bin
__global__ __launch_bounds__(EC_THREADS) void k_eco_insert(const float2* xf, float2* samples, int c, int Hf, int Wh, int n, int ind, int has_shift,
                                                           float s0, float s1) {
    const long i = (long)blockIdx.x * EC_THREADS + threadIdx.x, bins = (long)Hf * Wh;
    if (i >= bins * c) return;
    const int k = (int)(i % c);
    const long b = i / c;
    float2 v = xf[(size_t)k * bins + b];
    if (has_shift) {
        const int kx = (int)(b % Wh), r = (int)(b / Wh);
        v = cmul(cmul(v, expi(s0 * (float)(r - (Hf - 1) / 2))), expi(s1 * (float)kx));
    }
    samples[((size_t)b * n + ind) * c + k] = v;
}

// ---- localisation --------------------------------------------------------------------------------------------------------------------
struct SeriesArgs {
    const float2* sf[PT_ECO_MAX_BLOCKS];
    int Hf[PT_ECO_MAX_BLOCKS], Wh[PT_ECO_MAX_BLOCKS], top[PT_ECO_MAX_BLOCKS];
    float w[PT_ECO_MAX_BLOCKS];
    int nb, S, Oh, Ow;
    const double2 *twH, *twW;
    float2* G;
    float* scores;
};

__global__ __launch_bounds__(EC_THREADS) void k_eco_twiddles(double2* twH, double2* twW, int Oh, int Ow) {
    const int i = blockIdx.x * EC_THREADS + threadIdx.x;
    if (i < Oh) twH[i] = unit(i, Oh);
    else if (i - Oh < Ow) twW[i - Oh] = unit(i - Oh, Ow);
}

// G[s][y][kx] = sum_r A[s][r][kx] e^{+2 pi i (r - mid) y / Oh}, A = the blocks added at sum_fs's offsets.  grid (ceil(Oh / 4), S); a wave per
// row y, a lane per column kx (Wh <= 64)
__global__ __launch_bounds__(EC_THREADS) void k_eco_series_rows(SeriesArgs a) {
    const int kx = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), s = blockIdx.y;
    const int Hf = a.Hf[0], Wh = a.Wh[0], Oh = a.Oh, mid = (Hf - 1) / 2;
    if (y >= Oh || kx >= Wh) return;
    int idx = (int)((((long)-mid * y) % Oh + Oh) % Oh);
    double re = 0.0, im = 0.0;
    for (int r = 0; r < Hf; ++r) {
        float2 v = a.sf[0][((size_t)s * Hf + r) * Wh + kx];
        v.x *= a.w[0];
        v.y *= a.w[0];
        for (int b = 1; b < a.nb; ++b) {
            const int rb = r - a.top[b];
            if (rb >= 0 && rb < a.Hf[b] && kx < a.Wh[b]) {
                const float2 e = a.sf[b][((size_t)s * a.Hf[b] + rb) * a.Wh[b] + kx];
                v.x += a.w[b] * e.x;
                v.y += a.w[b] * e.y;
            }
        }
        const double2 tw = a.twH[idx];
        re = fma((double)v.x, tw.x, fma(-(double)v.y, tw.y, re));
        im = fma((double)v.x, tw.y, fma((double)v.y, tw.x, im));
        idx += y;
        if (idx >= Oh) idx -= Oh;
    }
    a.G[((size_t)s * Oh + y) * Wh + kx] = make_float2((float)re, (float)im);
}

// scores[s][y][x] = Re sum_kx m_kx G[s][y][kx] e^{+2 pi i kx x / Ow}, m_0 = 1, m_kx = 2.  grid (ceil(Ow / 256), ceil(Oh / 8), S); a thread
// = one column x of 8 rows, which share the twiddle
constexpr int SR = 8;
__global__ __launch_bounds__(EC_THREADS) void k_eco_series_cols(SeriesArgs a) {
    __shared__ float2 g[SR][64];
    const int t = threadIdx.x, x = blockIdx.x * EC_THREADS + t, y0 = blockIdx.y * SR, s = blockIdx.z;
    const int Wh = a.Wh[0], Oh = a.Oh, Ow = a.Ow;
    for (int q = t; q < SR * Wh; q += EC_THREADS) {
        const int j = q / Wh, kx = q - j * Wh;
        g[j][kx] = y0 + j < Oh ? a.G[((size_t)s * Oh + y0 + j) * Wh + kx] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    if (x >= Ow) return;
    double acc[SR];
#pragma unroll
    for (int j = 0; j < SR; ++j) acc[j] = (double)g[j][0].x;
    int idx = 0;
    for (int kx = 1; kx < Wh; ++kx) {
        idx += x;
        if (idx >= Ow) idx -= Ow;
        const double2 tw = a.twW[idx];
        const double c2 = 2.0 * tw.x, s2 = 2.0 * tw.y;
#pragma unroll
        for (int j = 0; j < SR; ++j) acc[j] = fma((double)g[j][kx].x, c2, fma(-(double)g[j][kx].y, s2, acc[j]));
    }
#pragma unroll
    for (int j = 0; j < SR; ++j)
        if (y0 + j < Oh) a.scores[((size_t)s * Oh + y0 + j) * Ow + x] = (float)acc[j];
}

inline size_t loc_tw_floats(int Oh, int Ow) { return pt_align_floats((size_t)4 * (Oh + Ow)); }          // two tables of double2

}  // namespace

extern "C" int pt_eco_sample_f32(const float* x, const float* proj, const float* window, const float* interp_y, const float* interp_x,
                                 int has_shift, float shift_y, float shift_x, float* xf, int S, int Cin, int c, int H, int W, void* stream) {
    if (!x || !xf || (!interp_y) != (!interp_x)) return PT_ERR_NULL;
    if (S <= 0 || Cin <= 0 || c <= 0 || H <= 0 || W <= 0 || (!proj && c != Cin)) return PT_ERR_SHAPE;
    if (H > PT_ECO_MAX_FEAT || W > PT_ECO_MAX_FEAT || c > 65535 || S > 65535) return PT_ERR_UNSUPPORTED;
    SampleArgs a{x, proj, window, (const float2*)interp_y, (const float2*)interp_x, (float2*)xf, Cin, c, H, W, H + (H + 1) % 2, W / 2 + 1,
                 has_shift ? 1 : 0, shift_y, shift_x};
    hipLaunchKernelGGL(k_eco_sample, dim3(c, S), dim3(EC_THREADS), 0, (hipStream_t)stream, a);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" int pt_eco_shift_f32(const float* xf, float shift_y, float shift_x, float* out, int S, int c, int Hf, int Wh, void* stream) {
    if (!xf || !out) return PT_ERR_NULL;
    if (S <= 0 || c <= 0 || Hf <= 0 || Wh <= 0 || Hf % 2 == 0) return PT_ERR_SHAPE;
    const long total = (long)S * c * Hf * Wh;
    if (total > (1L << 30)) return PT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_eco_shift, dim3((unsigned)((total + EC_THREADS - 1) / EC_THREADS)), dim3(EC_THREADS), 0, (hipStream_t)stream,
                       (const float2*)xf, (float2*)out, total, Hf, Wh, shift_y, shift_x);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" int pt_eco_apply_filter_f32(const float* hf, const float* xf, float* sf, int S, int c, int Hf, int Wh, void* stream) {
    if (!hf || !xf || !sf) return PT_ERR_NULL;
    if (S <= 0 || c <= 0 || Hf <= 0 || Wh <= 0) return PT_ERR_SHAPE;
    const long bins = (long)Hf * Wh;
    if (bins > (1 << 24) || (long)S * c * bins > (1L << 30)) return PT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_eco_apply_filter, dim3((unsigned)((S * bins + EC_THREADS - 1) / EC_THREADS)), dim3(EC_THREADS), 0, (hipStream_t)stream,
                       (const float2*)hf, (const float2*)xf, (float2*)sf, S, c, (int)bins);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" int pt_eco_insert_f32(const float* xf, int has_shift, float shift_y, float shift_x, float* samples, int c, int Hf, int Wh, int n,
                                 int ind, void* stream) {
    if (!xf || !samples) return PT_ERR_NULL;
    if (c <= 0 || Hf <= 0 || Wh <= 0 || n <= 0 || ind < 0 || ind >= n || Hf % 2 == 0) return PT_ERR_SHAPE;
    const long total = (long)Hf * Wh * c;
    if (total * n > (1L << 30)) return PT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_eco_insert, dim3((unsigned)((total + EC_THREADS - 1) / EC_THREADS)), dim3(EC_THREADS), 0, (hipStream_t)stream,
                       (const float2*)xf, (float2*)samples, c, Hf, Wh, n, ind, has_shift ? 1 : 0, shift_y, shift_x);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

static bool eco_loc_covered(int S, int Wh, int Oh, int Ow) {
    return S > 0 && S <= 65535 && Wh > 0 && Wh <= 64 && Oh > 0 && Ow > 0 && Oh <= PT_ECO_MAX_GRID && Ow <= PT_ECO_MAX_GRID;
}

extern "C" size_t pt_eco_localize_ws_bytes(int S, int Wh, int Oh, int Ow) {
    if (!eco_loc_covered(S, Wh, Oh, Ow)) return 0;
    return (loc_tw_floats(Oh, Ow) + pt_align_floats((size_t)2 * S * Oh * Wh)) * sizeof(float);
}

extern "C" int pt_eco_localize_f32(const float* const* sf, const int* Hf, const int* Wh, const float* weight, int nb, int S, int Oh, int Ow,
                                   float* scores, float* max_val, long long* argmax, void* ws, size_t ws_bytes, void* stream) {
    if (!sf || !Hf || !Wh || !scores || !max_val || !argmax || !ws) return PT_ERR_NULL;
    if (nb <= 0 || S <= 0 || Oh <= 0 || Ow <= 0) return PT_ERR_SHAPE;
    if (nb > PT_ECO_MAX_BLOCKS) return PT_ERR_UNSUPPORTED;
    SeriesArgs a{};
    for (int b = 0; b < nb; ++b) {
        if (!sf[b]) return PT_ERR_NULL;
        if (Hf[b] <= 0 || Wh[b] <= 0 || Hf[b] % 2 == 0 || Hf[b] > Hf[0] || Wh[b] > Wh[0]) return PT_ERR_SHAPE;
        a.sf[b] = (const float2*)sf[b];
        a.Hf[b] = Hf[b];
        a.Wh[b] = Wh[b];
        a.top[b] = (Hf[0] - 1) / 2 - (Hf[b] - 1) / 2;
        a.w[b] = weight ? weight[b] : 1.f;
    }
    if (Oh < Hf[0] || Ow < 2 * Wh[0] - 1) return PT_ERR_SHAPE;
    if (!eco_loc_covered(S, Wh[0], Oh, Ow)) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < pt_eco_localize_ws_bytes(S, Wh[0], Oh, Ow) || ((uintptr_t)ws & 255)) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    a.nb = nb; a.S = S; a.Oh = Oh; a.Ow = Ow;
    a.twH = (const double2*)base;
    a.twW = a.twH + Oh;
    a.G = (float2*)(base + loc_tw_floats(Oh, Ow));
    a.scores = scores;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_eco_twiddles, dim3((Oh + Ow + EC_THREADS - 1) / EC_THREADS), dim3(EC_THREADS), 0, st, (double2*)base, (double2*)base + Oh, Oh, Ow);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eco_series_rows, dim3((Oh + 3) / 4, S), dim3(EC_THREADS), 0, st, a);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eco_series_cols, dim3((Ow + EC_THREADS - 1) / EC_THREADS, (Oh + SR - 1) / SR, S), dim3(EC_THREADS), 0, st, a);
    PT_CHECK_LAUNCH();
    return pt_max2d_f32(scores, max_val, argmax, S, Oh, Ow, stream);
}

// ======================================================================================================================================
// Filter update: FilterOptim.run (pytracking/tracker/eco/optim.py:142-208) on ConjugateGradientBase.run_CG (libs/optimization.py:72-163).
//
//   k_eco_fu_setup   per bin: sample-energy moving average, b = yf conj(sum_n w_n S_n), diag_M; the forget factor on the carried rho   1 launch
//   k_eco_fu_data    per bin: (the direction update p = z + beta p of this bin, then) q = S^H diag(w) S v for v = x or p               1 per A
//   k_eco_fu_reg     per coefficient: q += the regulariser (two convolutions with the real reg filter over the conjugate-extended v)    1 per A
//   k_eco_fu_rho     per block: (r = b - q,) z = r / diag_M, rho = ip(r, z), the Polak-Ribiere term, beta, the joint rho == 0 flag     1 per iteration
//   k_eco_fu_step    per block: ip(p, q), ip(p, r), alpha, r_prev = r, x += alpha p, r -= alpha q                                        1 per iteration
//
// A bin's n c samples are contiguous; a workgroup takes one bin, forms S v per sample (thread = sample) into LDS and then S^H of it per
// channel (thread = channel): the samples are read once from HBM and once more from cache per application of A.  All feature blocks ride
// in every launch (grid.y); the CG scalars are per block and live in the caller's state (rho, whether p is valid) and in the workspace.
// The early exit is joint: any block whose rho is exactly 0 raises the flags of all later steps in the workspace and every later launch of the call
// returns at once, so x stays as it is; nothing is read back.  Sums over samples, channels and coefficients run in double registers in one fixed order.
namespace {

struct FuBlock {
    const float2* S; const float *w, *yf, *reg;
    float* se; const float2* new_xf;
    float2 *x, *p, *rprev; float* scal;                     // caller state: scal[0] = rho, scal[1] = p valid
    float2 *b, *r, *z, *q; float *dM, *tmp;                 // workspace; tmp[0] = beta, tmp[1] = p was valid
    int Hf, Wh, c, n, Rh, Rw, pad1, pad2, remove;
    float lr, one_minus_lr, reg_energy;
};
struct FuArgs {
    FuBlock blk[PT_ECO_MAX_BLOCKS];
    int* flag;
    float dp, rp, forget;
    int fr, std_alpha, reset;
};

__device__ inline double fu_block_sum(double v, double* sh) {              // 1024 threads, fixed order; every thread gets the result
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    if ((t & 63) == 0) {
        double s = 0.0;
        for (int j = 0; j < 64; ++j) s += sh[t + j];
        sh[t] = s;
    }
    __syncthreads();
    double tot = 0.0;
    for (int wv = 0; wv < 16; ++wv) tot += sh[wv * 64];
    return tot;
}

// grid (max bins, blocks), 64 threads
__global__ __launch_bounds__(64) void k_eco_fu_setup(FuArgs a) {
    __shared__ float se_s[64];
    const FuBlock& B = a.blk[blockIdx.y];
    const int bins = B.Hf * B.Wh, bin = blockIdx.x, k = threadIdx.x;
    if (bin == 0 && blockIdx.y == 0) a.flag[k] = 0;
    if (bin == 0 && k == 0) {
        if (a.reset) { B.scal[0] = 1.f; B.scal[1] = 0.f; }
        else if (B.scal[1] != 0.f) B.scal[0] = B.scal[0] / a.forget;
    }
    if (bin >= bins) return;
    float se = 0.f;
    if (k < B.c) {
        se = B.se[(size_t)k * bins + bin];
        if (B.new_xf) {
            const float2 v = B.new_xf[(size_t)k * bins + bin];
            se = B.one_minus_lr * se + B.lr * (v.x * v.x + v.y * v.y);
            B.se[(size_t)k * bins + bin] = se;
        }
        se_s[k] = se;
    }
    __syncthreads();
    if (k >= B.c) return;
    double m = 0.0;
    for (int j = 0; j < B.c; ++j) m += (double)se_s[j];
    const float mean = (float)(m / B.c);
    B.dM[(size_t)k * bins + bin] = (1.f - a.rp) * (a.dp * se + (1.f - a.dp) * mean) + a.rp * B.reg_energy;
    double re = 0.0, im = 0.0;
    const float2* s = B.S + (size_t)bin * B.n * B.c + k;
    for (int i = 0; i < B.n; ++i) {
        const float2 v = s[(size_t)i * B.c];
        const double w = (double)B.w[i];
        re = fma(w, (double)v.x, re);
        im = fma(w, (double)v.y, im);
    }
    const float y = B.yf[bin];
    B.b[(size_t)k * bins + bin] = make_float2(y * (float)re, -(y * (float)im));
}

// grid (max bins, blocks), 256 threads; from_p: v = p after p = z + beta p, else v = x
__global__ __launch_bounds__(256) void k_eco_fu_data(FuArgs a, int from_p, int it) {
    __shared__ float2 v_s[64];
    __shared__ double2 sh_s[PT_ECO_MAX_SAMPLES];
    if (from_p && a.flag[it + 1]) return;
    const FuBlock& B = a.blk[blockIdx.y];
    const int bins = B.Hf * B.Wh, bin = blockIdx.x, t = threadIdx.x;
    if (bin >= bins) return;
    if (t < B.c) {
        const size_t e = (size_t)t * bins + bin;
        float2 v;
        if (from_p) {
            v = B.z[e];
            if (B.tmp[1] != 0.f) {
                const float beta = B.tmp[0];
                const float2 p = B.p[e];
                v = make_float2(v.x + p.x * beta, v.y + p.y * beta);
            }
            B.p[e] = v;
        } else {
            v = B.x[e];
        }
        v_s[t] = v;
    }
    __syncthreads();
    const float2* s = B.S + (size_t)bin * B.n * B.c;
    for (int i = t; i < B.n; i += 256) {
        double re = 0.0, im = 0.0;
        for (int k = 0; k < B.c; ++k) {
            const float2 x = s[(size_t)i * B.c + k], v = v_s[k];
            re = fma((double)x.x, (double)v.x, fma(-(double)x.y, (double)v.y, re));
            im = fma((double)x.x, (double)v.y, fma((double)x.y, (double)v.x, im));
        }
        const double w = (double)B.w[i];
        sh_s[i] = make_double2((double)(float)(w * (float)re), (double)(float)(w * (float)im));
    }
    __syncthreads();
    if (t >= B.c) return;
    double re = 0.0, im = 0.0;
    for (int i = 0; i < B.n; ++i) {                                   // sh conj(S): (a + ib)(c - id) = ac + bd + i(bc - ad)
        const double2 h = sh_s[i];
        const float2 x = s[(size_t)i * B.c + t];
        re = fma(h.x, (double)x.x, fma(h.y, (double)x.y, re));
        im = fma(h.y, (double)x.x, fma(-h.x, (double)x.y, im));
    }
    B.q[(size_t)t * bins + bin] = make_float2((float)re, (float)im);
}

// v extended to the left by padl = min(pad2, Wh - 1) columns: column x >= 0 is v[r][x], column x < 0 is conj(v[Hf - 1 - r][-x]); zero outside
__device__ inline float2 fu_ext(const float2* v, int r, int x, int Hf, int Wh, int padl) {
    if (r < 0 || r >= Hf || x >= Wh || x < -padl) return make_float2(0.f, 0.f);
    if (x >= 0) return v[r * Wh + x];
    const float2 e = v[(Hf - 1 - r) * Wh - x];
    return make_float2(e.x, -e.y);
}

// grid (ceil(max c bins / 256), blocks), 256 threads
__global__ __launch_bounds__(256) void k_eco_fu_reg(FuArgs a, int from_p, int it) {
    if (from_p && a.flag[it + 1]) return;
    const FuBlock& B = a.blk[blockIdx.y];
    const int bins = B.Hf * B.Wh;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B.c * bins) return;
    const int k = (int)(e / bins), bin = (int)(e - (long)k * bins), i = bin / B.Wh, j = bin - i * B.Wh;
    const float2* v = (from_p ? B.p : B.x) + (size_t)k * bins;
    const int h1 = B.Hf + 2 * B.pad1 - B.Rh + 1, w1 = B.Wh + B.remove + 2 * B.pad2 - B.Rw + 1;      // extent of the first convolution
    double re = 0.0, im = 0.0;
    for (int a2 = 0; a2 < B.Rh; ++a2)
        for (int b2 = 0; b2 < B.Rw; ++b2) {
            const int u = i + a2, c1 = j + B.remove + b2;
            if (u >= h1 || c1 >= w1) continue;
            double r1 = 0.0, i1 = 0.0;
            for (int a1 = 0; a1 < B.Rh; ++a1)
                for (int b1 = 0; b1 < B.Rw; ++b1) {
                    const float2 x = fu_ext(v, u + a1 - B.pad1, c1 + b1 - B.pad2 - B.remove, B.Hf, B.Wh, B.remove);
                    const double g = (double)B.reg[a1 * B.Rw + b1];
                    r1 = fma(g, (double)x.x, r1);
                    i1 = fma(g, (double)x.y, i1);
                }
            const double g = (double)B.reg[a2 * B.Rw + b2];
            re = fma(g, (double)(float)r1, re);
            im = fma(g, (double)(float)i1, im);
        }
    float2 q = B.q[e];
    B.q[e] = make_float2(q.x + (float)re, q.y + (float)im);
}

// inner_prod_fs weight of a coefficient: 2 <a, b> - <a[.., 0, :], b[.., 0, :]>
__device__ inline double fu_wt(long e, int Wh) { return (e % Wh) == 0 ? 1.0 : 2.0; }

// grid (blocks), 1024 threads
__global__ __launch_bounds__(1024) void k_eco_fu_rho(FuArgs a, int it) {
    const int first = it == 0;
    __shared__ double sh[1024];
    if (a.flag[it]) return;              // raised by an EARLIER iteration: the blocks of one launch never see each other's flag
    const FuBlock& B = a.blk[blockIdx.x];
    const long N = (long)B.c * B.Hf * B.Wh;
    const bool pr = !a.fr && B.scal[1] != 0.f;
    double rz = 0.0, pz = 0.0;
    for (long e = threadIdx.x; e < N; e += 1024) {
        float2 r;
        if (first) {
            const float2 b = B.b[e], q = B.q[e];
            r = make_float2(b.x - q.x, b.y - q.y);
            B.r[e] = r;
        } else {
            r = B.r[e];
        }
        const float d = B.dM[e];
        const float2 z = make_float2(r.x / d, r.y / d);
        B.z[e] = z;
        const double w = fu_wt(e, B.Wh);
        rz += w * ((double)r.x * z.x + (double)r.y * z.y);
        if (pr) {
            const float2 o = B.rprev[e];
            pz += w * ((double)o.x * z.x + (double)o.y * z.y);
        }
    }
    rz = fu_block_sum(rz, sh);
    pz = fu_block_sum(pz, sh);
    if (threadIdx.x == 0) {
        const float rho1 = B.scal[0], rho = (float)rz;
        B.scal[0] = rho;
        if (rho == 0.f)
            for (int j = it + 1; j < 64; ++j) a.flag[j] = 1;
        float beta = a.fr ? rho / rho1 : (rho - (float)pz) / rho1;
        B.tmp[0] = beta > 0.f ? beta : 0.f;
        B.tmp[1] = B.scal[1];
    }
}

// grid (blocks), 1024 threads
__global__ __launch_bounds__(1024) void k_eco_fu_step(FuArgs a, int last, int it) {
    __shared__ double sh[1024];
    if (a.flag[it + 1]) return;
    const FuBlock& B = a.blk[blockIdx.x];
    const long N = (long)B.c * B.Hf * B.Wh;
    double pq = 0.0, pr = 0.0;
    for (long e = threadIdx.x; e < N; e += 1024) {
        const float2 p = B.p[e], q = B.q[e], r = B.r[e];
        const double w = fu_wt(e, B.Wh);
        pq += w * ((double)p.x * q.x + (double)p.y * q.y);
        pr += w * ((double)p.x * r.x + (double)p.y * r.y);
    }
    pq = fu_block_sum(pq, sh);
    pr = fu_block_sum(pr, sh);
    const float alpha = (a.std_alpha ? B.scal[0] : (float)pr) / (float)pq;
    __syncthreads();
    for (long e = threadIdx.x; e < N; e += 1024) {
        const float2 p = B.p[e], r = B.r[e];
        if (!a.fr) B.rprev[e] = r;
        float2 x = B.x[e];
        B.x[e] = make_float2(x.x + p.x * alpha, x.y + p.y * alpha);
        if (!last) {
            const float2 q = B.q[e];
            B.r[e] = make_float2(r.x - q.x * alpha, r.y - q.y * alpha);
        }
    }
    if (threadIdx.x == 0) B.scal[1] = 1.f;
}

inline size_t fu_block_floats(int Hf, int Wh, int c) {
    const size_t N = (size_t)c * Hf * Wh;
    return 4 * pt_align_floats(2 * N) + pt_align_floats(N) + 64;
}

}  // namespace

extern "C" size_t pt_eco_filter_update_ws_bytes(const pt_eco_fu_block* blk, int nb) {
    if (!blk || nb <= 0 || nb > PT_ECO_MAX_BLOCKS) return 0;
    size_t fl = 64;
    for (int b = 0; b < nb; ++b) {
        if (blk[b].Hf <= 0 || blk[b].Wh <= 0 || blk[b].c <= 0 || blk[b].c > 64 || blk[b].n <= 0 || blk[b].n > PT_ECO_MAX_SAMPLES) return 0;
        fl += fu_block_floats(blk[b].Hf, blk[b].Wh, blk[b].c);
    }
    return fl * sizeof(float);
}

extern "C" int pt_eco_filter_update_f32(const pt_eco_fu_block* blk, int nb, int num_iter, int fletcher_reeves, int standard_alpha,
                                        float direction_forget_factor, float precond_data_param, float precond_reg_param, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (!blk || !ws) return PT_ERR_NULL;
    if (nb <= 0 || num_iter < 0) return PT_ERR_SHAPE;
    if (num_iter > 62) return PT_ERR_UNSUPPORTED;
    if (nb > PT_ECO_MAX_BLOCKS) return PT_ERR_UNSUPPORTED;
    FuArgs a{};
    int maxbins = 0;
    long maxel = 0;
    for (int b = 0; b < nb; ++b) {
        const pt_eco_fu_block& s = blk[b];
        if (!s.samples || !s.weights || !s.yf || !s.reg_filter || !s.sample_energy || !s.x || !s.p || !s.r_prev || !s.state) return PT_ERR_NULL;
        if (s.Hf <= 0 || s.Wh <= 0 || s.c <= 0 || s.n <= 0 || s.Rh <= 0 || s.Rw <= 0 || s.Hf % 2 == 0) return PT_ERR_SHAPE;
        if (s.c > 64 || s.n > PT_ECO_MAX_SAMPLES || s.Rh > 15 || s.Rw > 15 || (long)s.Hf * s.Wh > (1 << 20)) return PT_ERR_UNSUPPORTED;
        FuBlock& B = a.blk[b];
        B.pad1 = s.Rh - 1 < s.Hf - 1 ? s.Rh - 1 : s.Hf - 1;
        B.pad2 = s.Rw - 1 < 2 * s.Wh - 2 ? s.Rw - 1 : 2 * s.Wh - 2;
        B.remove = B.pad2 < s.Wh - 1 ? B.pad2 : s.Wh - 1;
        // the two convolutions must give the filter's own size back (the reference's conv2d raises otherwise)
        if (s.Hf + 2 * B.pad1 - 2 * s.Rh + 2 != s.Hf || s.Wh + 2 * B.pad2 - 2 * s.Rw + 2 != s.Wh) return PT_ERR_UNSUPPORTED;
        B.S = (const float2*)s.samples; B.w = s.weights; B.yf = s.yf; B.reg = s.reg_filter; B.se = s.sample_energy;
        B.new_xf = (const float2*)s.new_xf; B.x = (float2*)s.x; B.p = (float2*)s.p; B.rprev = (float2*)s.r_prev; B.scal = s.state;
        B.Hf = s.Hf; B.Wh = s.Wh; B.c = s.c; B.n = s.n; B.Rh = s.Rh; B.Rw = s.Rw;
        B.lr = s.learning_rate; B.one_minus_lr = (float)(1.0 - (double)s.learning_rate); B.reg_energy = s.reg_energy;
        if (s.Hf * s.Wh > maxbins) maxbins = s.Hf * s.Wh;
        if ((long)s.c * s.Hf * s.Wh > maxel) maxel = (long)s.c * s.Hf * s.Wh;
    }
    if (num_iter == 0) return PT_OK;                                   // the reference returns before the sample-energy update
    if (ws_bytes < pt_eco_filter_update_ws_bytes(blk, nb) || ((uintptr_t)ws & 255)) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    a.flag = (int*)base;
    base += 64;
    for (int b = 0; b < nb; ++b) {
        FuBlock& B = a.blk[b];
        const size_t N = (size_t)B.c * B.Hf * B.Wh, s2 = pt_align_floats(2 * N);
        B.b = (float2*)base; B.r = (float2*)(base + s2); B.z = (float2*)(base + 2 * s2); B.q = (float2*)(base + 3 * s2);
        B.dM = base + 4 * s2; B.tmp = B.dM + pt_align_floats(N);
        base += fu_block_floats(B.Hf, B.Wh, B.c);
    }
    a.dp = precond_data_param; a.rp = precond_reg_param; a.forget = direction_forget_factor;
    a.fr = fletcher_reeves ? 1 : 0; a.std_alpha = standard_alpha ? 1 : 0; a.reset = direction_forget_factor == 0.f ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 gbin(maxbins, nb), gel((unsigned)((maxel + 255) / 256), nb);
    hipLaunchKernelGGL(k_eco_fu_setup, gbin, dim3(64), 0, st, a);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eco_fu_data, gbin, dim3(256), 0, st, a, 0, 0);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eco_fu_reg, gel, dim3(256), 0, st, a, 0, 0);
    PT_CHECK_LAUNCH();
    for (int it = 0; it < num_iter; ++it) {
        hipLaunchKernelGGL(k_eco_fu_rho, dim3(nb), dim3(1024), 0, st, a, it);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_eco_fu_data, gbin, dim3(256), 0, st, a, 1, it);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_eco_fu_reg, gel, dim3(256), 0, st, a, 1, it);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_eco_fu_step, dim3(nb), dim3(1024), 0, st, a, it == num_iter - 1 ? 1 : 0, it);
        PT_CHECK_LAUNCH();
    }
    return PT_OK;
}
