// ToMP transformer model predictor on gfx950 (BASELINE configs[3]).
//
// Replaces, for inference:
//   FilterPredictor.predict_filter / predict_cls_bbreg_filters_parallel   ltr/models/transformer/filter_predictor.py:50-150
//   Transformer.forward + post-norm encoder / decoder layers              ltr/models/transformer/transformer.py:90-96,172-180,224-238
//   PositionEmbeddingSine('lin_sine', avoid_aliazing)                     ltr/models/transformer/position_encoding.py:6-58
//   DenseBoxRegressor.forward, the Linear of LinearFilterClassifier       ltr/models/transformer/heads.py:93-98,119-141
//
// This path is MFMA-bound (45 GFLOP per frame, AI >> 100 flop/B), unlike the solver passes: every dense contraction runs
// on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation -- the reference computes in fp32 and north_star
// asks for 1e-4).  Layout: tokens are rows, `(batch row, token) x channel` row-major, so every nn.Linear is an NT GEMM
// with both operands K-contiguous; the NCHW <-> token-major transposes happen once on the way in and once on the way out.
//
//   k_gemm      C = A W^T (+bias, affine, ReLU, residual, exp), LDS-staged 64x64 / 64x32 / 32x32 tiles, register
//               prefetch of the next K-step, optional "+pos" on the A operand of the q/k column blocks, optional 3x3
//               gather on the A operand (implicit GEMM for the regression tower)
//   k_attn      fp32 flash attention: S^T = K Q^T per 16-key tile so that the MFMA accumulator of the score tile IS the
//               B operand of the PV product (no LDS round trip for P), online softmax per 64-key chunk
//   decoder     one query token per batch row: the K/V projections of the memory are never formed --
//               q.(Wk m + bk) = (Wk^T q).m + const and sum_l p_l (Wv m_l + bv) = Wv (sum_l p_l m_l) + bv, and the weight
//               products this leaves (Wo Wv, Wk_h^T Wq_h, Wo[:,h] Wv_h) are folded once per weight update
//               (pt_tomp_prepare_f32), so a layer is 5 GEMVs plus two MFMA passes over the memory
#include "common.h"
#include "pt_internal.h"
#include "mfma_gemm.h"

#include <algorithm>
#include <math.h>
#include <stdint.h>

namespace {

// A launch of this file that no dispatcher stands in front of: with a route log (the host-only query) its id is noted and nothing is
// queued; without one the kernel is launched and the launch status checked.  `log` is the enclosing function's PtRouteLog*.
#define PT_TOMP_LAUNCH(ID, ...)                   \
    do {                                          \
        if (log) {                                \
            pt_route_note(log, ID);               \
        } else {                                  \
            hipLaunchKernelGGL(__VA_ARGS__);      \
            PT_CHECK_LAUNCH();                    \
        }                                         \
    } while (0)

// ------------------------------------------------------------------------------------------------------------------
// fp32 flash attention over the packed (rows, 3D) q|k|v projections
// ------------------------------------------------------------------------------------------------------------------
struct AttnArgs {
    const float* qkv; unsigned qkv_bytes;
    float* out;
    int L, D, nhead;
    float scale;
    int mlo[8], mhi[8];                         // keys [mlo[b], mhi[b]) of batch row b are padding (never attended)
};

// Workgroup = 64 queries x 2 key halves: wavefronts 0-3 own the even 64-key chunks, 4-7 the odd ones (two wavefronts per
// SIMD, so one half's softmax / LDS waits hide behind the other's MFMAs -- B*nhead*L/16 query tiles alone are only one
// wavefront per SIMD); the halves' (max, sum, O^T) are merged through LDS at the end.
// (Issuing the exponentials of the next key tile between the PV MFMAs of the current one: same bits, no gain, 0.8875-0.8890 vs
// 0.8850-0.8878 ms -- profiles/r06q_attention_ablation.txt.)
template <int HD>
__global__ __launch_bounds__(512) void k_attn(AttnArgs a) {
    constexpr int KS = HD + 4, NV = HD / 4, NF4 = HD / 16, DT = HD / 16;   // NV floats of q/k per lane, NF4 float4s
    // LDS strides: K rows 4 mod 64 words, V rows 16 mod 32 words; together with the key permutation prow() below they
    // make the ds_read_b128 K fragments and the ds_read_b32 V operands bank-conflict free (see k_gemm for the lane
    // groups of ds_read_b128)
    constexpr int VS = HD <= 48 ? 48 : 80;
    __shared__ __attribute__((aligned(16))) float Ks[128 * KS];
    __shared__ __attribute__((aligned(16))) float Vs[128 * VS];
    auto prow = [](int i) { return (i >= 4 && i < 12) ? 2 * (i - 4) : (i < 4 ? 2 * i + 1 : 2 * i - 15); };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int half = wave >> 2, h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * 64 + (wave & 3) * 16;
    const int ld = 3 * a.D;
    const __amdgpu_buffer_rsrc_t rs = pt_rsrc(a.qkv, a.qkv_bytes);
    const long rowbase = (long)b * a.L;
    const int mlo = a.mlo[b], mhi = a.mhi[b];

    // Q fragment (B operand of S^T = K Q^T): lane (query li, k-slot kq) holds q[query][kq*NV .. +NV), pre-scaled
    float qf[NV];
    {
        const int q = min(q0 + li, a.L - 1);
        const unsigned off = (unsigned)(((rowbase + q) * ld + h * HD + kq * NV) * 4);
#pragma unroll
        for (int v = 0; v < NF4; ++v) {
            const f32x4 t = pt_bload4(rs, off + 16u * v);
#pragma unroll
            for (int e = 0; e < 4; ++e) qf[4 * v + e] = t[e] * a.scale;
        }
    }
    // cooperative K / V loads of 128 keys (one chunk per half) per iteration
    constexpr int LPT = (128 * HD / 4) / 512;                     // float4 per thread per operand
    constexpr int F4R = HD / 4;                                   // float4 per row
    f32x4 rk[LPT], rv[LPT];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + 512 * i, r = idx / F4R, c4 = (idx - r * F4R) * 4, key = c0 + r;
            const unsigned off = key < a.L ? (unsigned)(((rowbase + key) * ld + a.D + h * HD + c4) * 4) : OOB;
            rk[i] = pt_bload4(rs, off);
            rv[i] = pt_bload4(rs, off == OOB ? OOB : off + (unsigned)a.D * 4u);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + 512 * i, r = idx / F4R, c4 = (idx - r * F4R) * 4;
            *reinterpret_cast<f32x4*>(&Ks[r * KS + c4]) = rk[i];
            *reinterpret_cast<f32x4*>(&Vs[r * VS + c4]) = rv[i];
        }
    };

    f32x4 ot[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) ot[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // Padding keys (round 4).  A 128-key iteration that lies entirely inside the padding range [mlo, mhi) contributes exp(-inf) = 0
    // to every query and leaves (max, sum, O) bit for bit as they were: it is not fetched at all (ToMP's second batch row masks 324
    // of its 972 keys: two of its eight iterations).  A 64-key half chunk inside the range is skipped by its four wavefronts; one
    // that touches neither the range nor the end of the sequence runs without the per-key tests.
    const int nit = (a.L + 127) / 128;
    auto live = [&](int it) { return !(it * 128 >= mlo && it * 128 + 128 <= mhi); };
    int pk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pk[r] = prow(4 * kq + r);
    int it = 0;
    while (it < nit && !live(it)) ++it;
    if (it < nit) fetch(it * 128);
    while (it < nit) {
        int nx = it + 1;
        while (nx < nit && !live(nx)) ++nx;
        __syncthreads();                                          // previous iteration's LDS reads are done
        stash();
        __syncthreads();
        if (nx < nit) fetch(nx * 128);
        const int c0 = it * 128 + half * 64;
        it = nx;
        if (c0 >= a.L || (c0 >= mlo && c0 + 64 <= mhi)) continue;  // wave-uniform: nothing but padding in this half chunk
        const bool tests = c0 + 64 > a.L || (c0 < mhi && c0 + 64 > mlo);
        const float* Kh = Ks + half * 64 * KS;
        const float* Vh = Vs + half * 64 * VS;
        // ---- S^T tiles: rows = keys, cols = queries.  The K fragments of tile kt+1 (and the V operands of the first PV
        //      tile) are read while tile kt is multiplied; the sched_barriers keep the scheduler from sinking the reads to
        //      their first use (it did: one exposed LDS round trip per 2 PV MFMAs, per 8 S MFMAs).
        f32x4 st[4];
        float mc = -INFINITY;
        f32x4 kf[2][NF4];
        float vf[2][4][DT];
        auto read_k = [&](int kt, int set) {
            const float* kp = Kh + (kt * 16 + prow(li)) * KS + kq * NV;   // S^T row i of the tile <-> key prow(i)
#pragma unroll
            for (int v = 0; v < NF4; ++v) kf[set][v] = *reinterpret_cast<const f32x4*>(kp + 4 * v);
        };
        auto read_v = [&](int kt, int set) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vp = Vh + (kt * 16 + prow(4 * kq + r)) * VS + li;
#pragma unroll
                for (int d = 0; d < DT; ++d) vf[set][r][d] = vp[16 * d];
            }
        };
        read_k(0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kt < 3) read_k(kt + 1, (kt + 1) & 1);
            else read_v(0, 0);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < NF4; ++v) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sc = mfma16(kf[kt & 1][v][e], qf[4 * v + e], sc);
            }
            if (tests) {                                          // wave-uniform
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = c0 + kt * 16 + pk[r];
                    if (key >= a.L || (key >= mlo && key < mhi)) sc[r] = -INFINITY;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) mc = fmaxf(mc, sc[r]);
            st[kt] = sc;
            __builtin_amdgcn_sched_barrier(0);
        }
        mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
        mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
        const float m_new = fmaxf(m_run, mc);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __expf(m_run - m_use);                 // m_run = -inf -> 0
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < DT; ++d) ot[d] *= alpha;
        m_run = m_new;
        // ---- P^T = exp(S^T - m) feeds the PV product straight from the accumulator registers:
        //      O^T[d][query] += sum_key V[key][d] * P^T[key][query]; k-slot kq of MFMA r <-> key prow(4*kq + r) of the tile
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kt < 3) read_v(kt + 1, (kt + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pe = __expf(st[kt][r] - m_use);
                l_run += pe;
#pragma unroll
                for (int d = 0; d < DT; ++d) ot[d] = mfma16(vf[kt & 1][r][d], pe, ot[d]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    // ---- merge the two key halves (the exchange area aliases the K staging buffer)
    __syncthreads();
    float* xch = Ks + ((wave & 3) * 64 + lane) * (4 * DT + 2);
    if (half == 1) {
        xch[0] = m_run;
        xch[1] = l_run;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) xch[2 + 4 * d + r] = ot[d][r];
    }
    __syncthreads();
    if (half == 0) {
        const float m1 = xch[0], l1 = xch[1];
        const float m = fmaxf(m_run, m1);
        const float a0 = __expf(m_run - m), a1 = m1 == -INFINITY ? 0.f : __expf(m1 - m);
        const float inv = 1.f / (l_run * a0 + l1 * a1);
        const int q = q0 + li;
        if (q < a.L) {
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                f32x4 o;                                           // rows d*16 + 4*kq + r of O^T = 4 consecutive channels
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (ot[d][r] * a0 + xch[2 + 4 * d + r] * a1) * inv;
                *reinterpret_cast<f32x4*>(&a.out[(rowbase + q) * a.D + h * HD + d * 16 + 4 * kq]) = o;
            }
        }
    }
}

// head width -> instantiation (dims_check admits 16 / 32 / 64 only)
int attn_route(int HD) { return HD == 32 ? PT_TOMP_R_ATTN32 : HD == 16 ? PT_TOMP_R_ATTN16 : PT_TOMP_R_ATTN64; }

int launch_attn(const AttnArgs& at, int B, hipStream_t st, PtRouteLog* log) {
    const int route = attn_route(at.D / at.nhead);
    if (log) {
        pt_route_note(log, route);
        return PT_OK;
    }
    const dim3 ag((at.L + 63) / 64, at.nhead, B);
    if (route == PT_TOMP_R_ATTN32) hipLaunchKernelGGL((k_attn<32>), ag, dim3(512), 0, st, at);
    else if (route == PT_TOMP_R_ATTN16) hipLaunchKernelGGL((k_attn<16>), ag, dim3(512), 0, st, at);
    else hipLaunchKernelGGL((k_attn<64>), ag, dim3(512), 0, st, at);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// row LayerNorm, one wavefront per row (D % 64 == 0, D <= 512); in-place safe
// ------------------------------------------------------------------------------------------------------------------
// PER = D / 64 known at compile time: the row is ONE vector load per lane and gamma / beta are requested with it (with a run-time
// count the loop stayed rolled -- a memory round trip per element -- and gamma / beta were read behind both reductions)
// in2 / in3 (optional, same layout): further addends of the row -- the second half of a split-K product and the residual the
// GEMM epilogue would have added (v = (in + in2) + in3, fixed order)
template <int PER>
__global__ __launch_bounds__(256) void k_ln_rows_t(const float* in, float* out, const float* __restrict__ gam,
                                                   const float* __restrict__ bet, int rows, const float* in2 = nullptr,
                                                   const float* in3 = nullptr, const float* gam2 = nullptr, const float* bet2 = nullptr,
                                                   const float* in4 = nullptr, const float* in5 = nullptr) {
    constexpr int D = 64 * PER;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float v[PER], g[PER], b[PER];
    const long ro = (long)row * D + lane * PER;
    const float* src = in + ro;
    if (PER == 4) {
        const f32x4 t = *(const f32x4*)src, tg = *(const f32x4*)(gam + lane * 4), tb = *(const f32x4*)(bet + lane * 4);
        f32x4 t2 = {0, 0, 0, 0}, t3 = {0, 0, 0, 0}, t4 = {0, 0, 0, 0}, t5 = {0, 0, 0, 0};
        if (in2) t2 = *(const f32x4*)(in2 + ro);                     // uniform branches: all loads requested together
        if (in3) t3 = *(const f32x4*)(in3 + ro);
        if (in4) { t4 = *(const f32x4*)(in4 + ro); t5 = *(const f32x4*)(in5 + ro); }   // splits 3 and 4 of a four-way split-K product (both or neither)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = in4 ? (((t[i] + t2[i]) + t4[i]) + t5[i]) + t3[i] : (in2 ? (t[i] + t2[i]) + t3[i] : t[i]);
            g[i] = tg[i]; b[i] = tb[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            v[i] = src[i];
            if (in2) v[i] = (v[i] + in2[ro + i]) + (in3 ? in3[ro + i] : 0.f);
            g[i] = gam[lane * PER + i]; b[i] = bet[lane * PER + i];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += v[i];
    const float mean = wave_sum(s) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) q += (v[i] - mean) * (v[i] - mean);
    const float rstd = rsqrtf(wave_sum(q) / D + 1e-5f);
    float* dst = out + (long)row * D + lane * PER;
    if (gam2) {                                                     // uniform: a second LayerNorm on the result (the decoder's norm3 + final norm)
        float o[PER], s2 = 0.f;
#pragma unroll
        for (int i = 0; i < PER; ++i) { o[i] = (v[i] - mean) * rstd * g[i] + b[i]; s2 += o[i]; }
        const float mean2 = wave_sum(s2) / D;
        float q2 = 0.f;
#pragma unroll
        for (int i = 0; i < PER; ++i) q2 += (o[i] - mean2) * (o[i] - mean2);
        const float rstd2 = rsqrtf(wave_sum(q2) / D + 1e-5f);
#pragma unroll
        for (int i = 0; i < PER; ++i) dst[i] = (o[i] - mean2) * rstd2 * gam2[lane * PER + i] + bet2[lane * PER + i];
        return;
    }
    if (PER == 4) {
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (v[i] - mean) * rstd * g[i] + b[i];
        *(f32x4*)dst = o;
    } else {
#pragma unroll
        for (int i = 0; i < PER; ++i) dst[i] = (v[i] - mean) * rstd * g[i] + b[i];
    }
}

__global__ __launch_bounds__(256) void k_ln_rows(const float* in, float* out, const float* gam, const float* bet,
                                                 int rows, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int per = D / 64;
    float v[8];
    float s = 0.f;
    for (int i = 0; i < per; ++i) {
        v[i] = in[(long)row * D + lane * per + i];
        s += v[i];
    }
    const float mean = wave_sum(s) / D;
    float q = 0.f;
    for (int i = 0; i < per; ++i) q += (v[i] - mean) * (v[i] - mean);
    const float rstd = rsqrtf(wave_sum(q) / D + 1e-5f);
    for (int i = 0; i < per; ++i) {
        const int c = lane * per + i;
        out[(long)row * D + c] = (v[i] - mean) * rstd * gam[c] + bet[c];
    }
}

// in2 / in3 are only served by the 256-wide vector path: callers check ln_rows_wide_ok() first
static bool ln_rows_wide_ok(const float* in, const float* out, const float* gam, const float* bet, int D) {
    return D == 256 && ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((uintptr_t)gam % 16 == 0) && ((uintptr_t)bet % 16 == 0);
}

// The kernel launch_ln_rows runs (PT_TOMP_R_LN*), from the operands alone.  PT_ERR_UNSUPPORTED when extra operands are given that only
// the 256-wide vector kernel serves and that kernel cannot be used: dropping in2 / in3 / the second norm silently would lose the split-K
// half, the residual or a LayerNorm.
static int ln_rows_route(const float* in, const float* out, const float* gam, const float* bet, int D, const float* in2, const float* in3,
                         const float* gam2, const float* bet2, const float* in4, const float* in5, int* route) {
    const bool al = ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((uintptr_t)gam % 16 == 0) && ((uintptr_t)bet % 16 == 0) &&
                    ((uintptr_t)in2 % 16 == 0) && ((uintptr_t)in3 % 16 == 0) && ((uintptr_t)gam2 % 16 == 0) && ((uintptr_t)bet2 % 16 == 0) &&
                    ((uintptr_t)in4 % 16 == 0) && ((uintptr_t)in5 % 16 == 0);
    if (!(D == 256 && al) && (in2 || in3 || gam2 || bet2 || in4 || in5)) return PT_ERR_UNSUPPORTED;
    if ((in4 == nullptr) != (in5 == nullptr) || (in4 && !in2)) return PT_ERR_UNSUPPORTED;
    if (D == 256 && al) *route = gam2 ? PT_TOMP_R_LN256_DOUBLE : in4 ? PT_TOMP_R_LN256_SPLIT4 : (in2 || in3) ? PT_TOMP_R_LN256_SPLIT2 : PT_TOMP_R_LN256;
    else if (D == 128) *route = PT_TOMP_R_LN128;
    else if (D == 64) *route = PT_TOMP_R_LN64;
    else *route = PT_TOMP_R_LN_GENERIC;
    return PT_OK;
}

// Nothing is queued when the status is not PT_OK, or when a route log is given (the route is noted instead).
static int launch_ln_rows(const float* in, float* out, const float* gam, const float* bet, int rows, int D, hipStream_t st, PtRouteLog* log,
                          const float* in2 = nullptr, const float* in3 = nullptr, const float* gam2 = nullptr,
                          const float* bet2 = nullptr, const float* in4 = nullptr, const float* in5 = nullptr) {
    int route = 0;
    const int rc = ln_rows_route(in, out, gam, bet, D, in2, in3, gam2, bet2, in4, in5, &route);
    if (rc) return rc;
    if (log) {
        pt_route_note(log, route);
        return PT_OK;
    }
    const dim3 grid((rows + 3) / 4), block(256);
    switch (route) {
    case PT_TOMP_R_LN128: hipLaunchKernelGGL(k_ln_rows_t<2>, grid, block, 0, st, in, out, gam, bet, rows); break;
    case PT_TOMP_R_LN64: hipLaunchKernelGGL(k_ln_rows_t<1>, grid, block, 0, st, in, out, gam, bet, rows); break;
    case PT_TOMP_R_LN_GENERIC: hipLaunchKernelGGL(k_ln_rows, grid, block, 0, st, in, out, gam, bet, rows, D); break;
    default: hipLaunchKernelGGL(k_ln_rows_t<4>, grid, block, 0, st, in, out, gam, bet, rows, in2, in3, gam2, bet2, in4, in5); break;
    }
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// token build (filter_predictor.py:113-128)
// ------------------------------------------------------------------------------------------------------------------
struct TokArgs {
    const float *train, *test, *label, *fg, *testtok;
    float* X;
    int nf, ns, dup, D, HW, L;
    float* zero; int nzero;         // a buffer this launch clears on the side (the decoder's initial state: no memset node per frame)
    // two more side jobs (round 4): `rep` copies of cp_src[k] (cp_n[k] floats) into cp_dst[k] -- the first decoder layer's state
    // after self-attention and its folded query do not depend on the frame (the decoder starts from zeros) and come from the
    // prepared buffer instead of two GEMV launches
    const float* cp_src[2]; float* cp_dst[2]; int cp_n[2]; int rep;
};

// NCHW feature maps -> token-major rows, + fg_token * label (memory frames) or + test_token (test frame)
__global__ __launch_bounds__(256) void k_tomp_tokens(TokArgs a) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < a.nzero; i += 256) a.zero[i] = 0.f;
    if (blockIdx.z == 0 && blockIdx.y >= 1 && blockIdx.y <= 2 && a.cp_src[blockIdx.y - 1]) {     // spread over the blocks of row y
        const int k = blockIdx.y - 1, n = a.cp_n[k];
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n * a.rep; i += gridDim.x * 256) a.cp_dst[k][i] = a.cp_src[k][i % n];
    }
    const int B = a.dup ? 2 : a.ns;
    const int fr = blockIdx.z / B, b = blockIdx.z - fr * B, s = a.dup ? 0 : b;
    const bool train = fr < a.nf;
    const float* src = train ? a.train + ((long)(fr * a.ns + s) * a.D) * a.HW : a.test + ((long)s * a.D) * a.HW;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        tile[ty + 8 * i][tx] = (c < a.D && p < a.HW) ? src[(long)c * a.HW + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        if (p >= a.HW || c >= a.D) continue;
        float v = tile[tx][ty + 8 * i];
        v += train ? a.fg[c] * a.label[(long)(fr * a.ns + s) * a.HW + p] : a.testtok[c];
        a.X[((long)b * a.L + (long)fr * a.HW + p) * a.D + c] = v;
    }
}

struct BoxArgs {
    const float *ltrb, *w1, *b1, *bn1, *bn2;     // bn: [weight, bias, running_mean, running_var] of D4 / D floats
    float *E1, *scale2, *shift2;
    int nf, ns, dup, D, D4, HW;
};

// first layer of the ltrb MLP (Conv1d 4 -> D/4, BatchNorm1d on running statistics, ReLU) and the folded scale / shift
// of the second BatchNorm for the epilogue of the next GEMM (filter_predictor.py:6-17)
__global__ __launch_bounds__(256) void k_tomp_box1(BoxArgs a) {
    const int B = a.dup ? 2 : a.ns, Ltr = a.nf * a.HW;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < a.D; c += 256) {
            const float sc = a.bn2[c] / sqrtf(a.bn2[3 * a.D + c] + 1e-5f);
            a.scale2[c] = sc;
            a.shift2[c] = a.bn2[a.D + c] - a.bn2[2 * a.D + c] * sc;
        }
    }
    if (idx >= (long)B * Ltr * a.D4) return;
    const int j = (int)(idx % a.D4);
    const long row = idx / a.D4;
    const int b = (int)(row / Ltr), l = (int)(row - (long)b * Ltr), fr = l / a.HW, p = l - fr * a.HW;
    const int s = a.dup ? 0 : b;
    const float* t = a.ltrb + ((long)(fr * a.ns + s) * 4) * a.HW + p;
    float e = a.b1[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) e += a.w1[j * 4 + i] * t[(long)i * a.HW];
    e = (e - a.bn1[2 * a.D4 + j]) / sqrtf(a.bn1[3 * a.D4 + j] + 1e-5f) * a.bn1[j] + a.bn1[a.D4 + j];
    a.E1[idx] = fmaxf(e, 0.f);
}

// token-major rows of the test frame -> NCHW (enc_opt, filter_predictor.py:142-147)
__global__ __launch_bounds__(256) void k_tokens_to_nchw(const float* X, float* out, int B, int L, int D, int HW,
                                                        int l0) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (p < HW && c < D) ? X[((long)b * L + l0 + p) * D + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        if (c < D && p < HW) out[((long)b * D + c) * HW + p] = tile[tx][ty + 8 * i];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// positional encoding (position_encoding.py:6-58), written once per map size and cached by the caller
// ------------------------------------------------------------------------------------------------------------------
__global__ void k_tomp_posenc(float* pos, int H, int W, int D, double factor) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= H * W * D) return;
    const int p = idx / D, c = idx - p * D, depth = D / 4;
    const int y = p / W, x = p - y * W;
    const bool cosine = c >= 2 * depth;
    const int cc = cosine ? c - 2 * depth : c;
    const int i = cc / 2 + 1, isy = cc & 1;
    const float coord = isy ? ((float)(y + 1) - 0.5f) / ((float)H + 1e-6f) : ((float)(x + 1) - 0.5f) / ((float)W + 1e-6f);
    const float arg = (float)((double)i * factor * 3.14159265358979323846) * coord;   // scalar rounded to fp32, fp32 product
    pos[idx] = cosine ? cosf(arg) : sinf(arg);
}

// ------------------------------------------------------------------------------------------------------------------
// decoder: GEMV family (one wavefront per output feature; B <= 8 batch rows ride along in registers)
// ------------------------------------------------------------------------------------------------------------------
struct GemvArgs {
    const float* Wt; const float* bias; int N, K;
    const float* x;                                 // (B, K) input rows
    const float *xg, *xb;                           // optional LayerNorm applied to the input rows (K = model width)
    const float* xadd;                              // optional (K) vector added to every input row after the LayerNorm
    const float* res; const float *rg, *rb;         // optional residual rows (B, N), optionally LayerNorm'ed
    int relu, B;
    float* out;
};

template <int V>
__device__ __forceinline__ void ldv(const float* p, float* out) {      // V consecutive floats, 16-byte aligned when V = 4
    if (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = t[3];
    } else {
        out[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void wave_row_stats(const float* x, int K, int lane, float& mean, float& rstd) {
    float s = 0.f;
    for (int k = lane * V; k < K; k += 64 * V) {
        float t[V];
        ldv<V>(x + k, t);
#pragma unroll
        for (int e = 0; e < V; ++e) s += t[e];
    }
    mean = wave_sum(s) / K;
    float q = 0.f;
    for (int k = lane * V; k < K; k += 64 * V) {
        float t[V];
        ldv<V>(x + k, t);
#pragma unroll
        for (int e = 0; e < V; ++e) q += (t[e] - mean) * (t[e] - mean);
    }
    rstd = rsqrtf(wave_sum(q) / K + 1e-5f);
}

template <int V>
__global__ __launch_bounds__(256) void k_gemv(GemvArgs a) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= a.N) return;
    float acc[8], mean[8], rstd[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        acc[b] = 0.f;
        mean[b] = 0.f;
        rstd[b] = 1.f;
    }
    // all weight loads of the row are issued before anything that has to wait (LayerNorm statistics of the input and of
    // the residual are two dependent reductions each): the chain is latency, not bandwidth
    constexpr int WCH = 8;
    const float* w = a.Wt + (long)n * a.K;
    const int nch = a.K / (64 * V);
    const bool pre = nch <= WCH;
    float wreg[WCH][V];
    if (pre) {
#pragma unroll
        for (int ch = 0; ch < WCH; ++ch)
            if (ch < nch) ldv<V>(w + ch * 64 * V + lane * V, wreg[ch]);
    }
    const float bias = a.bias ? a.bias[n] : 0.f;
    float rterm[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) rterm[b] = 0.f;
    // <= 2 batch rows of <= 64*V*WCH elements (the decoder's shapes): the input rows and the residual rows are read ONCE,
    // together with the weights, and their LayerNorm statistics come from registers -- otherwise every statistic is two
    // dependent sweeps through memory and the dot product a third
    const bool cached = pre && a.B <= 2 && (!a.rg || a.N <= 64 * V * WCH);
    float xc[2][WCH][V];
    if (cached) {
        float rc[2][WCH][V];
        const int nrc = a.rg ? a.N / (64 * V) : 0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b >= a.B) continue;
#pragma unroll
            for (int ch = 0; ch < WCH; ++ch) {
                if (ch < nch) ldv<V>(a.x + (long)b * a.K + ch * 64 * V + lane * V, xc[b][ch]);
                if (ch < nrc) ldv<V>(a.res + (long)b * a.N + ch * 64 * V + lane * V, rc[b][ch]);
            }
        }
        float rn[2] = {0.f, 0.f};
        if (a.res) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (b < a.B) rn[b] = a.res[(long)b * a.N + n];
        }
        auto stats = [&](float (&v)[WCH][V], int nc, int len, float& m, float& rs) {     // same two-pass formula, from registers
            float s = 0.f;
#pragma unroll
            for (int ch = 0; ch < WCH; ++ch)
                if (ch < nc) {
#pragma unroll
                    for (int e = 0; e < V; ++e) s += v[ch][e];
                }
            m = wave_sum(s) / len;
            float q = 0.f;
#pragma unroll
            for (int ch = 0; ch < WCH; ++ch)
                if (ch < nc) {
#pragma unroll
                    for (int e = 0; e < V; ++e) q += (v[ch][e] - m) * (v[ch][e] - m);
                }
            rs = rsqrtf(wave_sum(q) / len + 1e-5f);
        };
        if (a.res) {
            const float rgn = a.rg ? a.rg[n] : 1.f, rbn = a.rg ? a.rb[n] : 0.f;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (b >= a.B) continue;
                float m = 0.f, rs = 1.f;
                if (a.rg) stats(rc[b], nrc, a.N, m, rs);
                rterm[b] = (rn[b] - m) * rs * rgn + rbn;
            }
        }
        if (a.xg) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (b < a.B) stats(xc[b], nch, a.K, mean[b], rstd[b]);
        }
    } else {
        if (a.res) {
            const float rgn = a.rg ? a.rg[n] : 1.f, rbn = a.rg ? a.rb[n] : 0.f;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (b >= a.B) continue;
                const float* r = a.res + (long)b * a.N;
                float m = 0.f, rs = 1.f;
                if (a.rg) wave_row_stats<V>(r, a.N, lane, m, rs);
                rterm[b] = (r[n] - m) * rs * rgn + rbn;
            }
        }
        if (a.xg) {
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (b < a.B) wave_row_stats<V>(a.x + (long)b * a.K, a.K, lane, mean[b], rstd[b]);
        }
    }
    auto body = [&](int k, const float* wv, int ch) {
        float gv[V], bv[V], av[V];
#pragma unroll
        for (int e = 0; e < V; ++e) gv[e] = 1.f, bv[e] = 0.f, av[e] = 0.f;
        if (a.xg) {
            ldv<V>(a.xg + k, gv);
            ldv<V>(a.xb + k, bv);
        }
        if (a.xadd) ldv<V>(a.xadd + k, av);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (b >= a.B) continue;
            float xr[V];
            if (cached && b < 2 && ch >= 0) {
#pragma unroll
                for (int e = 0; e < V; ++e) xr[e] = xc[b][ch][e];
            } else {
                ldv<V>(a.x + (long)b * a.K + k, xr);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float xv = (xr[e] - mean[b]) * rstd[b] * gv[e] + bv[e];
                xv += av[e];
                acc[b] += wv[e] * xv;
            }
        }
    };
    if (pre) {
#pragma unroll
        for (int ch = 0; ch < WCH; ++ch)
            if (ch < nch) body(ch * 64 * V + lane * V, wreg[ch], ch);
    } else {
        for (int k = lane * V; k < a.K; k += 64 * V) {
            float wv[V];
            ldv<V>(w + k, wv);
            body(k, wv, -1);
        }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if (b >= a.B) continue;
        float v = wave_sum(acc[b]) + bias;
        if (a.relu) v = fmaxf(v, 0.f);
        v += rterm[b];
        if (lane == 0) a.out[(long)b * a.N + n] = v;
    }
}

// The decoder's GEMVs (<= 2 batch rows, K = 256 * NCH): the `cached` path of k_gemv as its own kernel.  What the prologue needs to
// REQUEST every operand arrives as preloaded scalar parameters (six pointers, two packed words = 14 dwords); bias / residual-LayerNorm
// parameters / output pointer are fetched behind the loads (pt_late_args).  The LayerNorm gamma / beta of the input and the additive
// vector are requested with the weights instead of behind the statistics.  Same arithmetic in the same order as k_gemv.
struct GemvLate { pt_gcf bias, rg, rb; pt_gf out; };
template <int NCH>
__global__ __launch_bounds__(256) void k_gemv_dec(const float* __restrict__ Wt, const float* __restrict__ x, const float* __restrict__ xg,
                                                  const float* __restrict__ xb, const float* __restrict__ xadd,
                                                  const float* __restrict__ res, unsigned nk, unsigned flags, GemvLate l_arg) {
    constexpr int V = 4, WCH = 8;
    const int N = (int)(nk & 0xffffu), K = (int)(nk >> 16);
    const int B = (int)(flags & 15u), nrc = (int)((flags >> 8) & 15u);
    const bool relu = (flags >> 4) & 1u, has_rg = (flags >> 5) & 1u;
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* w = Wt + (long)n * K;
    float wreg[NCH][V], xc[2][NCH][V], gv[NCH][V], bv[NCH][V], av[NCH][V], rc[2][WCH][V];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int k = ch * 64 * V + lane * V;
        ldv<V>(w + k, wreg[ch]);
#pragma unroll
        for (int b = 0; b < 2; ++b)
            if (b < B) ldv<V>(x + (long)b * K + k, xc[b][ch]);
#pragma unroll
        for (int e = 0; e < V; ++e) gv[ch][e] = 1.f, bv[ch][e] = 0.f, av[ch][e] = 0.f;
        if (xg) {
            ldv<V>(xg + k, gv[ch]);
            ldv<V>(xb + k, bv[ch]);
        }
        if (xadd) ldv<V>(xadd + k, av[ch]);
    }
    float rn[2] = {0.f, 0.f};
    if (res) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b >= B) continue;
            rn[b] = res[(long)b * N + n];
            if (has_rg) {
#pragma unroll
                for (int ch = 0; ch < WCH; ++ch)
                    if (ch < nrc) ldv<V>(res + (long)b * N + ch * 64 * V + lane * V, rc[b][ch]);
            }
        }
    }
    const GemvLate l = pt_late_args<GemvLate>(56);                  // 6 pointers + 2 dwords = 56 bytes
    const float bias = l.bias ? l.bias[n] : 0.f;
    const float rgn = has_rg ? l.rg[n] : 1.f, rbn = has_rg ? l.rb[n] : 0.f;
    float mean[2] = {0.f, 0.f}, rstd[2] = {1.f, 1.f}, rterm[2] = {0.f, 0.f};
    if (res) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b >= B) continue;
            float m = 0.f, rs = 1.f;
            if (has_rg) {                                           // the two-pass formula of wave_row_stats, from registers
                float s = 0.f;
#pragma unroll
                for (int ch = 0; ch < WCH; ++ch)
                    if (ch < nrc) {
#pragma unroll
                        for (int e = 0; e < V; ++e) s += rc[b][ch][e];
                    }
                m = wave_sum(s) / N;
                float q = 0.f;
#pragma unroll
                for (int ch = 0; ch < WCH; ++ch)
                    if (ch < nrc) {
#pragma unroll
                        for (int e = 0; e < V; ++e) q += (rc[b][ch][e] - m) * (rc[b][ch][e] - m);
                    }
                rs = rsqrtf(wave_sum(q) / N + 1e-5f);
            }
            rterm[b] = (rn[b] - m) * rs * rgn + rbn;
        }
    }
    if (xg) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b >= B) continue;
            float s = 0.f;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int e = 0; e < V; ++e) s += xc[b][ch][e];
            mean[b] = wave_sum(s) / K;
            float q = 0.f;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int e = 0; e < V; ++e) q += (xc[b][ch][e] - mean[b]) * (xc[b][ch][e] - mean[b]);
            rstd[b] = rsqrtf(wave_sum(q) / K + 1e-5f);
        }
    }
    float acc[2] = {0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b >= B) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float xv = (xc[b][ch][e] - mean[b]) * rstd[b] * gv[ch][e] + bv[ch][e];
                xv += av[ch][e];
                acc[b] += wreg[ch][e] * xv;
            }
        }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (b >= B) continue;
        float v = wave_sum(acc[b]) + bias;
        if (relu) v = fmaxf(v, 0.f);
        v += rterm[b];
        if (lane == 0) l.out[(long)b * N + n] = v;
    }
}

// The kernel launch_gemv runs (PT_TOMP_R_GEMV_*), from the arguments alone
int gemv_route(const GemvArgs& a, int* route) {
    if (a.B > 8 || a.K % 64 != 0 || (a.rg && a.N % 64 != 0)) return PT_ERR_UNSUPPORTED;
    const bool v4 = a.K % 256 == 0 && (!a.rg || a.N % 256 == 0);
    const int nch = a.K / 256;
    auto al16 = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
    const bool dec = v4 && a.B <= 2 && (nch == 1 || nch == 2 || nch == 4 || nch == 8) && a.N < 65536 && (!a.rg || (a.res && a.N <= 2048)) &&
                     al16(a.Wt) && al16(a.x) && al16(a.xg) && al16(a.xb) && al16(a.xadd) && al16(a.res);
    if (dec) *route = nch == 1 ? PT_TOMP_R_GEMV_DEC1 : nch == 2 ? PT_TOMP_R_GEMV_DEC2 : nch == 4 ? PT_TOMP_R_GEMV_DEC4 : PT_TOMP_R_GEMV_DEC8;
    else *route = v4 ? PT_TOMP_R_GEMV_V4 : PT_TOMP_R_GEMV_V1;
    return PT_OK;
}

int launch_gemv(const GemvArgs& a, hipStream_t st, PtRouteLog* log = nullptr) {
    int route = 0;
    const int rc = gemv_route(a, &route);
    if (rc) return rc;
    if (log) {
        pt_route_note(log, route);
        return PT_OK;
    }
    const dim3 grid((a.N + 3) / 4), block(256);
    if (route == PT_TOMP_R_GEMV_V4) {
        hipLaunchKernelGGL((k_gemv<4>), grid, block, 0, st, a);
    } else if (route == PT_TOMP_R_GEMV_V1) {
        hipLaunchKernelGGL((k_gemv<1>), grid, block, 0, st, a);
    } else {
        const unsigned nk = (unsigned)a.N | ((unsigned)a.K << 16);
        const unsigned flags = (unsigned)a.B | ((a.relu ? 1u : 0u) << 4) | ((a.rg ? 1u : 0u) << 5) | ((unsigned)(a.rg ? a.N / 256 : 0) << 8);
        const GemvLate l{(pt_gcf)a.bias, (pt_gcf)a.rg, (pt_gcf)a.rb, (pt_gf)a.out};
#define PT_GEMV_DEC(NC) hipLaunchKernelGGL((k_gemv_dec<NC>), grid, block, 0, st, a.Wt, a.x, a.xg, a.xb, a.xadd, a.res, nk, flags, l)
        if (route == PT_TOMP_R_GEMV_DEC1) PT_GEMV_DEC(1);
        else if (route == PT_TOMP_R_GEMV_DEC2) PT_GEMV_DEC(2);
        else if (route == PT_TOMP_R_GEMV_DEC4) PT_GEMV_DEC(4);
        else PT_GEMV_DEC(8);
#undef PT_GEMV_DEC
    }
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// One-time folding of the decoder's weight products (pt_tomp_prepare_f32).  With a single query token per batch row
//   self-attention      out_proj(v_proj(t))                  = (Wo Wv) t + (Wo bv + bo)
//   query . key         q_h . (Wk_h (m + pos))               = (Wk_h^T Wq_h x + Wk_h^T bq_h) . (m + pos)   [+ const in l]
//   value + out_proj    Wo concat_h(Wv_h ctx_h + bv_h) + bo  = sum_h (Wo[:, h] Wv_h) ctx_h + (Wo bv + bo)
// so a decoder layer is 5 GEMVs + 2 passes over the memory instead of 8 + 2.  Plain loops: runs once per weight update.
__global__ void k_prep_sa(const float* Wo, const float* bo, const float* Wv, const float* bv, float* Wsa, float* bsa,
                          int D) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= D * D) return;
    const int i = idx / D, j = idx - i * D;
    float s = 0.f;
    for (int k = 0; k < D; ++k) s += Wo[i * D + k] * Wv[k * D + j];
    Wsa[idx] = s;
    if (j == 0) {
        float t = bo[i];
        for (int k = 0; k < D; ++k) t += Wo[i * D + k] * bv[k];
        bsa[i] = t;
    }
}

__global__ void k_prep_mq(const float* Wq, const float* bq, const float* Wk, float* Mq, float* cq, int D, int nhead,
                          float scale) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)nhead * D * D) return;
    const int HD = D / nhead, h = (int)(idx / ((long)D * D)), c = (int)((idx / D) % D), k = (int)(idx % D);
    float s = 0.f, t = 0.f;
    for (int j = 0; j < HD; ++j) {
        const float wk = Wk[(long)(h * HD + j) * D + c];
        s += wk * Wq[(long)(h * HD + j) * D + k];
        t += wk * bq[h * HD + j];
    }
    Mq[idx] = s * scale;
    if (k == 0) cq[h * D + c] = t * scale;
}

__global__ void k_prep_ov(const float* Wo, const float* bo, const float* Wv, const float* bv, float* Wov, float* bov,
                          int D, int nhead) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)D * nhead * D) return;
    const int HD = D / nhead, n = (int)(idx / ((long)nhead * D)), h = (int)((idx / D) % nhead), c = (int)(idx % D);
    float s = 0.f;
    for (int j = 0; j < HD; ++j) s += Wo[(long)n * D + h * HD + j] * Wv[(long)(h * HD + j) * D + c];
    Wov[idx] = s;
    if (h == 0 && c == 0) {
        float t = bo[n];
        for (int j = 0; j < D; ++j) t += Wo[(long)n * D + j] * bv[j];
        bov[n] = t;
    }
}

struct DecAttnArgs {
    const float *mem, *pos, *qk;
    float *scores, *ctx;
    int B, L, D, nhead, HW;
    int mlo[8], mhi[8];
};

// scores[b][h][l] = qk[b][h] . (mem[b][l] + pos[l % HW]) as a (16 rows x 16 heads) MFMA tile per wavefront:
// A = 16 memory rows (+pos), B = the folded queries of the (<= 16) heads, K = channels
__global__ __launch_bounds__(64) void k_dec_scores(DecAttnArgs a) {
    const int lane = threadIdx.x, li = lane & 15, kq = lane >> 4, b = blockIdx.y, l0 = blockIdx.x * 16;
    const int l = min(l0 + li, a.L - 1);
    const __amdgpu_buffer_rsrc_t rm = pt_rsrc(a.mem, (unsigned)((long)a.B * a.L * a.D * 4));
    const __amdgpu_buffer_rsrc_t rp = pt_rsrc(a.pos, (unsigned)((long)a.HW * a.D * 4));
    const __amdgpu_buffer_rsrc_t rq = pt_rsrc(a.qk, (unsigned)((long)a.B * a.nhead * a.D * 4));
    const unsigned om = (unsigned)((((long)b * a.L + l) * a.D + 4 * kq) * 4);
    const unsigned op = (unsigned)(((long)(l % a.HW) * a.D + 4 * kq) * 4);
    const unsigned oq = li < a.nhead ? (unsigned)((((long)b * a.nhead + li) * a.D + 4 * kq) * 4) : OOB;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nks = a.D / 16;                                     // D % 64 == 0: whole batches of 4 k-steps
    for (int k0 = 0; k0 < nks; k0 += 4) {                         // 12 loads in flight, then 16 MFMAs (24 in flight: measured slower, round 4)
        f32x4 m[4], pp[4], qv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            m[u] = pt_bload4(rm, om + 64u * (k0 + u));
            pp[u] = pt_bload4(rp, op + 64u * (k0 + u));
            qv[u] = pt_bload4(rq, oq == OOB ? OOB : oq + 64u * (k0 + u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma16(m[u][e] + pp[u][e], qv[u][e], acc);
    }
    if (li < a.nhead) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ll = l0 + 4 * kq + r;
            if (ll < a.L)
                a.scores[((long)b * a.nhead + li) * a.L + ll] = (ll >= a.mlo[b] && ll < a.mhi[b]) ? -INFINITY : acc[r];
        }
    }
}

// ctx[b][h][c] = sum_l softmax(scores[b][h])[l] * mem[b][l][c]: grid (D/16, B), 16 wavefronts.  Prologue: wavefront h
// turns scores[b][h] into exp(s - max) in LDS and keeps 1/sum; then every wavefront contracts its share of the memory
// rows on MFMA (A = probabilities of the <= 16 heads, B = 16 channels of 4 memory rows), partial tiles reduced in LDS
__global__ __launch_bounds__(1024) void k_dec_ctx(DecAttnArgs a) {
    extern __shared__ float sm[];                                // nhead * Lp probabilities, 16 inverse sums, 16 x 256 partials
    const int Lp = (a.L + 3) & ~3;
    float* p = sm;
    float* inv = sm + (size_t)a.nhead * Lp;
    float* part = inv + 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, c0 = blockIdx.x * 16;
    // the first round of memory rows is requested in front of the softmax (it does not depend on it)
    const __amdgpu_buffer_rsrc_t rm = pt_rsrc(a.mem, (unsigned)((long)a.B * a.L * a.D * 4));
    const int nks = Lp / 4;
    float mv0[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k2 = wave + 16 * u, l = 4 * k2 + kq;
        mv0[u] = pt_bload1(rm, (k2 < nks && l < a.L) ? (unsigned)((((long)b * a.L + l) * a.D + c0 + li) * 4) : OOB);
    }
    if (wave < a.nhead) {
        // the head's score row in ONE batch of loads (L <= 1408 by the LDS budget the launcher checks: 22 per lane), kept in
        // registers for both softmax passes.  As two strided loops with a run-time bound (round 3) every element was its own
        // memory round trip, twice: 32 dependent round trips = the kernel's 10 us (round 4: profiles/r04x_*)
        constexpr int NSV = 22;
        const float* s = a.scores + ((long)b * a.nhead + wave) * a.L;
        if (a.L > 64 * NSV) {                                       // uniform: longer rows (few heads) keep the two strided passes
            float mx = -INFINITY;
            for (int l = lane; l < a.L; l += 64) mx = fmaxf(mx, s[l]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int l = lane; l < Lp; l += 64) {
                const float e = l < a.L ? __expf(s[l] - mx) : 0.f;
                p[(size_t)wave * Lp + l] = e;
                sum += e;
            }
            sum = wave_sum(sum);
            if (lane == 0) inv[wave] = 1.f / sum;
        } else {
        float sv[NSV];
#pragma unroll
        for (int u = 0; u < NSV; ++u) sv[u] = s[min(lane + 64 * u, a.L - 1)];
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < NSV; ++u) mx = fmaxf(mx, lane + 64 * u < a.L ? sv[u] : -INFINITY);
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < NSV; ++u) {
            const int l = lane + 64 * u;
            const float e = l < a.L ? __expf(sv[u] - mx) : 0.f;
            if (l < Lp) p[(size_t)wave * Lp + l] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        if (lane == 0) inv[wave] = 1.f / sum;
        }
    }
    __syncthreads();
    const float hsel = li < a.nhead ? 1.f : 0.f;
    const float* ph = p + (size_t)min(li, a.nhead - 1) * Lp;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = wave; ks < nks; ks += 64) {                     // this wavefront's k-steps ks, ks+16, ks+32, ks+48:
        float mv[4], pv[4];                                       // four loads in flight, then four MFMAs (sixteen: measured slower)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k2 = ks + 16 * u, l = 4 * k2 + kq;
            const bool live = k2 < nks;
            if (ks == wave) mv[u] = mv0[u];                       // uniform: the round requested in front of the softmax
            else mv[u] = pt_bload1(rm, (live && l < a.L) ? (unsigned)((((long)b * a.L + l) * a.D + c0 + li) * 4) : OOB);
            pv[u] = live ? ph[l] * hsel : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = mfma16(pv[u], mv[u], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave * 256 + (4 * kq + r) * 16 + li] = acc[r];
    __syncthreads();
    if (tid < 256) {
        const int h = tid >> 4, c = tid & 15;
        if (h < a.nhead) {
            float t = 0.f;
            for (int w = 0; w < 16; ++w) t += part[w * 256 + tid];
            a.ctx[((long)b * a.nhead + h) * a.D + c0 + c] = t * inv[h];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// box-regression head pieces (heads.py:119-141)
// ------------------------------------------------------------------------------------------------------------------
// att[p] = feat[:, p] . filt;  T[p][c] = att[p] * feat[c][p] (token-major), one workgroup per (32 positions, image)
__global__ __launch_bounds__(256) void k_reg_attend(const float* feat, const float* filt, float* T, int D, int HW) {
    extern __shared__ float sm[];                                // D x 33 tile + 32 attention values
    float* tile = sm;
    float* att = sm + (size_t)D * 33;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, p0 = blockIdx.x * 32, img = blockIdx.y;
    const float* src = feat + (long)img * D * HW;
    float part = 0.f;
    // 16 channels per thread and batch, clamped: all loads of a batch in flight (with the run-time bound as the only loop every
    // channel was its own round trip: 32 of them at D = 256, 13 us for a 330 KB map; round 4)
    const int px = min(p0 + tx, HW - 1);
    const bool pin = p0 + tx < HW;
    for (int cb = 0; cb < D; cb += 128) {
        float v[16], fv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = min(cb + ty + 8 * u, D - 1);
            v[u] = src[(long)c * HW + px];
            fv[u] = filt[c];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = cb + ty + 8 * u;
            if (c < D) {
                const float x = pin ? v[u] : 0.f;
                tile[c * 33 + tx] = x;
                part += x * fv[u];
            }
        }
    }
    __shared__ float red[8][33];
    red[ty][tx] = part;
    __syncthreads();
    if (ty == 0) {
        float s = 0.f;
        for (int i = 0; i < 8; ++i) s += red[i][tx];
        att[tx] = s;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i;
        if (p >= HW) continue;
        for (int c = tx; c < D; c += 32) T[((long)img * HW + p) * D + c] = att[i] * tile[c * 33 + i];
    }
}

// GroupNorm(1, C) + ReLU of the regression tower, fed by the split-K partial products of the 3x3 convolution:
//   k_gn_reduce: x = sum_z part[z] (fixed order), written once, + per-slice (sum, sum of squares) of one image
//   k_gn_apply:  mean / variance from the slice sums (double, fixed order), normalise + affine + ReLU in place
// grid (slices of 4096 elements, images); token-major (HW, C) blocks
constexpr int GN_SLICE = 1024;

__global__ __launch_bounds__(256) void k_gn_reduce(const float* __restrict__ part, int nz, long zstride,
                                                   float* __restrict__ x, float* __restrict__ stats, int n_per_img) {
    __shared__ float scratch[4];
    const int img = blockIdx.y, i0 = blockIdx.x * GN_SLICE;
    const long base = (long)img * n_per_img;
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int u = 0; u < GN_SLICE / 1024; ++u) {
        const int i = i0 + (u * 256 + threadIdx.x) * 4;
        if (i < n_per_img) {
            // the split partials in ONE batch of loads, fixed order (a run-time bound leaves fewer than 8 iterations -- the
            // feature head's 8 channel splits -- to a remainder loop of one dependent load per round trip; round 4)
            f32x4 pv[9];                                            // 8 channel splits (feature head) or 9 taps (tower): one batch
#pragma unroll
            for (int z = 0; z < 9; ++z) pv[z] = *reinterpret_cast<const f32x4*>(part + (long)min(z, nz - 1) * zstride + base + i);
            f32x4 v = pv[0];
#pragma unroll
            for (int z = 1; z < 9; ++z)
                if (z < nz) v += pv[z];
            for (int z = 9; z < nz; ++z) v += *reinterpret_cast<const f32x4*>(part + z * zstride + base + i);
            *reinterpret_cast<f32x4*>(x + base + i) = v;
            s += (v[0] + v[1]) + (v[2] + v[3]);
            q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
    }
    s = block_sum(s, scratch);
    q = block_sum(q, scratch);
    if (threadIdx.x == 0) {
        stats[((long)img * gridDim.x + blockIdx.x) * 2] = s;
        stats[((long)img * gridDim.x + blockIdx.x) * 2 + 1] = q;
    }
}

__global__ __launch_bounds__(256) void k_gn_apply(float* __restrict__ x, const float* __restrict__ stats,
                                                  const float* __restrict__ gam, const float* __restrict__ bet, int D,
                                                  int n_per_img) {
    const int img = blockIdx.y, i0 = blockIdx.x * GN_SLICE;
    double s = 0.0, q = 0.0;
    for (unsigned k = 0; k < gridDim.x; ++k) {
        s += (double)stats[((long)img * gridDim.x + k) * 2];
        q += (double)stats[((long)img * gridDim.x + k) * 2 + 1];
    }
    const double mean_d = s / n_per_img;
    const float mean = (float)mean_d, rstd = (float)(1.0 / sqrt(fmax(q / n_per_img - mean_d * mean_d, 0.0) + 1e-5));
    const long base = (long)img * n_per_img;
#pragma unroll
    for (int u = 0; u < GN_SLICE / 1024; ++u) {
        const int i = i0 + (u * 256 + threadIdx.x) * 4;
        if (i < n_per_img) {
            const int c = i % D;
            f32x4 v = *reinterpret_cast<const f32x4*>(x + base + i);
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gam + c), b4 = *reinterpret_cast<const f32x4*>(bet + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf((v[e] - mean) * rstd * g4[e] + b4[e], 0.f);
            *reinterpret_cast<f32x4*>(x + base + i) = v;
        }
    }
}

// ltrb[img][n][p] = exp(sum_z part[z][img*HW + p][n]) (heads.py:134)
__global__ __launch_bounds__(256) void k_reg_finish(const float* __restrict__ part, int nz, long zstride,
                                                    float* __restrict__ out, int M, int HW) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * 4) return;
    float v = part[idx];
    for (int z = 1; z < nz; ++z) v += part[z * zstride + idx];
    const int row = idx >> 2, n = idx & 3, img = row / HW;
    out[((long)img * 4 + n) * HW + (row - img * HW)] = expf(v);
}

// ------------------------------------------------------------------------------------------------------------------
// parameter pack layout (documented in include/pt_hot.h)
// ------------------------------------------------------------------------------------------------------------------
struct MhaOff { size_t w_in, b_in, w_out, b_out; };
struct EncOff { MhaOff sa; size_t w1, b1, w2, b2, n1g, n1b, n2g, n2b; };
struct DecOff { MhaOff sa, ca; size_t w1, b1, w2, b2, n1g, n1b, n2g, n2b, n3g, n3b; };
struct PackOff {
    EncOff enc[16];
    DecOff dec[16];
    size_t dng, dnb, bw1, bb1, bn1, bw2, bb2, bn2, bw3, bb3, fg, testtok, total;
};

PackOff pack_layout(int D, int ff, int n_enc, int n_dec) {
    PackOff o{};
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += n; return r; };
    auto mha = [&](MhaOff& m) {
        m.w_in = take((size_t)3 * D * D); m.b_in = take((size_t)3 * D); m.w_out = take((size_t)D * D); m.b_out = take(D);
    };
    for (int i = 0; i < n_enc; ++i) {
        EncOff& e = o.enc[i];
        mha(e.sa);
        e.w1 = take((size_t)ff * D); e.b1 = take(ff); e.w2 = take((size_t)D * ff); e.b2 = take(D);
        e.n1g = take(D); e.n1b = take(D); e.n2g = take(D); e.n2b = take(D);
    }
    for (int i = 0; i < n_dec; ++i) {
        DecOff& d = o.dec[i];
        mha(d.sa);
        mha(d.ca);
        d.w1 = take((size_t)ff * D); d.b1 = take(ff); d.w2 = take((size_t)D * ff); d.b2 = take(D);
        d.n1g = take(D); d.n1b = take(D); d.n2g = take(D); d.n2b = take(D); d.n3g = take(D); d.n3b = take(D);
    }
    o.dng = take(D); o.dnb = take(D);
    const int D4 = D / 4;
    o.bw1 = take((size_t)D4 * 4); o.bb1 = take(D4); o.bn1 = take((size_t)4 * D4);
    o.bw2 = take((size_t)D * D4); o.bb2 = take(D); o.bn2 = take((size_t)4 * D);
    o.bw3 = take((size_t)D * D); o.bb3 = take(D);
    o.fg = take(D); o.testtok = take(D);
    o.total = c;
    return o;
}

struct PrepOff { size_t wsa, bsa, mq, cq, wov, bov; };
struct PrepLayout { PrepOff dec[16]; size_t qk0; size_t total; };   // qk0: the first decoder layer's folded query (below), (nhead, D)
PrepLayout prep_layout(int D, int nhead, int n_dec) {
    PrepLayout o{};
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += pt_align_floats(n); return r; };
    for (int i = 0; i < n_dec; ++i) {
        PrepOff& p = o.dec[i];
        p.wsa = take((size_t)D * D); p.bsa = take(D); p.mq = take((size_t)nhead * D * D); p.cq = take((size_t)nhead * D);
        p.wov = take((size_t)D * nhead * D); p.bov = take(D);
    }
    o.qk0 = take((size_t)nhead * D);
    o.total = c;
    return o;
}

int dims_check(const pt_tomp_dims* d) {
    if (!d) return PT_ERR_NULL;
    if (d->d_model <= 0 || d->nhead <= 0 || d->dim_ff <= 0 || d->n_enc < 0 || d->n_dec < 0 || d->H <= 0 || d->W <= 0 ||
        d->max_res <= 0)
        return PT_ERR_SHAPE;
    if (d->d_model % d->nhead != 0) return PT_ERR_SHAPE;
    const int hd = d->d_model / d->nhead;
    if ((hd != 16 && hd != 32 && hd != 64) || d->d_model % 128 != 0 || d->d_model > 512 || d->dim_ff % 64 != 0 ||
        d->n_enc > 16 || d->n_dec > 16 || d->nhead > 16)
        return PT_ERR_UNSUPPORTED;
    return PT_OK;
}

struct WsCarve {
    size_t X, QKV, AO, Y, Hd, E1, E2, bnsc, bnsh, zero, a, qk, scores, ctx, P[2], P1, P2, hdn, total;
};

WsCarve ws_carve(const pt_tomp_dims* d, int B, int nf) {
    WsCarve w{};
    const size_t D = d->d_model, HW = (size_t)d->H * d->W, L = (nf + 1) * HW, rows = B * L;
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += pt_align_floats(n); return r; };
    w.X = take(rows * D); w.QKV = take(rows * 3 * D); w.AO = take(rows * D); w.Y = take(rows * D);
    w.Hd = take(rows * d->dim_ff);
    w.E1 = take((size_t)B * nf * HW * (D / 4)); w.E2 = take((size_t)B * nf * HW * D);
    w.bnsc = take(D); w.bnsh = take(D);
    w.zero = take(B * D); w.a = take(B * D); w.qk = take((size_t)B * d->nhead * D);
    w.scores = take((size_t)B * d->nhead * L); w.ctx = take((size_t)B * d->nhead * D);
    w.P[0] = take(B * D); w.P[1] = take(B * D); w.P1 = take(B * D); w.P2 = take(B * D); w.hdn = take((size_t)B * d->dim_ff);
    w.total = c;
    return w;
}

}  // namespace

// ==================================================================================================================
// C ABI
// ==================================================================================================================
extern "C" size_t pt_tomp_param_floats(const pt_tomp_dims* d) {
    if (dims_check(d)) return 0;
    return pack_layout(d->d_model, d->dim_ff, d->n_enc, d->n_dec).total;
}

extern "C" int pt_tomp_posenc_f32(float* pos, int H, int W, int d_model, int max_res, void* stream) {
    if (!pos) return PT_ERR_NULL;
    if (H <= 0 || W <= 0 || d_model <= 0 || d_model % 4 != 0 || max_res <= 0) return PT_ERR_SHAPE;
    const int total = H * W * d_model;
    const double factor = (double)max_res / (double)(d_model / 4);
    hipLaunchKernelGGL(k_tomp_posenc, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos, H, W, d_model,
                       factor);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" size_t pt_tomp_predict_ws_bytes(const pt_tomp_dims* d, int n_train, int n_seq, int parallel) {
    if (dims_check(d) || n_train <= 0 || n_seq <= 0) return 0;
    const int B = parallel ? 2 : n_seq;
    if (B > 8 || (parallel && n_seq != 1)) return 0;
    if ((size_t)d->nhead * ((size_t)(n_train + 1) * d->H * d->W + 4) > 11000) return 0;   // LDS of k_dec_ctx
    return ws_carve(d, B, n_train).total * sizeof(float);
}

namespace {
int tomp_linear_impl(const float* weight, const float* bias, const float* x, float* y, int B, int N, int K, int relu, void* stream,
                     PtRouteLog* log) {
    if (!weight || !x || !y) return PT_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0) return PT_ERR_SHAPE;
    GemvArgs a{};
    a.Wt = weight; a.bias = bias; a.N = N; a.K = K; a.x = x; a.relu = relu; a.B = B; a.out = y;
    return launch_gemv(a, (hipStream_t)stream, log);
}
}  // namespace

extern "C" int pt_tomp_linear_f32(const float* weight, const float* bias, const float* x, float* y, int B, int N, int K,
                                  int relu, void* stream) {
    return tomp_linear_impl(weight, bias, x, y, B, N, K, relu, stream, nullptr);
}

extern "C" size_t pt_tomp_prepared_floats(const pt_tomp_dims* d) {
    if (dims_check(d)) return 0;
    return std::max<size_t>(prep_layout(d->d_model, d->nhead, d->n_dec).total, 64);
}

extern "C" int pt_tomp_prepare_f32(const pt_tomp_dims* d, const float* params, float* prepared, void* stream) {
    if (!params || !prepared) return PT_ERR_NULL;
    int rc = dims_check(d);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int D = d->d_model, NH = d->nhead;
    const PackOff po = pack_layout(D, d->dim_ff, d->n_enc, d->n_dec);
    const PrepLayout pl = prep_layout(D, NH, d->n_dec);
    const float scale = 1.0f / sqrtf((float)(D / NH));
    for (int i = 0; i < d->n_dec; ++i) {
        const DecOff& dc = po.dec[i];
        const PrepOff& pp = pl.dec[i];
        const float *sa_w = params + dc.sa.w_in, *sa_b = params + dc.sa.b_in, *ca_w = params + dc.ca.w_in,
                    *ca_b = params + dc.ca.b_in;
        hipLaunchKernelGGL(k_prep_sa, dim3((D * D + 255) / 256), dim3(256), 0, st, params + dc.sa.w_out,
                           params + dc.sa.b_out, sa_w + (size_t)2 * D * D, sa_b + 2 * D, prepared + pp.wsa, prepared + pp.bsa, D);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_prep_mq, dim3((unsigned)(((long)NH * D * D + 255) / 256)), dim3(256), 0, st, ca_w, ca_b,
                           ca_w + (size_t)D * D, prepared + pp.mq, prepared + pp.cq, D, NH, scale);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_prep_ov, dim3((unsigned)(((long)NH * D * D + 255) / 256)), dim3(256), 0, st,
                           params + dc.ca.w_out, params + dc.ca.b_out, ca_w + (size_t)2 * D * D, ca_b + 2 * D,
                           prepared + pp.wov, prepared + pp.bov, D, NH);
        PT_CHECK_LAUNCH();
    }
    if (d->n_dec > 0) {
        // The decoder starts from zeros (transformer.py:224-238), so layer 0's self-attention output is its folded bias,
        // Pa = (Wo bv + bo), and its folded query Mq (LN1(Pa) + query_pos) + cq is a constant of the weights: one GEMV here
        // instead of two per frame (the same kernel, one row -> bit-identical to what the per-frame launches produced)
        const DecOff& dc = po.dec[0];
        const PrepOff& pp = pl.dec[0];
        GemvArgs v{};
        v.Wt = prepared + pp.mq; v.bias = prepared + pp.cq; v.N = NH * D; v.K = D; v.x = prepared + pp.bsa; v.xg = params + dc.n1g;
        v.xb = params + dc.n1b; v.xadd = params + po.fg; v.B = 1; v.out = prepared + pl.qk0;
        const int rc2 = launch_gemv(v, st);
        if (rc2) return rc2;
    }
    return PT_OK;
}

namespace {
// The encoder stack (transformer.py:172-180, post-norm) over `rows` = B * L token rows in X, shared by the ToMP and the TaMOs predictor:
// X is updated in place; QKV (rows, 3D), AO, Y (rows, D) and Hd (rows, ff) are scratch.
int run_encoder(const pt_tomp_dims* d, const PackOff& po, const float* P, const float* pos, const AttnArgs& at, int B, int L, int HW,
                float* X, float* QKV, float* AO, float* Y, float* Hd, hipStream_t st, PtRouteLog* log) {
    const int D = d->d_model, ff = d->dim_ff, rows = B * L;
    int rc;
    for (int i = 0; i < d->n_enc; ++i) {
        const EncOff& e = po.enc[i];
        GemmArgs g = gemm_args(X, D, rows, P + e.sa.w_in, rows, 3 * D, D, P + e.sa.b_in, QKV, 3 * D);
        g.pos = pos; g.pos_bytes = (unsigned)((long)HW * D * 4); g.pos_cols = 2 * D; g.L = L; g.HW = HW;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        if ((rc = launch_attn(at, B, st, log))) return rc;
        g = gemm_args(AO, D, rows, P + e.sa.w_out, rows, D, D, P + e.sa.b_out, Y, D);
        g.R = X;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        // (norm1 folded into the FFN's first product saved a launch per layer and lost: frame 0.885 -> 0.894 ms,
        // profiles/r06p_tomp_ln1_fold.txt)
        if ((rc = launch_ln_rows(Y, X, P + e.n1g, P + e.n1b, rows, D, st, log))) return rc;
        g = gemm_args(X, D, rows, P + e.w1, rows, ff, D, P + e.b1, Hd, ff);
        g.relu = 1;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        const long rD = (long)rows * D;
        if ((ff / 64) % 4 == 0 && rows >= 1024 && D % 64 == 0 && AO == QKV + 3 * (size_t)rD &&
            ln_rows_wide_ok(QKV, X, P + e.n2g, P + e.n2b, D)) {
            // The FFN's second product (K = dim_ff) runs as K-slices whose partial sums, bias included, meet in the LayerNorm that
            // follows (which then also adds the residual); two halves: ToMP frame 1.006 -> 0.996 ms (round 4, profiles/r04e_*).
            // round 6: four K-quarters on 128 x 64 tiles (k_gemm_ps: 256 workgroups x 16 stages, M tiles on x) into the four row blocks
            // QKV[0..2], AO -- all free here -- that meet, with the residual, in the LayerNorm
            g = gemm_args(Hd, ff, rows, P + e.w2, rows, D, ff, P + e.b2, QKV, D);
            g.ksteps = ff / 64 / 4; g.c_zstride = rD;
            if ((rc = launch_gemm(g, st, false, log))) return rc;
            if ((rc = launch_ln_rows(QKV, X, P + e.n2g, P + e.n2b, rows, D, st, log, QKV + rD, X, nullptr, nullptr, QKV + 2 * rD, AO))) return rc;
            continue;
        }
        g = gemm_args(Hd, ff, rows, P + e.w2, rows, D, ff, P + e.b2, Y, D);
        g.R = X;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        if ((rc = launch_ln_rows(Y, X, P + e.n2g, P + e.n2b, rows, D, st, log))) return rc;
    }
    return PT_OK;
}

// log == nullptr: the predictor.  Otherwise the same walk through the same dispatchers with nothing queued: every launch site notes its
// route instead (pt_tomp_predict_routes).  Host code only derives addresses from the pointers, it never reads through them.
int tomp_predict_impl(const pt_tomp_dims* d, const float* params, const float* prepared, const float* pos, const float* train_feat,
                      const float* test_feat, const float* train_label, const float* train_ltrb, int n_train, int n_seq, int parallel,
                      int num_gth_frames, float* filters, float* enc_feat, void* ws, size_t ws_bytes, void* stream, PtRouteLog* log) {
    if (!params || !prepared || !pos || !train_feat || !test_feat || !train_label || !train_ltrb || !filters || !enc_feat || !ws)
        return PT_ERR_NULL;
    int rc = dims_check(d);
    if (rc) return rc;
    if (n_train <= 0 || n_seq <= 0 || num_gth_frames < 0 || num_gth_frames > n_train) return PT_ERR_SHAPE;
    const int B = parallel ? 2 : n_seq;
    if (B > 8 || (parallel && n_seq != 1)) return PT_ERR_UNSUPPORTED;
    const int D = d->d_model, ff = d->dim_ff, NH = d->nhead, HD = D / NH, HW = d->H * d->W, Ltr = n_train * HW,
              L = Ltr + HW, rows = B * L, D4 = D / 4;
    if ((size_t)NH * (L + 4) > 11000) return PT_ERR_UNSUPPORTED;
    const WsCarve cv = ws_carve(d, B, n_train);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    const PackOff po = pack_layout(D, ff, d->n_enc, d->n_dec);
    const float* P = params;
    float *X = base + cv.X, *QKV = base + cv.QKV, *AO = base + cv.AO, *Y = base + cv.Y, *Hd = base + cv.Hd;

    bool dec0_const = false;                                       // decoder layer 0's first two GEMVs replaced by prepared constants
    // ---- tokens (filter_predictor.py:113-128)
    {
        TokArgs t{train_feat, test_feat, train_label, P + po.fg, P + po.testtok, X, n_train, n_seq, parallel ? 1 : 0, D,
                  HW, L, base + cv.zero, B * D, {nullptr, nullptr}, {nullptr, nullptr}, {0, 0}, B};
        if (d->n_dec > 0 && (D + 31) / 32 >= 3) {    // layer 0 of the decoder: state after self-attention, folded query
            const PrepLayout pl0 = prep_layout(D, NH, d->n_dec);
            t.cp_src[0] = prepared + pl0.dec[0].bsa; t.cp_dst[0] = base + cv.P1; t.cp_n[0] = D;
            t.cp_src[1] = prepared + pl0.qk0; t.cp_dst[1] = base + cv.qk; t.cp_n[1] = NH * D;
        }
        dec0_const = t.cp_src[0] != nullptr;
        PT_TOMP_LAUNCH(PT_TOMP_R_TOKENS, k_tomp_tokens, dim3((HW + 31) / 32, (D + 31) / 32, (n_train + 1) * B), dim3(256), 0, st, t);
        BoxArgs bx{train_ltrb, P + po.bw1, P + po.bb1, P + po.bn1, P + po.bn2, base + cv.E1, base + cv.bnsc,
                   base + cv.bnsh, n_train, n_seq, parallel ? 1 : 0, D, D4, HW};
        const long tot = (long)B * Ltr * D4;
        PT_TOMP_LAUNCH(PT_TOMP_R_BOX1, k_tomp_box1, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, bx);
        GemmArgs g = gemm_args(base + cv.E1, D4, (long)B * Ltr, P + po.bw2, B * Ltr, D, D4, P + po.bb2, base + cv.E2, D);
        g.scale = base + cv.bnsc; g.shift = base + cv.bnsh; g.relu = 1;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        g = gemm_args(base + cv.E2, D, (long)B * Ltr, P + po.bw3, B * Ltr, D, D, P + po.bb3, X, D);
        g.R = X; g.c_seg = Ltr; g.c_segstride = L;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
    }
    AttnArgs at{};
    at.qkv = QKV; at.qkv_bytes = (unsigned)((long)rows * 3 * D * 4); at.out = AO; at.L = L; at.D = D; at.nhead = NH;
    at.scale = 1.0f / sqrtf((float)HD);
    for (int b = 0; b < 8; ++b) at.mlo[b] = at.mhi[b] = 0;
    if (parallel) {                                               // filter_predictor.py:134-136: batch row 1 only
        at.mlo[1] = num_gth_frames * HW;
        at.mhi[1] = L - HW;
    }
    // ---- encoder (transformer.py:172-180), post-norm
    if ((rc = run_encoder(d, po, P, pos, at, B, L, HW, X, QKV, AO, Y, Hd, st, log))) return rc;
    // ---- decoder (transformer.py:224-238), one query per batch row; T = LayerNorm(pre) is applied by the consumers
    // (base + cv.zero was cleared by k_tomp_tokens)
    DecAttnArgs da{};
    da.mem = X; da.pos = pos; da.qk = base + cv.qk; da.scores = base + cv.scores; da.ctx = base + cv.ctx;
    da.B = B; da.L = L; da.D = D; da.nhead = NH; da.HW = HW;
    for (int b = 0; b < 8; ++b) { da.mlo[b] = at.mlo[b]; da.mhi[b] = at.mhi[b]; }
    const float* qpos = P + po.fg;                                 // query_embed_fg_decoder IS query_embed_fg (:35)
    const float* tpre = base + cv.zero;                            // pre-LayerNorm state entering the layer
    const float *tg = nullptr, *tb = nullptr;                      // its LayerNorm (none for the initial zeros)
    const PrepLayout pl = prep_layout(D, NH, d->n_dec);
    // layer 0's state after self-attention and its folded query: copied by k_tomp_tokens (no launch of their own) or two GEMVs
    if (log && d->n_dec > 0) pt_route_note(log, dec0_const ? PT_TOMP_R_DEC0_CONST : PT_TOMP_R_DEC0_LIVE);
    for (int i = 0; i < d->n_dec; ++i) {
        const DecOff& dc = po.dec[i];
        const PrepOff& pp = pl.dec[i];
        float *Pa = base + cv.P1, *Pb = base + cv.P2, *Pc = base + cv.P[i & 1];
        GemvArgs v{};
        // self-attention over one token (softmax of a single key is 1), folded: Pa = t + (Wo Wv) t + (Wo bv + bo)
        v.Wt = prepared + pp.wsa; v.bias = prepared + pp.bsa; v.N = D; v.K = D; v.x = tpre; v.xg = tg; v.xb = tb;
        v.res = tpre; v.rg = tg; v.rb = tb; v.B = B; v.out = Pa;
        if (!(i == 0 && dec0_const) && (rc = launch_gemv(v, st, log))) return rc;        // layer 0: written by k_tomp_tokens
        // cross-attention query folded onto the keys: qk[b][h] = Wk_h^T (Wq_h (LN1(Pa) + query_pos) + bq_h) / sqrt(HD)
        v = GemvArgs{};
        v.Wt = prepared + pp.mq; v.bias = prepared + pp.cq; v.N = NH * D; v.K = D; v.x = Pa; v.xg = P + dc.n1g;
        v.xb = P + dc.n1b; v.xadd = qpos; v.B = B; v.out = base + cv.qk;     // one query_pos row for all batch rows
        if (!(i == 0 && dec0_const) && (rc = launch_gemv(v, st, log))) return rc;
        PT_TOMP_LAUNCH(PT_TOMP_R_DEC_SCORES, k_dec_scores, dim3((L + 15) / 16, B), dim3(64), 0, st, da);
        PT_TOMP_LAUNCH(PT_TOMP_R_DEC_CTX, k_dec_ctx, dim3(D / 16, B), dim3(1024),
                       ((size_t)NH * ((L + 3) & ~3) + 16 + 16 * 256) * sizeof(float), st, da);
        // value projection + out_proj folded over the heads' attention-weighted memories, residual LN1(Pa)
        v = GemvArgs{};
        v.Wt = prepared + pp.wov; v.bias = prepared + pp.bov; v.N = D; v.K = NH * D; v.x = base + cv.ctx;
        v.res = Pa; v.rg = P + dc.n1g; v.rb = P + dc.n1b; v.B = B; v.out = Pb;
        if ((rc = launch_gemv(v, st, log))) return rc;
        // feed-forward on LN2(Pb)
        v = GemvArgs{};
        v.Wt = P + dc.w1; v.bias = P + dc.b1; v.N = ff; v.K = D; v.x = Pb; v.xg = P + dc.n2g;
        v.xb = P + dc.n2b; v.relu = 1; v.B = B; v.out = base + cv.hdn;
        if ((rc = launch_gemv(v, st, log))) return rc;
        v = GemvArgs{};
        v.Wt = P + dc.w2; v.bias = P + dc.b2; v.N = D; v.K = ff; v.x = base + cv.hdn;
        v.res = Pb; v.rg = P + dc.n2g; v.rb = P + dc.n2b; v.B = B; v.out = Pc;
        if ((rc = launch_gemv(v, st, log))) return rc;
        tpre = Pc; tg = P + dc.n3g; tb = P + dc.n3b;
    }
    // norm3 of the last layer, then the decoder's final norm (transformer.py:141-142)
    if (d->n_dec > 0 && ln_rows_wide_ok(tpre, filters, tg, tb, D)) {
        if ((rc = launch_ln_rows(tpre, filters, tg, tb, B, D, st, log, nullptr, nullptr, P + po.dng, P + po.dnb))) return rc;   // both norms, one launch
    } else {
        if (d->n_dec > 0) {
            if ((rc = launch_ln_rows(tpre, base + cv.a, tg, tb, B, D, st, log))) return rc;
            tpre = base + cv.a;
        }
        if ((rc = launch_ln_rows(tpre, filters, P + po.dng, P + po.dnb, B, D, st, log))) return rc;
    }
    PT_TOMP_LAUNCH(PT_TOMP_R_TO_NCHW, k_tokens_to_nchw, dim3((HW + 31) / 32, (D + 31) / 32, B), dim3(256), 0, st, X, enc_feat, B, L, D,
                   HW, Ltr);
    return PT_OK;
}
}  // namespace

extern "C" int pt_tomp_predict_f32(const pt_tomp_dims* d, const float* params, const float* prepared, const float* pos,
                                   const float* train_feat,
                                   const float* test_feat, const float* train_label, const float* train_ltrb,
                                   int n_train, int n_seq, int parallel, int num_gth_frames, float* filters,
                                   float* enc_feat, void* ws, size_t ws_bytes, void* stream) {
    return tomp_predict_impl(d, params, prepared, pos, train_feat, test_feat, train_label, train_ltrb, n_train, n_seq, parallel,
                             num_gth_frames, filters, enc_feat, ws, ws_bytes, stream, nullptr);
}

// ---- DenseBoxRegressor (heads.py:119-141) ------------------------------------------------------------------------
// reg pack: linear.weight (D,D), linear.bias (D), 4 x [conv weight (D, 9, D) tap-major, conv bias (D), GroupNorm weight
// (D), GroupNorm bias (D)], bbreg_layer weight (4, 9, D), bbreg_layer bias (4)
namespace {
struct RegOff { size_t lw, lb, cw[4], cb[4], gg[4], gb[4], fw, fb, total; };
RegOff reg_layout(int D) {
    RegOff o{};
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += n; return r; };
    o.lw = take((size_t)D * D); o.lb = take(D);
    for (int i = 0; i < 4; ++i) { o.cw[i] = take((size_t)D * 9 * D); o.cb[i] = take(D); o.gg[i] = take(D); o.gb[i] = take(D); }
    o.fw = take((size_t)4 * 9 * D); o.fb = take(4);
    o.total = c;
    return o;
}
}  // namespace

extern "C" size_t pt_tomp_bbreg_param_floats(int d_model) {
    return d_model > 0 && d_model % 32 == 0 ? reg_layout(d_model).total : 0;
}

namespace {
struct RegCarve { size_t fproj, T0, T1, part, stats, total; int slices; };
RegCarve reg_carve(int n, int D, int H, int W) {
    RegCarve c{};
    const size_t M = (size_t)n * H * W;
    size_t o = 0;
    auto take = [&](size_t k) { size_t r = o; o += pt_align_floats(k); return r; };
    c.slices = (int)(((size_t)H * W * D + GN_SLICE - 1) / GN_SLICE);
    c.fproj = take(D); c.T0 = take(M * D); c.T1 = take(M * D); c.part = take(9 * M * D);
    c.stats = take((size_t)2 * n * c.slices);
    c.total = o;
    return c;
}
}  // namespace

extern "C" size_t pt_tomp_bbreg_ws_bytes(int n, int d_model, int H, int W) {
    if (n <= 0 || d_model <= 0 || d_model % 64 != 0 || d_model > 512 || H <= 0 || W <= 0) return 0;
    return reg_carve(n, d_model, H, W).total * sizeof(float);
}

namespace {
// GroupNorm + ReLU of tower layer i applied by layer i + 1's loader (mfma_gemm.h: gn_*) instead of k_gn_apply: the fused loader takes
// at most GEMM_GN_MAX_SLICES slices per image, maps of at least one 32-row tile and 16-byte aligned affine parameters
bool reg_fuse_gn(int slices, int HW, int D, const float* gg, const float* gb) {
    return slices <= GEMM_GN_MAX_SLICES && HW >= 32 && ((uintptr_t)gg % 16) == 0 && ((uintptr_t)gb % 16) == 0 && (D % 4) == 0;
}

int tomp_bbreg_impl(const float* params, const float* feat, const float* filter, float* ltrb, int n, int d_model, int H, int W, void* ws,
                    size_t ws_bytes, void* stream, PtRouteLog* log) {
    if (!params || !feat || !filter || !ltrb || !ws) return PT_ERR_NULL;
    if (n <= 0 || d_model <= 0 || H <= 0 || W <= 0) return PT_ERR_SHAPE;
    if (d_model % 64 != 0 || d_model > 512) return PT_ERR_UNSUPPORTED;
    const int D = d_model, HW = H * W, M = n * HW;
    const RegCarve cv = reg_carve(n, D, H, W);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const RegOff ro = reg_layout(D);
    float* base = (float*)ws;
    float *fproj = base + cv.fproj, *part = base + cv.part, *stats = base + cv.stats;
    GemvArgs v{};
    v.Wt = params + ro.lw; v.bias = params + ro.lb; v.N = D; v.K = D; v.x = filter; v.B = 1; v.out = fproj;
    int rc = launch_gemv(v, st, log);
    if (rc) return rc;
    PT_TOMP_LAUNCH(PT_TOMP_R_REG_ATTEND, k_reg_attend, dim3((HW + 31) / 32, n), dim3(256), ((size_t)D * 33 + 32) * sizeof(float), st, feat,
                   fproj, base + cv.T0, D, HW);
    // each 3x3 convolution = 9 per-tap partial GEMMs (one K-slice of Cin per tap) reduced by the GroupNorm statistics pass
    float *src = base + cv.T0, *dst = base + cv.T1;
    const long zs = (long)M * D;
    // Round 4: GroupNorm + ReLU of layer i are applied by layer i + 1's loader (mfma_gemm.h: gn_*): the tower is conv -> reduce per
    // layer, the activations between two layers exist only as raw sums + slice statistics (k_gn_apply stays for shapes the fused
    // loader does not take: more than GEMM_GN_MAX_SLICES slices per image, maps smaller than a 32-row tile)
    const bool fuse_gn = reg_fuse_gn(cv.slices, HW, D, params + ro.gg[0], params + ro.gb[0]);
    auto with_gn = [&](GemmArgs& g, int prev) {
        if (!fuse_gn || prev < 0) return;
        g.gn_stats = stats; g.gn_slices = cv.slices; g.gn_count = HW * D;
        g.gn_gam = params + ro.gg[prev]; g.gn_bet = params + ro.gb[prev];
    };
    for (int i = 0; i < 4; ++i) {
        GemmArgs g = gemm_args(src, D, M, params + ro.cw[i], M, D, 9 * D, params + ro.cb[i], part, D);
        g.H = H; g.Wd = W; g.Cin = D; g.HW = HW; g.ksteps = D / 64; g.c_zstride = zs;
        with_gn(g, i - 1);
        if ((rc = launch_gemm(g, st, true, log))) return rc;
        PT_TOMP_LAUNCH(PT_TOMP_R_GN_REDUCE, k_gn_reduce, dim3(cv.slices, n), dim3(256), 0, st, part, 9, zs, dst, stats, HW * D);
        if (!fuse_gn) {
            PT_TOMP_LAUNCH(PT_TOMP_R_GN_APPLY, k_gn_apply, dim3(cv.slices, n), dim3(256), 0, st, dst, stats, params + ro.gg[i],
                           params + ro.gb[i], D, HW * D);
        }
        std::swap(src, dst);
    }
    GemmArgs g = gemm_args(src, D, M, params + ro.fw, M, 4, 9 * D, params + ro.fb, part, 4);
    g.H = H; g.Wd = W; g.Cin = D; g.HW = HW; g.ksteps = D / 64; g.c_zstride = (long)M * 4;
    with_gn(g, 3);
    if ((rc = launch_gemm(g, st, true, log))) return rc;
    PT_TOMP_LAUNCH(PT_TOMP_R_REG_FINISH, k_reg_finish, dim3((M * 4 + 255) / 256), dim3(256), 0, st, part, 9, (long)M * 4, ltrb, M, HW);
    return PT_OK;
}
}  // namespace

extern "C" int pt_tomp_bbreg_f32(const float* params, const float* feat, const float* filter, float* ltrb, int n,
                                 int d_model, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    return tomp_bbreg_impl(params, feat, filter, ltrb, n, d_model, H, W, ws, ws_bytes, stream, nullptr);
}

// ---- host-only route queries (include/pt_hot.h: pt_tomp_*_routes) -----------------------------------------------------------------
// Each walks the entry point's own code with a route log and stand-in addresses: 256-byte aligned, as the Python wrappers allocate, and
// far enough apart that no two buffers overlap; the pack / prepared / workspace offsets added to them are the real ones, so every
// alignment predicate sees what a call sees.  Nothing is launched and no device is touched.
namespace {
float* route_fake(int k) { return reinterpret_cast<float*>((uintptr_t)(k + 1) << 40); }

int route_finish(int rc, const PtRouteLog& log, int* routes, int cap, int* n_routes) {
    if (rc == PT_OK && log.n > cap) rc = PT_ERR_WORKSPACE;
    if (rc != PT_OK) {
        for (int i = 0; i < cap; ++i) routes[i] = 0;
        *n_routes = 0;
        return rc;
    }
    for (int i = log.n; i < cap; ++i) routes[i] = 0;
    *n_routes = log.n;
    return PT_OK;
}
}  // namespace

extern "C" int pt_tomp_predict_routes(const pt_tomp_dims* d, int n_train, int n_seq, int parallel, int* routes, int cap, int* n_routes) {
    if (!routes || !n_routes || !d) return PT_ERR_NULL;
    if (cap < 0) return PT_ERR_SHAPE;
    PtRouteLog log{routes, cap, 0};
    const int rc = tomp_predict_impl(d, route_fake(0), route_fake(1), route_fake(2), route_fake(3), route_fake(4), route_fake(5),
                                     route_fake(6), n_train, n_seq, parallel, 0, route_fake(7), route_fake(8), route_fake(9), ~(size_t)0,
                                     nullptr, &log);
    return route_finish(rc, log, routes, cap, n_routes);
}

extern "C" int pt_tomp_bbreg_routes(int n, int d_model, int H, int W, int* routes, int cap, int* n_routes) {
    if (!routes || !n_routes) return PT_ERR_NULL;
    if (cap < 0) return PT_ERR_SHAPE;
    PtRouteLog log{routes, cap, 0};
    const int rc = tomp_bbreg_impl(route_fake(0), route_fake(1), route_fake(2), route_fake(3), n, d_model, H, W, route_fake(4), ~(size_t)0,
                                   nullptr, &log);
    return route_finish(rc, log, routes, cap, n_routes);
}

extern "C" int pt_tomp_linear_routes(int B, int N, int K, int* routes, int cap, int* n_routes) {
    if (!routes || !n_routes) return PT_ERR_NULL;
    if (cap < 0) return PT_ERR_SHAPE;
    PtRouteLog log{routes, cap, 0};
    const int rc = tomp_linear_impl(route_fake(0), route_fake(1), route_fake(2), route_fake(3), B, N, K, 0, nullptr, &log);
    return route_finish(rc, log, routes, cap, n_routes);
}

// ==================================================================================================================
// TaMOs multi-object filter predictor (pt_tamos_*, include/pt_hot.h): GOTFilterPredictor.predict_filter /
// _predict_cls_bbreg_filters_parallel with label_enc 'gaussian' and box_enc 'ltrb_token' (filter_predictor.py:180-233,245-315) around
// Transformer.forward (transformer.py:90-96).  T object queries per batch row instead of ToMP's one:
//   tokens    k_tamos_tokens (features + sum_o label[o] E[o]), k_tamos_box1 + two products on launch_gemm for sum_o E[o] (.) MLP(ltrb[o]):
//             the object sum in front of the last Linear is ONE product with K = T D against diag(E[o]) W3 (folded by prepare)
//   encoder   run_encoder, as ToMP runs it
//   decoder   per layer: q|k|v projection of the T queries (launch_gemm, +query_pos on the q|k column tiles), k_tamos_self_attn,
//             out_proj + residual, LayerNorm; folded query (ToMP's Wk_h^T Wq_h / sqrt(d_h)) for all T nhead query rows in one product,
//             k_tamos_xattn over 64-key chunks of the memory -- scores and context on v_mfma_f32_16x16x4_f32, 16 query rows per
//             wavefront, nothing of size L on chip -- whose (max, sum, context) partials k_tamos_xmerge merges in chunk order, the
//             folded value + out_proj product (K = nhead D), LayerNorm, FFN, LayerNorm
// No atomics, every reduction in a fixed order: the same inputs give the same bits.  No host synchronisation.
// ==================================================================================================================
namespace {

struct TamosTokArgs {
    const float *train, *test, *label, *E;                       // label (nf, ns, T, HW), E (T, D)
    float* X;
    int nf, ns, dup, D, HW, L, T;
    float* zero; int nzero;                                      // the decoder's initial state, cleared on the side by the blocks of z = 0
};

// NCHW feature maps -> token-major rows; memory frames + sum_o label[o] * E[o] (filter_predictor.py:205-208), test frame as it is
__global__ __launch_bounds__(256) void k_tamos_tokens(TamosTokArgs a) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    if (blockIdx.z == 0) {
        const int nb = gridDim.x * gridDim.y * 256;
        for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < a.nzero; i += nb) a.zero[i] = 0.f;
    }
    const int B = a.dup ? 2 : a.ns;
    const int fr = blockIdx.z / B, b = blockIdx.z - fr * B, s = a.dup ? 0 : b;
    const bool train = fr < a.nf;
    const float* src = train ? a.train + ((long)(fr * a.ns + s) * a.D) * a.HW : a.test + ((long)s * a.D) * a.HW;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        tile[ty + 8 * i][tx] = (c < a.D && p < a.HW) ? src[(long)c * a.HW + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        if (p >= a.HW || c >= a.D) continue;
        float v = tile[tx][ty + 8 * i];
        if (train) {
            const float* lab = a.label + ((long)(fr * a.ns + s) * a.T) * a.HW + p;
            float e = 0.f;
            for (int o = 0; o < a.T; ++o) e += a.E[o * a.D + c] * lab[(long)o * a.HW];
            v += e;
        }
        a.X[((long)b * a.L + (long)fr * a.HW + p) * a.D + c] = v;
    }
}

struct TamosBoxArgs {
    const float *ltrb, *w1, *b1, *bn1;           // ltrb (nf, ns, T, 4, HW); bn1: [weight, bias, running_mean, running_var] of D4 floats
    float* E1;                                   // ((b, l, o), D4)
    int nf, ns, dup, D4, HW, T;
};

// first layer of the ltrb MLP for every object (Conv1d 4 -> D/4, eval-mode BatchNorm1d, ReLU; filter_predictor.py:6-17,214-217)
__global__ __launch_bounds__(256) void k_tamos_box1(TamosBoxArgs a) {
    const int B = a.dup ? 2 : a.ns, Ltr = a.nf * a.HW;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * Ltr * a.T * a.D4) return;
    const int j = (int)(idx % a.D4);
    const long row = idx / a.D4;
    const int o = (int)(row % a.T);
    const long bl = row / a.T;
    const int b = (int)(bl / Ltr), l = (int)(bl - (long)b * Ltr), fr = l / a.HW, p = l - fr * a.HW;
    const int s = a.dup ? 0 : b;
    const float* t = a.ltrb + (((long)(fr * a.ns + s) * a.T + o) * 4) * a.HW + p;
    float e = a.b1[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) e += a.w1[j * 4 + i] * t[(long)i * a.HW];
    e = (e - a.bn1[2 * a.D4 + j]) / sqrtf(a.bn1[3 * a.D4 + j] + 1e-5f) * a.bn1[j] + a.bn1[a.D4 + j];
    a.E1[idx] = fmaxf(e, 0.f);
}

// Weight-only part of the token build (pt_tamos_prepare_f32): W3E[n][o D + k] = E[o][n] W3[n][k], b3E[n] = b3[n] sum_o E[o][n], and the
// second BatchNorm as the scale / shift of the GEMM epilogue.  Plain loops: runs once per weight update.
__global__ void k_tamos_prep_box(const float* W3, const float* b3, const float* E, const float* bn2, float* W3E, float* b3E, float* sc2,
                                 float* sh2, int D, int T) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)D * T * D) return;
    const int n = (int)(idx / ((long)T * D)), o = (int)((idx / D) % T), k = (int)(idx % D);
    W3E[idx] = E[o * D + n] * W3[(long)n * D + k];
    if (o == 0 && k == 0) {
        float t = 0.f;
        for (int q = 0; q < T; ++q) t += E[q * D + n];
        b3E[n] = b3[n] * t;
        const float sc = bn2[n] / sqrtf(bn2[3 * D + n] + 1e-5f);
        sc2[n] = sc;
        sh2[n] = bn2[D + n] - bn2[2 * D + n] * sc;
    }
}

// Self-attention among the T <= 16 queries of one (head, batch row) (transformer.py:226-228): grid (nhead, B), thread (i, j) of 16 x 16
__global__ __launch_bounds__(256) void k_tamos_self_attn(const float* __restrict__ qkv, float* __restrict__ out, int T, int D, int HD,
                                                         float scale) {
    __shared__ float S[16][17], Pm[16][17];
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15, h = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * D;
    const bool in = i < T && j < T;
    float s = -INFINITY;
    if (in) {
        const float* q = qkv + ((long)b * T + i) * ld + h * HD;
        const float* k = qkv + ((long)b * T + j) * ld + D + h * HD;
        float acc = 0.f;
        for (int c = 0; c < HD; ++c) acc += (q[c] * scale) * k[c];
        s = acc;
    }
    S[i][j] = s;
    __syncthreads();
    float p = 0.f;
    if (in) {
        float m = -INFINITY, sum = 0.f;
        for (int jj = 0; jj < T; ++jj) m = fmaxf(m, S[i][jj]);
        for (int jj = 0; jj < T; ++jj) sum += expf(S[i][jj] - m);
        p = expf(s - m) / sum;
    }
    Pm[i][j] = p;
    __syncthreads();
    if (i < T) {
        for (int c = j; c < HD; c += 16) {
            float acc = 0.f;
            for (int jj = 0; jj < T; ++jj) acc += Pm[i][jj] * qkv[((long)b * T + jj) * ld + 2 * D + h * HD + c];
            out[((long)b * T + i) * D + h * HD + c] = acc;
        }
    }
}

struct XAttnArgs {
    const float *mem, *pos, *qk;                 // mem (B, L, D); pos (HW, D); qk (B, R, D), row r = t nhead + h: the folded queries
    float *part, *pm, *ps;                       // (B, nch, R16, D) context partials, (B, nch, R16) chunk maxima and sums
    int B, L, D, R, R16, HW, nch;
    int mlo[8], mhi[8];                          // keys [mlo[b], mhi[b]) of batch row b are padding
};

// Cross-attention of 16 query rows over one 64-key chunk of the memory (transformer.py:231-232 with pt_tomp's fold): one wavefront.
//   S^T[key][row] = (mem[key] + pos[key]) . qk[row]      4 tiles of 16 keys, D / 4 MFMAs each (A = memory rows, B = folded queries)
//   P^T = exp(S^T - chunk maximum of the row)            masked keys and keys past L: exp(-inf) = 0
//   O^T[c][row] += mem[key][c] P^T[key][row]             the score accumulator IS the B operand (k-slot kq of MFMA r <-> key 4 kq + r)
// The chunk's (maximum, sum, unnormalised context) go to global memory; k_tamos_xmerge joins the chunks.  DT = D / 16.
template <int DT>
__global__ __launch_bounds__(64) void k_tamos_xattn(XAttnArgs a) {
    const int lane = threadIdx.x, li = lane & 15, kq = lane >> 4;
    const int ch = blockIdx.x, rt = blockIdx.y, b = blockIdx.z, c0 = ch * 64;
    const __amdgpu_buffer_rsrc_t rm = pt_rsrc(a.mem, (unsigned)((long)a.B * a.L * a.D * 4));
    const __amdgpu_buffer_rsrc_t rp = pt_rsrc(a.pos, (unsigned)((long)a.HW * a.D * 4));
    const __amdgpu_buffer_rsrc_t rq = pt_rsrc(a.qk, (unsigned)((long)a.B * a.R * a.D * 4));
    const int row = rt * 16 + li;
    const int mlo = a.mlo[b], mhi = a.mhi[b];
    f32x4 qf[DT];
    {
        const unsigned oq = row < a.R ? (unsigned)((((long)b * a.R + row) * a.D + 4 * kq) * 4) : OOB;
#pragma unroll
        for (int v = 0; v < DT; ++v) qf[v] = pt_bload4(rq, oq == OOB ? OOB : oq + 64u * v);
    }
    f32x4 st[4];
    float mc = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        const int l = min(c0 + kt * 16 + li, a.L - 1);
        const unsigned om = (unsigned)((((long)b * a.L + l) * a.D + 4 * kq) * 4);
        const unsigned op = (unsigned)(((long)(l % a.HW) * a.D + 4 * kq) * 4);
        f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v0 = 0; v0 < DT; v0 += 4) {                     // 8 loads in flight, then 16 MFMAs
            f32x4 m[4], pp[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                m[u] = pt_bload4(rm, om + 64u * (v0 + u));
                pp[u] = pt_bload4(rp, op + 64u * (v0 + u));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) sc = mfma16(m[u][e] + pp[u][e], qf[v0 + u][e], sc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = c0 + kt * 16 + 4 * kq + r;
            if (key >= a.L || (key >= mlo && key < mhi)) sc[r] = -INFINITY;
            mc = fmaxf(mc, sc[r]);
        }
        st[kt] = sc;
    }
    mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    const float m_use = mc == -INFINITY ? 0.f : mc;              // a chunk of nothing but padding: every weight exp(-inf) = 0
    f32x4 ot[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) ot[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pe = expf(st[kt][r] - m_use);
            lsum += pe;
            const int key = min(c0 + kt * 16 + 4 * kq + r, a.L - 1);   // past L: weight 0 on a finite value
            const unsigned ov = (unsigned)((((long)b * a.L + key) * a.D + li) * 4);
            float vf[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d) vf[d] = pt_bload1(rm, ov + 64u * d);
#pragma unroll
            for (int d = 0; d < DT; ++d) ot[d] = mfma16(vf[d], pe, ot[d]);
        }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const long prow = ((long)b * a.nch + ch) * a.R16 + row;        // row < R16 = 16 gridDim.y
    if (kq == 0) {
        a.pm[prow] = mc;
        a.ps[prow] = lsum;
    }
#pragma unroll
    for (int d = 0; d < DT; ++d)                                    // rows 16 d + 4 kq + r of O^T = 4 consecutive channels
        *reinterpret_cast<f32x4*>(&a.part[prow * a.D + 16 * d + 4 * kq]) = ot[d];
}

// ctx[b][row] = sum_ch exp(m_ch - M) part[ch] / sum_ch exp(m_ch - M) s_ch, M = max_ch m_ch, chunks in ascending order: grid (R, B)
__global__ __launch_bounds__(256) void k_tamos_xmerge(const float* __restrict__ part, const float* __restrict__ pm,
                                                      const float* __restrict__ ps, float* __restrict__ ctx, int R, int R16, int D,
                                                      int nch) {
    const int row = blockIdx.x, b = blockIdx.y;
    const long base = (long)b * nch * R16 + row;
    float M = -INFINITY;
    for (int c = 0; c < nch; ++c) M = fmaxf(M, pm[base + (long)c * R16]);
    float den = 0.f;
    for (int c = 0; c < nch; ++c) den += ps[base + (long)c * R16] * expf(pm[base + (long)c * R16] - M);
    const float inv = 1.f / den;
    for (int k = threadIdx.x; k < D; k += 256) {
        float acc = 0.f;
        for (int c = 0; c < nch; ++c) acc += expf(pm[base + (long)c * R16] - M) * part[(base + (long)c * R16) * D + k];
        ctx[((long)b * R + row) * D + k] = acc * inv;
    }
}

// ---- layouts ----------------------------------------------------------------------------------------------------------------------
// parameter pack: pt_tomp's transformer and box_encoding tensors, then query_embed_fg.weight (T, D); no test-frame token
struct TamosPack { PackOff po; size_t E, total; };
TamosPack tamos_pack(const pt_tomp_dims* d, int T) {
    TamosPack t{};
    t.po = pack_layout(d->d_model, d->dim_ff, d->n_enc, d->n_dec);
    t.E = t.po.fg;                                               // pack_layout's last two entries (fg, testtok: D floats each) give way
    t.total = t.E + (size_t)T * d->d_model;
    return t;
}

struct TamosPrepOff { size_t mq, cq, wov, bov; };
struct TamosPrep { TamosPrepOff dec[16]; size_t w3e, b3e, sc2, sh2, total; };
TamosPrep tamos_prep(int D, int nhead, int n_dec, int T) {
    TamosPrep o{};
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += pt_align_floats(n); return r; };
    for (int i = 0; i < n_dec; ++i) {
        TamosPrepOff& p = o.dec[i];
        p.mq = take((size_t)nhead * D * D); p.cq = take((size_t)nhead * D); p.wov = take((size_t)D * nhead * D); p.bov = take(D);
    }
    o.w3e = take((size_t)D * T * D); o.b3e = take(D); o.sc2 = take(D); o.sh2 = take(D);
    o.total = c;
    return o;
}

constexpr int TAMOS_KCH = 64;                                    // keys per k_tamos_xattn chunk

struct TamosCarve { size_t X, QKV, AO, Y, Hd, E1, E2, tgt, sqkv, sao, y, t1, qk, part, pm, ps, ctx, t2, hdn, total; int nch, R, R16; };
TamosCarve tamos_carve(const pt_tomp_dims* d, int T, int B, int nf) {
    TamosCarve w{};
    const size_t D = d->d_model, HW = (size_t)d->H * d->W, L = (nf + 1) * HW, rows = B * L, BT = (size_t)B * T;
    w.nch = (int)((L + TAMOS_KCH - 1) / TAMOS_KCH);
    w.R = T * d->nhead;
    w.R16 = (w.R + 15) / 16 * 16;
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += pt_align_floats(n); return r; };
    w.X = take(rows * D); w.QKV = take(rows * 3 * D); w.AO = take(rows * D); w.Y = take(rows * D);
    w.Hd = take(rows * d->dim_ff);
    w.E1 = take((size_t)B * nf * HW * T * (D / 4)); w.E2 = take((size_t)B * nf * HW * T * D);
    w.tgt = take(BT * D); w.sqkv = take(BT * 3 * D); w.sao = take(BT * D); w.y = take(BT * D); w.t1 = take(BT * D);
    w.qk = take(BT * d->nhead * D);
    w.part = take((size_t)B * w.nch * w.R16 * D); w.pm = take((size_t)B * w.nch * w.R16); w.ps = take((size_t)B * w.nch * w.R16);
    w.ctx = take(BT * d->nhead * D); w.t2 = take(BT * D); w.hdn = take(BT * d->dim_ff);
    w.total = c;
    return w;
}

// PT_OK when pt_tamos_predict_* covers the call: pt_tomp's dims, 1 <= T <= 16, <= 8 batch rows, and every buffer a kernel addresses
// through a raw buffer descriptor (pt_rsrc: 32-bit byte offsets) under 4 GiB
int tamos_check(const pt_tomp_dims* d, int T, int n_train, int n_seq, int parallel) {
    int rc = dims_check(d);
    if (rc) return rc;
    if (n_train <= 0 || n_seq <= 0) return PT_ERR_SHAPE;
    if (T < 1 || T > 16) return PT_ERR_UNSUPPORTED;
    const int B = parallel ? 2 : n_seq;
    if (B > 8 || (parallel && n_seq != 1)) return PT_ERR_UNSUPPORTED;
    const size_t D = d->d_model, HW = (size_t)d->H * d->W, L = (size_t)(n_train + 1) * HW, rows = B * L;
    const size_t widest = std::max<size_t>(std::max<size_t>(3 * D, d->dim_ff), (size_t)T * D);
    const size_t nch = (L + TAMOS_KCH - 1) / TAMOS_KCH, R16 = ((size_t)T * d->nhead + 15) / 16 * 16;
    if (rows * widest * 4 >= 0xFFFFFFE0ull || (size_t)B * nch * R16 * D * 4 >= 0xFFFFFFE0ull || L > 0x7FFFFFFFull / 8) return PT_ERR_UNSUPPORTED;
    return PT_OK;
}

int xattn_route(int D) {
    return D == 128 ? PT_TAMOS_R_XATTN128 : D == 256 ? PT_TAMOS_R_XATTN256 : D == 384 ? PT_TAMOS_R_XATTN384 : PT_TAMOS_R_XATTN512;
}

int launch_xattn(const XAttnArgs& a, hipStream_t st, PtRouteLog* log) {
    const int route = xattn_route(a.D);
    if (log) {
        pt_route_note(log, route);
        return PT_OK;
    }
    const dim3 grid(a.nch, a.R16 / 16, a.B), block(64);
    switch (route) {
    case PT_TAMOS_R_XATTN128: hipLaunchKernelGGL((k_tamos_xattn<8>), grid, block, 0, st, a); break;
    case PT_TAMOS_R_XATTN256: hipLaunchKernelGGL((k_tamos_xattn<16>), grid, block, 0, st, a); break;
    case PT_TAMOS_R_XATTN384: hipLaunchKernelGGL((k_tamos_xattn<24>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_tamos_xattn<32>), grid, block, 0, st, a); break;
    }
    PT_CHECK_LAUNCH();
    return PT_OK;
}

int tamos_predict_impl(const pt_tomp_dims* d, int T, const float* params, const float* prepared, const float* pos, const float* train_feat,
                       const float* test_feat, const float* train_label, const float* train_ltrb, int n_train, int n_seq, int parallel,
                       int num_gth_frames, float* filters, float* enc_feat, void* ws, size_t ws_bytes, void* stream, PtRouteLog* log) {
    if (!d || !params || !prepared || !pos || !train_feat || !test_feat || !train_label || !train_ltrb || !filters || !enc_feat || !ws)
        return PT_ERR_NULL;
    int rc = tamos_check(d, T, n_train, n_seq, parallel);
    if (rc) return rc;
    if (num_gth_frames < 0 || num_gth_frames > n_train) return PT_ERR_SHAPE;
    const int B = parallel ? 2 : n_seq;
    const int D = d->d_model, ff = d->dim_ff, NH = d->nhead, HD = D / NH, HW = d->H * d->W, Ltr = n_train * HW, L = Ltr + HW, D4 = D / 4,
              BT = B * T;
    const TamosCarve cv = tamos_carve(d, T, B, n_train);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    const TamosPack tp = tamos_pack(d, T);
    const PackOff& po = tp.po;
    const TamosPrep pl = tamos_prep(D, NH, d->n_dec, T);
    const float* P = params;
    const float* E = P + tp.E;
    float *X = base + cv.X, *QKV = base + cv.QKV, *AO = base + cv.AO, *Y = base + cv.Y, *Hd = base + cv.Hd;

    // ---- tokens (filter_predictor.py:204-222)
    {
        TamosTokArgs t{train_feat, test_feat, train_label, E, X, n_train, n_seq, parallel ? 1 : 0, D, HW, L, T, base + cv.tgt, BT * D};
        PT_TOMP_LAUNCH(PT_TAMOS_R_TOKENS, k_tamos_tokens, dim3((HW + 31) / 32, (D + 31) / 32, (n_train + 1) * B), dim3(256), 0, st, t);
        TamosBoxArgs bx{train_ltrb, P + po.bw1, P + po.bb1, P + po.bn1, base + cv.E1, n_train, n_seq, parallel ? 1 : 0, D4, HW, T};
        const long tot = (long)B * Ltr * T * D4;
        PT_TOMP_LAUNCH(PT_TAMOS_R_BOX1, k_tamos_box1, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, bx);
        const int Mo = B * Ltr * T;                               // one row per (batch row, position, object)
        GemmArgs g = gemm_args(base + cv.E1, D4, Mo, P + po.bw2, Mo, D, D4, P + po.bb2, base + cv.E2, D);
        g.scale = prepared + pl.sc2; g.shift = prepared + pl.sh2; g.relu = 1;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        // the same buffer as (B Ltr) rows of T D: X += E2 (diag(E[o]) W3)^T + b3 sum_o E[o]
        g = gemm_args(base + cv.E2, (long)T * D, (long)B * Ltr, prepared + pl.w3e, B * Ltr, D, T * D, prepared + pl.b3e, X, D);
        g.R = X; g.c_seg = Ltr; g.c_segstride = L;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
    }
    AttnArgs at{};
    at.qkv = QKV; at.qkv_bytes = (unsigned)((long)B * L * 3 * D * 4); at.out = AO; at.L = L; at.D = D; at.nhead = NH;
    at.scale = 1.0f / sqrtf((float)HD);
    for (int b = 0; b < 8; ++b) at.mlo[b] = at.mhi[b] = 0;
    if (parallel) {                                               // filter_predictor.py:298-299: batch row 1 only
        at.mlo[1] = num_gth_frames * HW;
        at.mhi[1] = L - HW;
    }
    if ((rc = run_encoder(d, po, P, pos, at, B, L, HW, X, QKV, AO, Y, Hd, st, log))) return rc;

    // ---- decoder (transformer.py:224-238), T queries per batch row, post-norm; tgt starts as zeros (cleared by k_tamos_tokens)
    float *tgt = base + cv.tgt, *sqkv = base + cv.sqkv, *sao = base + cv.sao, *y = base + cv.y, *t1 = base + cv.t1, *t2 = base + cv.t2;
    XAttnArgs xa{};
    xa.mem = X; xa.pos = pos; xa.qk = base + cv.qk; xa.part = base + cv.part; xa.pm = base + cv.pm; xa.ps = base + cv.ps;
    xa.B = B; xa.L = L; xa.D = D; xa.R = cv.R; xa.R16 = cv.R16; xa.HW = HW; xa.nch = cv.nch;
    for (int b = 0; b < 8; ++b) { xa.mlo[b] = at.mlo[b]; xa.mhi[b] = at.mhi[b]; }
    auto with_qpos = [&](GemmArgs& g, int cols) {                  // A[r] + E[r % T] on the leading `cols` output columns
        g.pos = E; g.pos_bytes = (unsigned)((long)T * D * 4); g.pos_cols = cols; g.L = T; g.HW = T;
    };
    for (int i = 0; i < d->n_dec; ++i) {
        const DecOff& dc = po.dec[i];
        const TamosPrepOff& pp = pl.dec[i];
        // self-attention: q = k = tgt + query_pos, v = tgt
        GemmArgs g = gemm_args(tgt, D, BT, P + dc.sa.w_in, BT, 3 * D, D, P + dc.sa.b_in, sqkv, 3 * D);
        with_qpos(g, 2 * D);
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        PT_TOMP_LAUNCH(PT_TAMOS_R_SELF_ATTN, k_tamos_self_attn, dim3(NH, B), dim3(256), 0, st, sqkv, sao, T, D, HD, at.scale);
        g = gemm_args(sao, D, BT, P + dc.sa.w_out, BT, D, D, P + dc.sa.b_out, y, D);
        g.R = tgt;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        if ((rc = launch_ln_rows(y, t1, P + dc.n1g, P + dc.n1b, BT, D, st, log))) return rc;
        // cross-attention, query folded onto the keys: qk[b][t][h] = Wk_h^T (Wq_h (t1 + query_pos) + bq_h) / sqrt(HD)
        g = gemm_args(t1, D, BT, prepared + pp.mq, BT, NH * D, D, prepared + pp.cq, base + cv.qk, (long)NH * D);
        with_qpos(g, NH * D);
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        if ((rc = launch_xattn(xa, st, log))) return rc;
        PT_TOMP_LAUNCH(PT_TAMOS_R_XMERGE, k_tamos_xmerge, dim3(cv.R, B), dim3(256), 0, st, base + cv.part, base + cv.pm, base + cv.ps,
                       base + cv.ctx, cv.R, cv.R16, D, cv.nch);
        // value projection + out_proj folded over the heads' contexts, residual t1
        g = gemm_args(base + cv.ctx, (long)NH * D, BT, prepared + pp.wov, BT, D, NH * D, prepared + pp.bov, y, D);
        g.R = t1;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        if ((rc = launch_ln_rows(y, t2, P + dc.n2g, P + dc.n2b, BT, D, st, log))) return rc;
        g = gemm_args(t2, D, BT, P + dc.w1, BT, ff, D, P + dc.b1, base + cv.hdn, ff);
        g.relu = 1;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        g = gemm_args(base + cv.hdn, ff, BT, P + dc.w2, BT, D, ff, P + dc.b2, y, D);
        g.R = t2;
        if ((rc = launch_gemm(g, st, false, log))) return rc;
        if ((rc = launch_ln_rows(y, tgt, P + dc.n3g, P + dc.n3b, BT, D, st, log))) return rc;
    }
    // the decoder's final norm (transformer.py:140-141)
    if ((rc = launch_ln_rows(tgt, filters, P + po.dng, P + po.dnb, BT, D, st, log))) return rc;
    PT_TOMP_LAUNCH(PT_TOMP_R_TO_NCHW, k_tokens_to_nchw, dim3((HW + 31) / 32, (D + 31) / 32, B), dim3(256), 0, st, X, enc_feat, B, L, D,
                   HW, Ltr);
    return PT_OK;
}
}  // namespace

extern "C" size_t pt_tamos_param_floats(const pt_tomp_dims* d, int num_tokens) {
    if (dims_check(d) || num_tokens < 1 || num_tokens > 16) return 0;
    return tamos_pack(d, num_tokens).total;
}

extern "C" size_t pt_tamos_prepared_floats(const pt_tomp_dims* d, int num_tokens) {
    if (dims_check(d) || num_tokens < 1 || num_tokens > 16) return 0;
    return tamos_prep(d->d_model, d->nhead, d->n_dec, num_tokens).total;
}

extern "C" int pt_tamos_prepare_f32(const pt_tomp_dims* d, int num_tokens, const float* params, float* prepared, void* stream) {
    if (!d || !params || !prepared) return PT_ERR_NULL;
    int rc = dims_check(d);
    if (rc) return rc;
    if (num_tokens < 1 || num_tokens > 16) return PT_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int D = d->d_model, NH = d->nhead, T = num_tokens;
    const TamosPack tp = tamos_pack(d, T);
    const TamosPrep pl = tamos_prep(D, NH, d->n_dec, T);
    const float scale = 1.0f / sqrtf((float)(D / NH));
    for (int i = 0; i < d->n_dec; ++i) {
        const DecOff& dc = tp.po.dec[i];
        const TamosPrepOff& pp = pl.dec[i];
        const float *ca_w = params + dc.ca.w_in, *ca_b = params + dc.ca.b_in;
        hipLaunchKernelGGL(k_prep_mq, dim3((unsigned)(((long)NH * D * D + 255) / 256)), dim3(256), 0, st, ca_w, ca_b, ca_w + (size_t)D * D,
                           prepared + pp.mq, prepared + pp.cq, D, NH, scale);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_prep_ov, dim3((unsigned)(((long)NH * D * D + 255) / 256)), dim3(256), 0, st, params + dc.ca.w_out,
                           params + dc.ca.b_out, ca_w + (size_t)2 * D * D, ca_b + 2 * D, prepared + pp.wov, prepared + pp.bov, D, NH);
        PT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_tamos_prep_box, dim3((unsigned)(((long)D * T * D + 255) / 256)), dim3(256), 0, st, params + tp.po.bw3,
                       params + tp.po.bb3, params + tp.E, params + tp.po.bn2, prepared + pl.w3e, prepared + pl.b3e, prepared + pl.sc2,
                       prepared + pl.sh2, D, T);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" size_t pt_tamos_predict_ws_bytes(const pt_tomp_dims* d, int num_tokens, int n_train, int n_seq, int parallel) {
    if (!d || tamos_check(d, num_tokens, n_train, n_seq, parallel)) return 0;
    return tamos_carve(d, num_tokens, parallel ? 2 : n_seq, n_train).total * sizeof(float);
}

extern "C" int pt_tamos_predict_f32(const pt_tomp_dims* d, int num_tokens, const float* params, const float* prepared, const float* pos,
                                    const float* train_feat, const float* test_feat, const float* train_label, const float* train_ltrb,
                                    int n_train, int n_seq, int parallel, int num_gth_frames, float* filters, float* enc_feat, void* ws,
                                    size_t ws_bytes, void* stream) {
    return tamos_predict_impl(d, num_tokens, params, prepared, pos, train_feat, test_feat, train_label, train_ltrb, n_train, n_seq, parallel,
                              num_gth_frames, filters, enc_feat, ws, ws_bytes, stream, nullptr);
}

extern "C" int pt_tamos_predict_routes(const pt_tomp_dims* d, int num_tokens, int n_train, int n_seq, int parallel, int* routes, int cap,
                                       int* n_routes) {
    if (!routes || !n_routes || !d) return PT_ERR_NULL;
    if (cap < 0) return PT_ERR_SHAPE;
    PtRouteLog log{routes, cap, 0};
    const int rc = tamos_predict_impl(d, num_tokens, route_fake(0), route_fake(1), route_fake(2), route_fake(3), route_fake(4),
                                      route_fake(5), route_fake(6), n_train, n_seq, parallel, 0, route_fake(7), route_fake(8),
                                      route_fake(9), ~(size_t)0, nullptr, &log);
    return route_finish(rc, log, routes, cap, n_routes);
}

// ==================================================================================================================
// Classification-feature head: `residual_bottleneck(num_blocks=0, final_conv=True,
// l2norm=True)` = Conv2d(Cin, Cout, 3, padding=1, bias=False) + InstanceL2Norm (ltr/models/target_classifier/
// features.py:49-73, ltr/models/layers/normalization.py:15-20).  DiMP-50 runs it once per frame (1024 -> 512), ToMP on
// the test frame and on both memory frames every frame (1024 -> 256, tomp.py:289-290).
//   NCHW -> token-major transpose, 9 per-tap partial GEMMs on the MFMA kernel above (split-K), fixed-order reduction
//   with the per-image sum of squares, normalise + transpose back to NCHW.
// ==================================================================================================================
namespace {

__global__ __launch_bounds__(256) void k_nchw_to_tokens(const float* in, float* X, int C, int HW) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, img = blockIdx.z;
    const float* src = in + (long)img * C * HW;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        tile[ty + 8 * i][tx] = (c < C && p < HW) ? src[(long)c * HW + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        if (p < HW && c < C) X[((long)img * HW + p) * C + c] = tile[tx][ty + 8 * i];
    }
}

// out[img][c][p] = x[img*HW + p][c] * scale * sqrt(C*HW / (sum x^2 + eps)); the per-image sum of squares comes from the
// slice partials of k_gn_reduce (double, fixed order)
__global__ __launch_bounds__(256) void k_head_finish(const float* X, const float* stats, int slices, float* out, int C,
                                                     int HW, float scale, float eps) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, img = blockIdx.z;
    __shared__ double sh[256];
    double q = 0.0;                                                 // fixed order: thread t sums slices t, t+256, ...; then a tree
    for (int k = threadIdx.x; k < slices; k += 256) q += (double)stats[((long)img * slices + k) * 2 + 1];
    sh[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const float f = scale * (float)sqrt((double)C * HW / (sh[0] + (double)eps));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (p < HW && c < C) ? X[((long)img * HW + p) * C + c] * f : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        if (c < C && p < HW) out[((long)img * C + c) * HW + p] = tile[tx][ty + 8 * i];
    }
}

// out = y * scale * sqrt(C*HW / (sum y^2 + eps)) for maps that already are (n, C, H, W)
// slot_dyn (graph-replayed one-call frame, frame_full.hip): the output lands slot_stride * *slot_dyn floats further -- the memory slot of
// this frame is read from a device descriptor instead of being baked into the captured launch
__global__ __launch_bounds__(256) void k_head_scale(const float* __restrict__ Y, const float* __restrict__ stats, int slices,
                                                    float* __restrict__ out, int C, int HW, float scale, float eps,
                                                    const int* __restrict__ slot_dyn, long slot_stride) {
    __shared__ double sh[256];
    if (slot_dyn) out += (long)(*slot_dyn) * slot_stride;
    const int img = blockIdx.y;
    double q = 0.0;                                                 // fixed order: thread t sums slices t, t+256, ...; then a tree
    for (int k = threadIdx.x; k < slices; k += 256) q += (double)stats[((long)img * slices + k) * 2 + 1];
    sh[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const float f = scale * (float)sqrt((double)C * HW / (sh[0] + (double)eps));
    const long base = (long)img * C * HW, i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i < (long)C * HW) {
        f32x4 v = *reinterpret_cast<const f32x4*>(Y + base + i);
        *reinterpret_cast<f32x4*>(out + base + i) = v * f;
    }
}

struct HeadCarve { size_t X, part, Y, stats, total; int slices; };
HeadCarve head_carve(int n, int Cin, int Cout, int H, int W) {
    HeadCarve c{};
    const size_t M = (size_t)n * H * W;
    size_t o = 0;
    auto take = [&](size_t k) { size_t r = o; o += pt_align_floats(k); return r; };
    c.slices = (int)(((size_t)H * W * Cout + GN_SLICE - 1) / GN_SLICE);
    c.X = take(M * Cin); c.part = take(9 * M * Cout); c.Y = take(M * Cout); c.stats = take((size_t)2 * n * c.slices);
    c.total = o;
    return c;
}

int head_check(int n, int Cin, int Cout, int H, int W) {
    if (n <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return PT_ERR_SHAPE;
    if (Cin % 64 != 0 || Cout % 4 != 0 || (size_t)n * H * W * Cin * 4 > 0xFFFFFFE0ull ||
        (size_t)Cout * 9 * Cin * 4 > 0xFFFFFFE0ull)
        return PT_ERR_UNSUPPORTED;
    return PT_OK;
}

}  // namespace

extern "C" size_t pt_clf_head_ws_bytes(int n, int Cin, int Cout, int H, int W) {
    if (head_check(n, Cin, Cout, H, W)) return 0;
    return head_carve(n, Cin, Cout, H, W).total * sizeof(float);
}

extern "C" int pt_clf_head_f32(const float* feat, const float* weight_tap_major, float* out, int n, int Cin, int Cout,
                               int H, int W, float norm_scale, float eps, void* ws, size_t ws_bytes, void* stream) {
    return pt_clf_head_impl(feat, weight_tap_major, out, n, Cin, Cout, H, W, norm_scale, eps, ws, ws_bytes, stream, nullptr, 0);
}

// slot_dyn != nullptr (one frame, banded-correlation route only): `out` is the BASE of the sample memory and the slot comes from the device
int pt_clf_head_impl(const float* feat, const float* weight_tap_major, float* out, int n, int Cin, int Cout, int H, int W,
                     float norm_scale, float eps, void* ws, size_t ws_bytes, void* stream, const int* slot_dyn, long slot_stride) {
    if (!feat || !weight_tap_major || !out || !ws) return PT_ERR_NULL;
    int rc = head_check(n, Cin, Cout, H, W);
    if (rc) return rc;
    const HeadCarve cv = head_carve(n, Cin, Cout, H, W);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    const int HW = H * W, M = n * HW;
    // The maps stay (n, C, H, W) end to end when the banded correlation kernel covers the shape (csrc/mf_kernels.hip: 16 output
    // channels per workgroup, weights transposed on their way into LDS, channel splits summed here): no token transposes,
    // 3 launches instead of 4, and the MFMA loop built on the issue model (66.6 -> 4x us on the DiMP-50 head).
    // (one frame of DiMP-50: 256 workgroups x 16 chunks; ToMP's three frames would need 32 chunk times and stay on the
    // GEMM path below, 76 vs 90 us)
    const int ks = ((Cout * HW) % 4 == 0 && ((uintptr_t)out % 16) == 0 && pt_mf_corr_tm_cost(n, Cout, Cin, H, W) <= 22)
                       ? pt_mf_corr_tm_splits(n, Cout, Cin, H, W) : 0;
    if (slot_dyn && !(ks > 0 && ks <= 9 && n == 1)) return PT_ERR_UNSUPPORTED;
    if (ks > 0 && ks <= 9) {
        if ((rc = pt_launch_mf_corr_tm(feat, (long)Cin * HW, weight_tap_major, base + cv.part, n, Cout, Cin, H, W, ks, st)) == PT_OK) {
            hipLaunchKernelGGL(k_gn_reduce, dim3(cv.slices, n), dim3(256), 0, st, base + cv.part, ks, (long)M * Cout, base + cv.Y,
                               base + cv.stats, HW * Cout);
            PT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_head_scale, dim3((Cout * HW / 4 + 255) / 256, n), dim3(256), 0, st, base + cv.Y, base + cv.stats,
                               cv.slices, out, Cout, HW, norm_scale, eps, slot_dyn, slot_stride);
            PT_CHECK_LAUNCH();
            return PT_OK;
        }
    }
    if (slot_dyn) return PT_ERR_UNSUPPORTED;                           // the token route writes through k_head_finish: static slot only
    hipLaunchKernelGGL(k_nchw_to_tokens, dim3((HW + 31) / 32, (Cin + 31) / 32, n), dim3(256), 0, st, feat, base + cv.X, Cin,
                       HW);
    PT_CHECK_LAUNCH();
    const long zs = (long)M * Cout;
    GemmArgs g = gemm_args(base + cv.X, Cin, M, weight_tap_major, M, Cout, 9 * Cin, nullptr, base + cv.part, Cout);
    g.H = H; g.Wd = W; g.Cin = Cin; g.HW = HW; g.ksteps = Cin / 64; g.c_zstride = zs;
    if ((rc = launch_gemm(g, st, true))) return rc;
    hipLaunchKernelGGL(k_gn_reduce, dim3(cv.slices, n), dim3(256), 0, st, base + cv.part, 9, zs, base + cv.Y,
                       base + cv.stats, HW * Cout);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_finish, dim3((HW + 31) / 32, (Cout + 31) / 32, n), dim3(256), 0, st, base + cv.Y,
                       base + cv.stats, cv.slices, out, Cout, HW, norm_scale, eps);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// ==================================================================================================================
// Feature head at stride 1 or 2 (pt_feat_head_f32): Conv2d(Cin, Cout, 3, stride, padding 1, no bias) -> InstanceL2Norm.
//   stride 1 IS the classification-feature head above (pt_clf_head_impl, same bits).
//   stride 2 (the RTS classifier head, 1024 x 30 x 52 -> 512 x 15 x 26): the token route of that head with a strided gather --
//   NCHW -> tokens (k_nchw_to_tokens), one partial product per tap (k_gemm_s2, grid.z = 9), the partials summed in fixed order with the
//   per-image sum of squares (k_gn_reduce), normalise + transpose back to NCHW (k_head_finish).  No atomics.
// ==================================================================================================================
namespace {

// k_gemm<32, 32, 1> (mfma_gemm.h: gemm_tile, MODE 1) with input and output maps of different size: row r of the product is output token
// (img, oy, ox) = (r / g.HW, (r % g.HW) / Wo, r % Wo) and tap (ky, kx) gathers input token (2 oy + ky - 1, 2 ox + kx - 1) of the
// g.H x g.Wd map of the SAME image (rows of A: img * g.H * g.Wd + y * g.Wd + x); a tap outside that map is an out-of-range buffer
// offset, which the hardware answers with zeros.  g.HW = Ho * Wo, g.M = n * Ho * Wo.  Same LDS layout, fragment permutation, register
// ring and epilogue as gemm_tile; blockIdx.z owns g.ksteps = Cin / 64 K-steps, i.e. one tap.
__global__ __launch_bounds__(256) void k_gemm_s2(GemmArgs g, int Wo) {
    constexpr int BM = 32, BN = 32, BK = 64, LS = BK + 4, RP = 1024 / BK, AL = BM / RP, BL = BN / RP, PD = 2;
    __shared__ __attribute__((aligned(16))) float As[2][BM * LS];
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN, bz = blockIdx.z;
    const int lrow = tid / (BK / 4), lc4 = (tid % (BK / 4)) * 4;
    const __amdgpu_buffer_rsrc_t rsA = pt_rsrc(g.A, g.a_bytes), rsW = pt_rsrc(g.Wt, g.w_bytes);
    unsigned aoff[AL], woff[BL];
    int py[AL], px[AL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int row = m0 + lrow + RP * i;
        const bool ok = row < g.M;
        const int img = row / g.HW, p = row - img * g.HW, oy = p / Wo;
        py[i] = ok ? 2 * oy : -4;                                        // -4: every tap falls outside the map
        px[i] = 2 * (p - oy * Wo);
        aoff[i] = (unsigned)(((long)img * g.H * g.Wd * g.lda + lc4) * 4);
    }
#pragma unroll
    for (int i = 0; i < BL; ++i) {
        const int n = n0 + lrow + RP * i;
        woff[i] = n < g.N ? (unsigned)(((long)n * g.K + lc4) * 4) : OOB;
    }
    const int nkt = g.K / BK;                                            // K = 9 Cin, Cin % 64 == 0
    f32x4 ra[PD][AL], rb[PD][BL];
    auto fetch = [&](int kb, int sl) {                                   // a step past the end re-fetches the last one (never consumed)
        const int kc = min(kb, nkt - 1);
        const int k0 = kc * BK, tap = k0 / g.Cin, c0 = k0 - tap * g.Cin;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int y = py[i] + dy, x = px[i] + dx;
            const bool in = y >= 0 && y < g.H && x >= 0 && x < g.Wd;
            ra[sl][i] = pt_bload4(rsA, in ? aoff[i] + (unsigned)(((long)(y * g.Wd + x) * g.lda + c0) * 4) : OOB);
        }
#pragma unroll
        for (int i = 0; i < BL; ++i)
            rb[sl][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW, woff[i], (unsigned)kc * (BK * 4u), 0));
    };
    auto stash = [&](int sl, int buf) {
#pragma unroll
        for (int i = 0; i < AL; ++i) *reinterpret_cast<f32x4*>(&As[buf][(lrow + RP * i) * LS + lc4]) = ra[sl][i];
#pragma unroll
        for (int i = 0; i < BL; ++i) *reinterpret_cast<f32x4*>(&Bs[buf][(lrow + RP * i) * LS + lc4]) = rb[sl][i];
    };
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const int qoff = ((lane >> 4) & 1) * 2 + (lane >> 5);                // conflict-free fragment maps of gemm_tile
    const int aso = (wm * 16 + gemm_prow(lane & 15)) * LS + qoff * 4, bso = (wn * 16 + gemm_prow(lane & 15)) * LS + qoff * 4;
    const int kb0 = bz * g.ksteps, nk = min(nkt, kb0 + g.ksteps);
#pragma unroll
    for (int sl = 0; sl < PD; ++sl) fetch(kb0 + sl, sl);
    stash(0, 0);
    __syncthreads();
    for (int t0 = kb0; t0 < nk; t0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            const int kb = t0 + u, buf = u & 1;
            fetch(kb + PD, u);                                           // slot u (step kb) already sits in LDS[buf]
            if (kb < nk) {                                               // workgroup-uniform
                f32x4 fa[BK / 16], fb[BK / 16];
#pragma unroll
                for (int hh = 0; hh < BK / 16; ++hh) {
                    fa[hh] = *reinterpret_cast<const f32x4*>(&As[buf][aso + hh * 16]);
                    fb[hh] = *reinterpret_cast<const f32x4*>(&Bs[buf][bso + hh * 16]);
                }
#pragma unroll
                for (int hh = 0; hh < BK / 16; ++hh)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[0][0] = mfma16(fa[hh][j], fb[hh][j], acc[0][0]);
            }
            stash((u + 1) % PD, buf ^ 1);                                // step kb+1 (past the end: never read)
            __syncthreads();
        }
    }
    gemm_store<1, 1>(g, acc, m0 + wm * 16, n0 + wn * 16, lane, bz);
}

struct FeatHeadCarve { size_t X, part, Y, stats, total; int slices, Ho, Wo; };
FeatHeadCarve feat_head_carve(int n, int Cin, int Cout, int H, int W) {
    FeatHeadCarve c{};
    c.Ho = (H - 1) / 2 + 1; c.Wo = (W - 1) / 2 + 1;
    const size_t Mo = (size_t)n * c.Ho * c.Wo;
    size_t o = 0;
    auto take = [&](size_t k) { size_t r = o; o += pt_align_floats(k); return r; };
    c.slices = (int)(((size_t)c.Ho * c.Wo * Cout + GN_SLICE - 1) / GN_SLICE);
    c.X = take((size_t)n * H * W * Cin); c.part = take(9 * Mo * Cout); c.Y = take(Mo * Cout); c.stats = take((size_t)2 * n * c.slices);
    c.total = o;
    return c;
}

// head_check's shapes and limits; stride 2 also keeps the nine partial products inside the epilogue's 32-bit byte offsets
int feat_head_check(int n, int Cin, int Cout, int H, int W, int stride) {
    const int rc = head_check(n, Cin, Cout, H, W);
    if (rc) return rc;
    if (stride == 1) return PT_OK;
    if (stride != 2) return PT_ERR_UNSUPPORTED;
    const size_t Mo = (size_t)n * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return 9 * Mo * Cout * 4 >= 0xFFFFFFE0ull ? PT_ERR_UNSUPPORTED : PT_OK;
}

}  // namespace

extern "C" size_t pt_feat_head_ws_bytes(int n, int Cin, int Cout, int H, int W, int stride) {
    if (feat_head_check(n, Cin, Cout, H, W, stride)) return 0;
    if (stride == 1) return pt_clf_head_ws_bytes(n, Cin, Cout, H, W);
    return feat_head_carve(n, Cin, Cout, H, W).total * sizeof(float);
}

extern "C" int pt_feat_head_f32(const float* feat, const float* weight_tap_major, float* out, int n, int Cin, int Cout, int H, int W,
                                int stride, float norm_scale, float eps, void* ws, size_t ws_bytes, void* stream) {
    if (!feat || !weight_tap_major || !out || !ws) return PT_ERR_NULL;
    const int rc = feat_head_check(n, Cin, Cout, H, W, stride);
    if (rc) return rc;
    if (stride == 1)
        return pt_clf_head_impl(feat, weight_tap_major, out, n, Cin, Cout, H, W, norm_scale, eps, ws, ws_bytes, stream, nullptr, 0);
    const FeatHeadCarve cv = feat_head_carve(n, Cin, Cout, H, W);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    const int HW = H * W, HWo = cv.Ho * cv.Wo, Mo = n * HWo;
    hipLaunchKernelGGL(k_nchw_to_tokens, dim3((HW + 31) / 32, (Cin + 31) / 32, n), dim3(256), 0, st, feat, base + cv.X, Cin, HW);
    PT_CHECK_LAUNCH();
    const long zs = (long)Mo * Cout;
    GemmArgs g = gemm_args(base + cv.X, Cin, (long)n * HW, weight_tap_major, Mo, Cout, 9 * Cin, nullptr, base + cv.part, Cout);
    g.H = H; g.Wd = W; g.Cin = Cin; g.HW = HWo; g.ksteps = Cin / 64; g.c_zstride = zs;
    hipLaunchKernelGGL(k_gemm_s2, dim3((Cout + 31) / 32, (Mo + 31) / 32, 9), dim3(256), 0, st, g, cv.Wo);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gn_reduce, dim3(cv.slices, n), dim3(256), 0, st, base + cv.part, 9, zs, base + cv.Y, base + cv.stats, HWo * Cout);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_finish, dim3((HWo + 31) / 32, (Cout + 31) / 32, n), dim3(256), 0, st, base + cv.Y, base + cv.stats, cv.slices,
                       out, Cout, HWo, norm_scale, eps);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// ==================================================================================================================
// TaMOs heads (pt_tamos_bbreg_*, pt_fpn2_*, include/pt_hot.h): the two-level FPN of heads.py:144-162 and the multi-object
// DenseBoxRegressor of heads.py:119-141 on the FPN map (T attended copies of a 48 x 72 map: 34 560 token rows per tower layer).
//   k_conv3<MODE>   direct 3x3 token convolution, stride 1, padding 1: one workgroup owns a 128 x 64 output tile of ONE image and walks
//                   K = 9 Cin itself (no per-tap partial buffer, no split-K, no atomics); the loader applies, per MODE, nothing / a
//                   per-row scalar (attention (.) feature) / the previous layer's GroupNorm + affine + ReLU / the FPN's top-down
//                   "nearest resize + add"; the zero padding is applied AFTER that transform (a halo pixel contributes 0); the epilogue
//                   adds the bias, writes token-major or NCHW and leaves the tile's (sum, sum of squares) in a fixed slot
//   k_conv3_gn_finish   the slots of an image summed in slot order in double -> (mean, rstd) per image, which the next loader reads
//   k_reg_out       the 4-channel bbreg_layer + exp on the last GroupNorm'ed map, one wavefront per run of 8 pixels
// ==================================================================================================================
namespace {

constexpr int C3_BM = 128, C3_BN = 64;
enum { C3_PLAIN = 0, C3_ROWSCALE = 1, C3_GN = 2, C3_UPADD = 3 };

struct Conv3Args {
    const float* A; unsigned a_bytes; int a_div;      // token-major (source image, HW, Cin); grid image z reads source image z / a_div
    const float* Wt; unsigned w_bytes;                // (N, 9, Cin) tap-major
    const float* bias;
    float* C; int nchw;                               // (z, HW, N) token-major, or (z, N, H, W)
    int H, W, HW, Cin, N;
    const float* rowscale; unsigned rs_bytes;         // C3_ROWSCALE: (source image, HW, a_div): the gathered pixel q of the source image
                                                      // enters as rowscale[src][q][z % a_div] * A[src][q][k]
    const float* gn_mr; const float* gn_gam; const float* gn_bet;     // C3_GN: (mean, rstd) per grid image, affine per channel
    const float* A2; unsigned a2_bytes; int H3, W3; float sy, sx;     // C3_UPADD: + A2[src][nearest(y, x)][k], (source image, H3 W3, Cin)
    float* stats;                                     // optional: (z, row tile, column tile, 2) tile sums of the output incl. bias
};

// Tile choice: 128 x 64 x 32, eight wavefronts (4 x 2, each 32 x 32 = 2 x 2 MFMA fragments), 54 KB of LDS in two
// stages -> two workgroups per CU; LDS layout, fragment permutation (gemm_prow) and register ring as gemm_tile (mfma_gemm.h).
template <int MODE>
__global__ __launch_bounds__(512) void k_conv3(Conv3Args g) {
    constexpr int BM = C3_BM, BN = C3_BN, BK = 32, LS = 36, MT = 2, NT = 2, WGN = 2, STAGE = (BM + BN) * LS, PD = 2;
    __shared__ __attribute__((aligned(16))) float lds[2][STAGE];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, z = blockIdx.z;
    const int simg = z / g.a_div, K = 9 * g.Cin;
    const __amdgpu_buffer_rsrc_t rsA = pt_rsrc(g.A, g.a_bytes), rsW = pt_rsrc(g.Wt, g.w_bytes);
    const __amdgpu_buffer_rsrc_t rsA2 = pt_rsrc(MODE == C3_UPADD ? g.A2 : g.A, MODE == C3_UPADD ? g.a2_bytes : 16u);
    const __amdgpu_buffer_rsrc_t rsS = pt_rsrc(MODE == C3_ROWSCALE ? g.rowscale : g.A, MODE == C3_ROWSCALE ? g.rs_bytes : 16u);
    // loader: thread t covers 16 bytes (k-quad t & 7) of A rows t / 8 and t / 8 + 64 and of W row t / 8
    const int lr = tid >> 3, lc4 = (tid & 7) * 4;
    unsigned arow[2], amask[2];
    int py[2], px[2];
    unsigned soff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = m0 + lr + 64 * i;
        const bool ok = p < g.HW;
        const int pc = ok ? p : 0;
        py[i] = pc / g.W;
        px[i] = pc - py[i] * g.W;
        unsigned m = 0u;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int y = py[i] + tap / 3 - 1, x = px[i] + tap % 3 - 1;
            m |= (ok && y >= 0 && y < g.H && x >= 0 && x < g.W) ? (1u << tap) : 0u;
        }
        amask[i] = m;                                                     // the taps of this row that fall inside the map
        arow[i] = (unsigned)((((long)simg * g.HW + pc) * g.Cin + lc4) * 4);
        soff[i] = (unsigned)((((long)simg * g.HW + pc) * g.a_div + (z - simg * g.a_div)) * 4);
    }
    const unsigned woff = n0 + lr < g.N ? (unsigned)((((long)(n0 + lr)) * K + lc4) * 4) : OOB;
    const int nst = K / BK;                                               // Cin % 64 == 0: a stage never straddles two taps
    f32x4 ra[PD][2], ra2[PD][2], rb[PD], rgam[PD], rbet[PD];
    float rsc[PD][2];                                                     // C3_ROWSCALE: the scalar of the gathered pixel
    unsigned inm[PD] = {0u, 0u};
    float gmean = 0.f, grstd = 1.f;
    auto fetch = [&](int s, int sl) {                                     // a stage past the end re-fetches the last one (never consumed)
        const int sc = min(s, nst - 1), k0 = sc * BK, tap = k0 / g.Cin, c0 = k0 - tap * g.Cin;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        const unsigned delta = (unsigned)(dy * g.W + dx) * (unsigned)(g.Cin * 4) + (unsigned)(c0 * 4);     // modulo 2^32: arow + delta is exact
        unsigned m = 0u;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool in = ((amask[i] >> tap) & 1u) != 0u;
            m |= in ? (1u << i) : 0u;
            ra[sl][i] = pt_bload4(rsA, in ? arow[i] + delta : OOB);
            if (MODE == C3_ROWSCALE) rsc[sl][i] = pt_bload1(rsS, in ? soff[i] + (unsigned)(dy * g.W + dx) * (unsigned)(g.a_div * 4) : OOB);
            if (MODE == C3_UPADD) {                                       // F.interpolate(mode='nearest', size=...): floor(dst * (in / out)) in fp32
                const int ly = min((int)floorf((float)(py[i] + dy) * g.sy), g.H3 - 1), lx = min((int)floorf((float)(px[i] + dx) * g.sx), g.W3 - 1);
                ra2[sl][i] = pt_bload4(rsA2, in ? (unsigned)((((long)simg * g.H3 * g.W3 + ly * g.W3 + lx) * g.Cin + c0 + lc4) * 4) : OOB);
            }
        }
        inm[sl] = m;
        if (MODE == C3_GN) {
            rgam[sl] = *reinterpret_cast<const f32x4*>(g.gn_gam + c0 + lc4);
            rbet[sl] = *reinterpret_cast<const f32x4*>(g.gn_bet + c0 + lc4);
        }
        rb[sl] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW, woff, (unsigned)sc * (BK * 4u), 0));
    };
    auto stash = [&](int sl, int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f32x4 v = ra[sl][i];
            const bool in = ((inm[sl] >> i) & 1u) != 0u;
            if (MODE == C3_UPADD) v += ra2[sl][i];                        // both are zero outside the map
            if (MODE == C3_ROWSCALE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = in ? rsc[sl][i] * v[e] : 0.f;
            }
            if (MODE == C3_GN) {                                          // the expression of k_gn_apply; the padding stays 0
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = in ? fmaxf((v[e] - gmean) * grstd * rgam[sl][e] + rbet[sl][e], 0.f) : 0.f;
            }
            *reinterpret_cast<f32x4*>(&lds[buf][(lr + 64 * i) * LS + lc4]) = v;
        }
        *reinterpret_cast<f32x4*>(&lds[buf][(BM + lr) * LS + lc4]) = rb[sl];
    };
    f32x4 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int qoff = ((lane >> 4) & 1) * 2 + (lane >> 5);                 // conflict-free fragment maps of gemm_tile
    const int aso = (wm * 32 + gemm_prow(lane & 15)) * LS + qoff * 4, bso = (BM + wn * 32 + gemm_prow(lane & 15)) * LS + qoff * 4;
#pragma unroll
    for (int sl = 0; sl < PD; ++sl) fetch(sl, sl);
    if (MODE == C3_GN) { gmean = g.gn_mr[2 * z]; grstd = g.gn_mr[2 * z + 1]; }
    stash(0, 0);
    __syncthreads();
    for (int t0 = 0; t0 < nst; t0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            const int s = t0 + u, buf = u & 1;
            fetch(s + PD, u);                                             // slot u (stage s) already sits in lds[buf]
            if (s < nst) {                                                // workgroup-uniform
                const float* as = &lds[buf][aso];
                const float* bs = &lds[buf][bso];
                f32x4 fa[BK / 16][MT], fb[BK / 16][NT];
#pragma unroll
                for (int hh = 0; hh < BK / 16; ++hh) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) fa[hh][mt] = *reinterpret_cast<const f32x4*>(as + mt * 16 * LS + hh * 16);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) fb[hh][nt] = *reinterpret_cast<const f32x4*>(bs + nt * 16 * LS + hh * 16);
                }
#pragma unroll
                for (int hh = 0; hh < BK / 16; ++hh)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(fa[hh][mt][j], fb[hh][nt][j], acc[mt][nt]);
            }
            stash((u + 1) % PD, buf ^ 1);                                 // stage s + 1 (past the end: never read)
            __syncthreads();
        }
    }
    // epilogue: bias, tile statistics of what GroupNorm(1, N) sees, stores (rows past the image's last pixel are dropped)
    const __amdgpu_buffer_rsrc_t rsC = pt_rsrc(g.C, 0xFFFFFFE0u);
    float s = 0.f, q = 0.f;
    unsigned rbase[MT][4];
    bool rok[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = m0 + wm * 32 + mt * 16 + gemm_prow(4 * (lane >> 4) + r);
            rok[mt][r] = p < g.HW;
            const long o = g.nchw ? (long)z * g.N * g.HW + p : ((long)z * g.HW + p) * g.N;
            rbase[mt][r] = rok[mt][r] ? (unsigned)(o * 4) : OOB;
        }
    const unsigned cstep = (unsigned)(g.nchw ? g.HW : 1) * 4u;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + wn * 32 + nt * 16 + gemm_prow(lane & 15);
        const bool cok = col < g.N;
        const float bv = g.bias ? g.bias[cok ? col : 0] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[mt][nt][r] + bv;
                const bool ok = cok && rok[mt][r];
                s += ok ? v : 0.f;
                q += ok ? v * v : 0.f;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC, ok ? rbase[mt][r] + (unsigned)col * cstep : OOB, 0, 0);
            }
    }
    if (g.stats) {                                                        // uniform; fixed order: lanes (xor tree), then wavefronts 0..7
        double sd = (double)s, qd = (double)q;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sd += __shfl_xor(sd, off, 64); qd += __shfl_xor(qd, off, 64); }
        if (lane == 0) { red[2 * wave] = sd; red[2 * wave + 1] = qd; }
        __syncthreads();
        if (tid == 0) {
            double ts = 0.0, tq = 0.0;
            for (int w = 0; w < 8; ++w) { ts += red[2 * w]; tq += red[2 * w + 1]; }
            float* dst = g.stats + (((long)z * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * 2;
            dst[0] = (float)ts;
            dst[1] = (float)tq;
        }
    }
}

// (mean, rstd) of every image from its tile slots, summed in slot order in double (the arithmetic of k_gn_apply); one workgroup per image
__global__ __launch_bounds__(64) void k_conv3_gn_finish(const float* __restrict__ stats, int nslots, float* __restrict__ mr, int count) {
    __shared__ double ps[64], pq[64];
    const int z = blockIdx.x, t = threadIdx.x;
    const int per = (nslots + 63) / 64, k0 = t * per, k1 = min(nslots, k0 + per);     // thread t: a contiguous run of slots
    double s = 0.0, q = 0.0;
    for (int k = k0; k < k1; ++k) {
        s += (double)stats[((long)z * nslots + k) * 2];
        q += (double)stats[((long)z * nslots + k) * 2 + 1];
    }
    ps[t] = s; pq[t] = q;
    __syncthreads();
    if (t == 0) {
        double ts = 0.0, tq = 0.0;
        for (int w = 0; w < 64; ++w) { ts += ps[w]; tq += pq[w]; }
        const double mean_d = ts / count;
        mr[2 * z] = (float)mean_d;
        mr[2 * z + 1] = (float)(1.0 / sqrt(fmax(tq / count - mean_d * mean_d, 0.0) + 1e-5));
    }
}

// ltrb[z][n][p] = exp(bias[n] + sum_{tap, c} w[n][tap][c] relu(GroupNorm(x))[z][p + tap][c]) (heads.py:135): one wavefront per run of 8
// pixels of a map row, lane l owns channels 4 l + 256 i; the 10 input pixels of a row of taps are normalised once and serve all three
// horizontal taps; the 32 dot products are reduced across the wavefront in fixed order (wave_sum).  Halo pixels contribute 0.
__global__ __launch_bounds__(256) void k_reg_out(const float* __restrict__ X, const float* __restrict__ gn_mr, const float* __restrict__ gam,
                                                 const float* __restrict__ bet, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                 float* __restrict__ out, int H, int W, int D, int nimg) {
    const int lane = threadIdx.x & 63, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int runs = (W + 7) / 8;
    if (wv >= nimg * H * runs) return;                                    // whole wavefronts leave; no barrier below
    const int z = wv / (H * runs), rem = wv - z * H * runs, y = rem / runs, x0 = (rem - y * runs) * 8;
    const float mean = gn_mr[2 * z], rstd = gn_mr[2 * z + 1];
    const long HW = (long)H * W;
    float acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[a][n] = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(gam + c), b4 = *reinterpret_cast<const f32x4*>(bet + c);
        for (int dy = 0; dy < 3; ++dy) {
            const int yy = y + dy - 1;
            if (yy < 0 || yy >= H) continue;                              // uniform
            f32x4 xv[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const int xx = x0 - 1 + j;
                const bool in = xx >= 0 && xx < W;
                const f32x4 v = *reinterpret_cast<const f32x4*>(X + ((long)z * HW + (long)yy * W + min(max(xx, 0), W - 1)) * D + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[j][e] = in ? fmaxf((v[e] - mean) * rstd * g4[e] + b4[e], 0.f) : 0.f;
            }
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                f32x4 w[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) w[n] = *reinterpret_cast<const f32x4*>(Wt + ((long)n * 9 + dy * 3 + dx) * D + c);
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const f32x4 v = xv[a + dx];
                        acc[a][n] += (v[0] * w[n][0] + v[1] * w[n][1]) + (v[2] * w[n][2] + v[3] * w[n][3]);
                    }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const float t = wave_sum(acc[a][n]);
            if (lane == a * 4 + n && x0 + a < W) out[((long)z * 4 + n) * HW + (long)y * W + x0 + a] = expf(t + bias[n]);
        }
}

int conv3_route(int mode) {
    return mode == C3_PLAIN ? PT_HEADS_R_CONV3_PLAIN : mode == C3_ROWSCALE ? PT_HEADS_R_CONV3_ROWSCALE : mode == C3_GN ? PT_HEADS_R_CONV3_GN
                                                                                                                    : PT_HEADS_R_CONV3_UPADD;
}

// Cin, N multiples of 64 up to 512; every operand and the output inside the 32-bit byte offsets of the raw buffer accesses; the grid's z
bool conv3_ok(long nimg, long nsrc, int Cin, int N, int H, int W) {
    if (nimg <= 0 || nsrc <= 0 || H <= 0 || W <= 0 || Cin <= 0 || N <= 0) return false;
    if (Cin % 64 != 0 || N % 64 != 0 || Cin > 512 || N > 512 || nimg > 65535 || nsrc > 65535) return false;
    const unsigned long lim = 0xFFFFFFE0ul / 4 / (unsigned long)std::max(Cin, N);     // pixels whose channel rows stay addressable
    if ((unsigned long)H > lim || (unsigned long)W > lim || (unsigned long)H * W > lim) return false;
    return (unsigned long)nimg * H * W <= lim && (unsigned long)nsrc * H * W <= lim;
}

int launch_conv3(int mode, const Conv3Args& g, int nimg, hipStream_t st, PtRouteLog* log) {
    if (!conv3_ok(nimg, (nimg + g.a_div - 1) / g.a_div, g.Cin, g.N, g.H, g.W)) return PT_ERR_UNSUPPORTED;
    if (log) {
        pt_route_note(log, conv3_route(mode));
        return PT_OK;
    }
    const dim3 grid((g.HW + C3_BM - 1) / C3_BM, g.N / C3_BN, nimg), block(512);
    if (mode == C3_PLAIN) hipLaunchKernelGGL((k_conv3<C3_PLAIN>), grid, block, 0, st, g);
    else if (mode == C3_ROWSCALE) hipLaunchKernelGGL((k_conv3<C3_ROWSCALE>), grid, block, 0, st, g);
    else if (mode == C3_GN) hipLaunchKernelGGL((k_conv3<C3_GN>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((k_conv3<C3_UPADD>), grid, block, 0, st, g);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

Conv3Args conv3_args(const float* A, long src_imgs, int a_div, const float* Wt, const float* bias, float* C, int nchw, int H, int W, int Cin,
                     int N) {
    Conv3Args g{};
    g.A = A; g.a_bytes = (unsigned)(src_imgs * H * W * Cin * 4); g.a_div = a_div;
    g.Wt = Wt; g.w_bytes = (unsigned)((long)N * 9 * Cin * 4); g.bias = bias;
    g.C = C; g.nchw = nchw; g.H = H; g.W = W; g.HW = H * W; g.Cin = Cin; g.N = N;
    return g;
}

struct TamosRegCarve { size_t X, fproj, att, T0, T1, stats, mr, total; int nslots; };
TamosRegCarve tamos_reg_carve(int n_img, int T, int D, int H, int W) {
    TamosRegCarve c{};
    const size_t HW = (size_t)H * W, Mz = (size_t)n_img * T * HW;
    size_t o = 0;
    auto take = [&](size_t k) { size_t r = o; o += pt_align_floats(k); return r; };
    c.nslots = (int)((HW + C3_BM - 1) / C3_BM) * (D / C3_BN);
    c.X = take((size_t)n_img * HW * D); c.fproj = take((size_t)n_img * T * D); c.att = take((size_t)n_img * HW * T);
    c.T0 = take(Mz * D); c.T1 = take(Mz * D);
    c.stats = take((size_t)2 * n_img * T * c.nslots); c.mr = take((size_t)2 * n_img * T);
    c.total = o;
    return c;
}

int tamos_reg_check(int n_img, int T, int D, int H, int W) {
    if (n_img <= 0 || T <= 0 || D <= 0 || H <= 0 || W <= 0) return PT_ERR_SHAPE;
    if (T > 16 || !conv3_ok((long)n_img * T, n_img, D, D, H, W)) return PT_ERR_UNSUPPORTED;
    return PT_OK;
}

int tamos_bbreg_impl(const float* params, const float* feat, const float* filters, float* ltrb, int n_img, int T, int D, int H, int W,
                     void* ws, size_t ws_bytes, void* stream, PtRouteLog* log) {
    if (!params || !feat || !filters || !ltrb || !ws) return PT_ERR_NULL;
    int rc = tamos_reg_check(n_img, T, D, H, W);
    if (rc) return rc;
    const TamosRegCarve cv = tamos_reg_carve(n_img, T, D, H, W);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const RegOff ro = reg_layout(D);
    const int HW = H * W, nz = n_img * T;
    float* base = (float*)ws;
    float *X = base + cv.X, *fproj = base + cv.fproj, *att = base + cv.att, *stats = base + cv.stats, *mr = base + cv.mr;
    PT_TOMP_LAUNCH(PT_HEADS_R_NCHW_TOKENS, k_nchw_to_tokens, dim3((HW + 31) / 32, (D + 31) / 32, n_img), dim3(256), 0, st, feat, X, D, HW);
    // the T filters of every image through `linear` (heads.py:123), then the T attention maps of an image as one HW x D by D x T product
    GemmArgs gp = gemm_args(filters, D, nz, params + ro.lw, nz, D, D, params + ro.lb, fproj, D);
    if ((rc = launch_gemm(gp, st, false, log))) return rc;
    for (int i = 0; i < n_img; ++i) {
        GemmArgs ga = gemm_args(X + (size_t)i * HW * D, D, HW, fproj + (size_t)i * T * D, HW, T, D, nullptr, att + (size_t)i * HW * T, T);
        if ((rc = launch_gemm(ga, st, false, log))) return rc;
    }
    // tower: layer 0 reads attention (.) feature through the per-row scalar, layers 1..3 the previous layer's raw output through its
    // GroupNorm + ReLU; every layer leaves its tile statistics, k_conv3_gn_finish turns them into (mean, rstd) per image
    float *src = base + cv.T0, *dst = base + cv.T1;
    for (int i = 0; i < 4; ++i) {
        Conv3Args g = i == 0 ? conv3_args(X, n_img, T, params + ro.cw[0], params + ro.cb[0], src, 0, H, W, D, D)
                             : conv3_args(src, nz, 1, params + ro.cw[i], params + ro.cb[i], dst, 0, H, W, D, D);
        g.stats = stats;
        if (i == 0) {
            g.rowscale = att; g.rs_bytes = (unsigned)((size_t)n_img * HW * T * 4);
        } else {
            g.gn_mr = mr; g.gn_gam = params + ro.gg[i - 1]; g.gn_bet = params + ro.gb[i - 1];
        }
        if ((rc = launch_conv3(i == 0 ? C3_ROWSCALE : C3_GN, g, nz, st, log))) return rc;
        PT_TOMP_LAUNCH(PT_HEADS_R_CONV3_GN_FINISH, k_conv3_gn_finish, dim3(nz), dim3(64), 0, st, stats, cv.nslots, mr, HW * D);
        if (i > 0) std::swap(src, dst);
    }
    const int waves = nz * H * ((W + 7) / 8);
    PT_TOMP_LAUNCH(PT_HEADS_R_REG_OUT, k_reg_out, dim3((waves + 3) / 4), dim3(256), 0, st, src, mr, params + ro.gg[3], params + ro.gb[3],
                   params + ro.fw, params + ro.fb, ltrb, H, W, D, nz);
    return PT_OK;
}

// ---- heads.FPN with two levels (heads.py:144-162 around torchvision's FeaturePyramidNetwork) ----------------------------------------
// pack: inner_blocks.0 weight (D, C_hi), bias (D); inner_blocks.1 weight (D, C_lo), bias (D); layer_blocks.0 weight (D, 9, D) tap-major,
// bias (D); layer_blocks.1 weight (D, 9, D) tap-major, bias (D)
struct FpnOff { size_t iw0, ib0, iw1, ib1, lw0, lb0, lw1, lb1, total; };
FpnOff fpn_layout(int C_hi, int C_lo, int D) {
    FpnOff o{};
    size_t c = 0;
    auto take = [&](size_t n) { size_t r = c; c += n; return r; };
    o.iw0 = take((size_t)D * C_hi); o.ib0 = take(D); o.iw1 = take((size_t)D * C_lo); o.ib1 = take(D);
    o.lw0 = take((size_t)D * 9 * D); o.lb0 = take(D); o.lw1 = take((size_t)D * 9 * D); o.lb1 = take(D);
    o.total = c;
    return o;
}

struct FpnCarve { size_t X2, X3, L2, L3, total; };
FpnCarve fpn_carve(int n, int C_hi, int C_lo, int D, int H2, int W2, int H3, int W3) {
    FpnCarve c{};
    size_t o = 0;
    auto take = [&](size_t k) { size_t r = o; o += pt_align_floats(k); return r; };
    const size_t M2 = (size_t)n * H2 * W2, M3 = (size_t)n * H3 * W3;
    c.X2 = take(M2 * C_hi); c.X3 = take(M3 * C_lo); c.L2 = take(M2 * D); c.L3 = take(M3 * D);
    c.total = o;
    return c;
}

int fpn_check(int n, int C_hi, int C_lo, int D, int H2, int W2, int H3, int W3) {
    if (n <= 0 || C_hi <= 0 || C_lo <= 0 || D <= 0 || H2 <= 0 || W2 <= 0 || H3 <= 0 || W3 <= 0) return PT_ERR_SHAPE;
    if (C_hi % 64 != 0 || C_lo % 64 != 0 || C_hi > 2048 || C_lo > 2048) return PT_ERR_UNSUPPORTED;
    if (!conv3_ok(n, n, D, D, H2, W2) || !conv3_ok(n, n, D, D, H3, W3)) return PT_ERR_UNSUPPORTED;
    if ((size_t)n * H2 * W2 * C_hi * 4 >= 0xFFFFFFE0ull || (size_t)n * H3 * W3 * C_lo * 4 >= 0xFFFFFFE0ull) return PT_ERR_UNSUPPORTED;
    return PT_OK;
}

int fpn2_impl(const float* params, const float* feat_hi, const float* feat_lo, float* feat2, float* feat3, int n, int C_hi, int C_lo, int D,
              int H2, int W2, int H3, int W3, int want_feat3, void* ws, size_t ws_bytes, void* stream, PtRouteLog* log) {
    if (!params || !feat_hi || !feat_lo || !feat2 || !ws || (want_feat3 && !feat3)) return PT_ERR_NULL;
    int rc = fpn_check(n, C_hi, C_lo, D, H2, W2, H3, W3);
    if (rc) return rc;
    const FpnCarve cv = fpn_carve(n, C_hi, C_lo, D, H2, W2, H3, W3);
    if (ws_bytes < cv.total * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const FpnOff fo = fpn_layout(C_hi, C_lo, D);
    float* base = (float*)ws;
    const int HW2 = H2 * W2, HW3 = H3 * W3, M2 = n * HW2, M3 = n * HW3;
    PT_TOMP_LAUNCH(PT_HEADS_R_NCHW_TOKENS, k_nchw_to_tokens, dim3((HW2 + 31) / 32, (C_hi + 31) / 32, n), dim3(256), 0, st, feat_hi, base + cv.X2,
                   C_hi, HW2);
    PT_TOMP_LAUNCH(PT_HEADS_R_NCHW_TOKENS, k_nchw_to_tokens, dim3((HW3 + 31) / 32, (C_lo + 31) / 32, n), dim3(256), 0, st, feat_lo, base + cv.X3,
                   C_lo, HW3);
    // the 1x1 lateral convolutions are plain products over the tokens
    GemmArgs g2 = gemm_args(base + cv.X2, C_hi, M2, params + fo.iw0, M2, D, C_hi, params + fo.ib0, base + cv.L2, D);
    if ((rc = launch_gemm(g2, st, false, log))) return rc;
    GemmArgs g3 = gemm_args(base + cv.X3, C_lo, M3, params + fo.iw1, M3, D, C_lo, params + fo.ib1, base + cv.L3, D);
    if ((rc = launch_gemm(g3, st, false, log))) return rc;
    // top-down: the high map's 3x3 loader adds the nearest low lateral to the high lateral on the way into LDS (no pass of its own)
    Conv3Args c2 = conv3_args(base + cv.L2, n, 1, params + fo.lw0, params + fo.lb0, feat2, 1, H2, W2, D, D);
    c2.A2 = base + cv.L3; c2.a2_bytes = (unsigned)((long)M3 * D * 4); c2.H3 = H3; c2.W3 = W3;
    c2.sy = (float)H3 / (float)H2; c2.sx = (float)W3 / (float)W2;
    if ((rc = launch_conv3(C3_UPADD, c2, n, st, log))) return rc;
    if (want_feat3) {
        Conv3Args c3 = conv3_args(base + cv.L3, n, 1, params + fo.lw1, params + fo.lb1, feat3, 1, H3, W3, D, D);
        if ((rc = launch_conv3(C3_PLAIN, c3, n, st, log))) return rc;
    }
    return PT_OK;
}

}  // namespace

extern "C" size_t pt_tamos_bbreg_ws_bytes(int n_img, int T, int d_model, int H, int W) {
    if (tamos_reg_check(n_img, T, d_model, H, W)) return 0;
    return tamos_reg_carve(n_img, T, d_model, H, W).total * sizeof(float);
}

extern "C" int pt_tamos_bbreg_f32(const float* params, const float* feat, const float* filters, float* ltrb, int n_img, int T, int d_model,
                                  int H, int W, void* ws, size_t ws_bytes, void* stream) {
    return tamos_bbreg_impl(params, feat, filters, ltrb, n_img, T, d_model, H, W, ws, ws_bytes, stream, nullptr);
}

extern "C" int pt_tamos_bbreg_routes(int n_img, int T, int d_model, int H, int W, int* routes, int cap, int* n_routes) {
    if (!routes || !n_routes) return PT_ERR_NULL;
    if (cap < 0) return PT_ERR_SHAPE;
    PtRouteLog log{routes, cap, 0};
    const int rc = tamos_bbreg_impl(route_fake(0), route_fake(1), route_fake(2), route_fake(3), n_img, T, d_model, H, W, route_fake(4),
                                    ~(size_t)0, nullptr, &log);
    return route_finish(rc, log, routes, cap, n_routes);
}

extern "C" size_t pt_fpn2_param_floats(int C_hi, int C_lo, int d_out) {
    if (C_hi <= 0 || C_lo <= 0 || d_out <= 0 || C_hi % 64 != 0 || C_lo % 64 != 0 || d_out % 64 != 0 || d_out > 512) return 0;
    return fpn_layout(C_hi, C_lo, d_out).total;
}

extern "C" size_t pt_fpn2_ws_bytes(int n, int C_hi, int C_lo, int d_out, int H2, int W2, int H3, int W3) {
    if (fpn_check(n, C_hi, C_lo, d_out, H2, W2, H3, W3)) return 0;
    return fpn_carve(n, C_hi, C_lo, d_out, H2, W2, H3, W3).total * sizeof(float);
}

extern "C" int pt_fpn2_f32(const float* params, const float* feat_hi, const float* feat_lo, float* feat2, float* feat3, int n, int C_hi,
                           int C_lo, int d_out, int H2, int W2, int H3, int W3, int want_feat3, void* ws, size_t ws_bytes, void* stream) {
    return fpn2_impl(params, feat_hi, feat_lo, feat2, feat3, n, C_hi, C_lo, d_out, H2, W2, H3, W3, want_feat3, ws, ws_bytes, stream, nullptr);
}

extern "C" int pt_fpn2_routes(int n, int C_hi, int C_lo, int d_out, int H2, int W2, int H3, int W3, int want_feat3, int* routes, int cap,
                              int* n_routes) {
    if (!routes || !n_routes) return PT_ERR_NULL;
    if (cap < 0) return PT_ERR_SHAPE;
    PtRouteLog log{routes, cap, 0};
    const int rc = fpn2_impl(route_fake(0), route_fake(1), route_fake(2), route_fake(3), route_fake(4), n, C_hi, C_lo, d_out, H2, W2, H3, W3,
                             want_feat3, route_fake(5), ~(size_t)0, nullptr, &log);
    return route_finish(rc, log, routes, cap, n_routes);
}
