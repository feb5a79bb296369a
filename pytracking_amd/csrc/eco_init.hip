// ECO's first-frame joint optimisation of the filter and the projection matrix (pytracking/tracker/eco/eco.py:152-158):
// GaussNewtonCG.run (pytracking/libs/optimization.py:293-421) on FactorizedConvProblem (pytracking/tracker/eco/optim.py:8-118), with the
// Gauss-Newton operator that the reference obtains from two autograd passes written out.
//
// Per block: the filter h (c, Hf, Wh) complex, the projection P (Cin, c) real, the uncompressed samples X (Hf, Wh, n, Cin) complex, the real
// label y, sw = sample_weights_sqrt (1 or n entries), the real reg filter.  Residuals: sw_s (x[k,s]^T P h[k] - y[k]) per bin k and sample s;
// ONE correlation of [conj(flip(h[.., 1 : pad2 + 1])), h] with the reg filter at padding (pad1, pad2) = (min(Rh - 1, Hf - 1),
// min(Rw - 1, Wh - 1)); sqrt(projection_reg) P.  The left extension is detached in the reference: it is part of the residual, not of J.
//
//   k_eci_data    per bin: m = P dh[k] + dP h[k] (linearisation: m = P h[k]), g[s] = sw_s (x[k,s] . m (- y[k])),
//                 v[i] = sum_s conj(x[k,s,i]) sw_s g[s] (stored for k_eci_pgrad), q_h[k,c] = sum_i P[i,c] v[i]                    1 per J^T J
//   k_eci_reg     per filter coefficient: q_h += J_reg^T J_reg (linearisation: J_reg^T of the residual with the left extension)     1 per J^T J
//   k_eci_pgrad   per (i, c): q_P = sum_k Re(v[k,i] conj(h[k,c])) + projection_reg dP (linearisation: P)                             1 per J^T J
//   k_eci_rho     per block: (r = -q,) z = r / M, rho = ip(r, z) over filter AND projection, beta, p = z + beta p, joint flag       1 per iteration
//   k_eci_step    per block: ip(p, q), alpha = rho / ip(p, q), delta += alpha p, r -= alpha q (not on the last iteration)           1 per iteration
//   k_eci_apply   h += delta_h, P += delta_P                                                                                        1 per GN iteration
//   k_eci_clear   lowers the exit flags                                                                                             1 per call
//
// One CG iteration is 5 launches, one Gauss-Newton iteration 3 + 5 num_cg_iter + 1; all blocks ride in every launch.  CG is run_CG as GaussNewtonCG constructs it:
// Fletcher-Reeves, alpha = rho / ip(p, q), p and rho reset at every Gauss-Newton iteration, x = None (r = b = -J^T f0), the last residual
// update skipped.  ip is one scalar per block, inner_prod_fs of the filter parts plus the dot product of the projection parts; alpha and
// beta are per block, the rho == 0 check is joint.
//
// rho == 0 (exactly, in any block, at the top of a CG iteration): the CG run of that Gauss-Newton iteration ends for every block, the
// delta accumulated so far (zero when it is the first iteration) is added, and the next Gauss-Newton iteration linearises again.  Where the
// reference goes on (an exact zero after the first iteration) this is what it does; on a zero in the FIRST iteration the reference adds
// `None` to its variable and raises, here the variables are left as they stand.  A flag row per Gauss-Newton iteration in the workspace turns the remaining
// launches of that run into no-ops; nothing is read back.
//
// The samples of a bin (n Cin complex, contiguous) are read twice by the bin's workgroup, the second time from cache: X comes from HBM once
// per application of J^T J and once per linearisation.  Storage is fp32; every sum over samples, channels and coefficients runs in double
// registers in one fixed order (wave reductions are fixed shuffle trees): no atomics, repeated calls give the same bits.
#include <math.h>
#include "common.h"
#include "pt_internal.h"

namespace {

constexpr int ECI_MAX_CIN = 512, ECI_MAX_C = 64, ECI_MAX_N = 64, ECI_MAX_GN = 32, ECI_MAX_CG = 62, ECI_FLAGS = ECI_MAX_GN * 64;

struct InitBlock {
    const float2* X; const float *sw, *yf, *reg, *dM;
    float2* h; float* P;                                             // in/out
    float2 *V, *q, *r, *p, *dx; float *qP, *rP, *pP, *dxP, *scal;    // workspace; scal[0] = rho
    int Hf, Wh, Cin, c, n, nw, Rh, Rw, pad1, pad2;
    float precond;
};
struct InitArgs {
    InitBlock blk[PT_ECO_MAX_BLOCKS];
    int* flag;
    float preg;
};

__device__ inline double eci_wave_sum(double v) {                      // fixed tree over the 64 lanes; lane 0 holds the result
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ inline double eci_block_sum(double v, double* sh) {         // 1024 threads, fixed order; every thread gets the result
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

// grid (max bins, blocks), 256 threads.  lin: the linearisation (J^T f0 at the variables), else J^T J of the direction p
__global__ __launch_bounds__(256) void k_eci_data(InitArgs a, int lin, int gn, int it) {
    __shared__ float2 h_s[ECI_MAX_C], d_s[ECI_MAX_C];
    __shared__ double2 m_s[ECI_MAX_CIN];
    __shared__ double2 g_s[ECI_MAX_N];
    __shared__ float2 v_s[ECI_MAX_CIN];
    __shared__ double2 part[4][ECI_MAX_C];
    if (!lin && a.flag[gn * 64 + it + 1]) return;
    const InitBlock& B = a.blk[blockIdx.y];
    const int bins = B.Hf * B.Wh, bin = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (bin >= bins) return;
    const int Cin = B.Cin, c = B.c, n = B.n;
    if (t < c) {
        h_s[t] = B.h[(size_t)t * bins + bin];
        if (!lin) d_s[t] = B.p[(size_t)t * bins + bin];
    }
    __syncthreads();
    for (int i = t; i < Cin; i += 256) {                               // m[i] = sum_c P[i,c] dh[c] + dP[i,c] h[c]
        const float* Pr = B.P + (size_t)i * c;
        double re = 0.0, im = 0.0;
        if (lin) {
            for (int k = 0; k < c; ++k) {
                const double w = (double)Pr[k];
                re = fma(w, (double)h_s[k].x, re);
                im = fma(w, (double)h_s[k].y, im);
            }
        } else {
            const float* Dr = B.pP + (size_t)i * c;
            for (int k = 0; k < c; ++k) {
                const double w = (double)Pr[k], d = (double)Dr[k];
                re = fma(w, (double)d_s[k].x, fma(d, (double)h_s[k].x, re));
                im = fma(w, (double)d_s[k].y, fma(d, (double)h_s[k].y, im));
            }
        }
        m_s[i] = make_double2(re, im);
    }
    __syncthreads();
    const float2* X = B.X + (size_t)bin * n * Cin;
    const double y = lin ? (double)B.yf[bin] : 0.0;
    for (int s = wv; s < n; s += 4) {                                  // a wave per sample: g[s] = sw_s (x[s] . m - y)
        const float2* xs = X + (size_t)s * Cin;
        double re = 0.0, im = 0.0;
        for (int i = lane; i < Cin; i += 64) {
            const float2 x = xs[i];
            const double2 m = m_s[i];
            re = fma((double)x.x, m.x, fma(-(double)x.y, m.y, re));
            im = fma((double)x.x, m.y, fma((double)x.y, m.x, im));
        }
        re = eci_wave_sum(re);
        im = eci_wave_sum(im);
        if (lane == 0) {
            const double w = (double)B.sw[B.nw == 1 ? 0 : s];
            g_s[s] = make_double2(w * (w * (re - y)), w * (w * im));  // sw_s g[s]: the weight of J^T as well
        }
    }
    __syncthreads();
    for (int i = t; i < Cin; i += 256) {                               // v[i] = sum_s conj(x[s,i]) sw_s g[s]
        double re = 0.0, im = 0.0;
        for (int s = 0; s < n; ++s) {
            const float2 x = X[(size_t)s * Cin + i];
            const double2 g = g_s[s];
            re = fma((double)x.x, g.x, fma((double)x.y, g.y, re));
            im = fma((double)x.x, g.y, fma(-(double)x.y, g.x, im));
        }
        const float2 v = make_float2((float)re, (float)im);
        v_s[i] = v;
        B.V[(size_t)bin * Cin + i] = v;
    }
    __syncthreads();
    if (lane < c) {                                                    // q_h[c] = sum_i P[i,c] v[i]: four ranges of i, added in order
        const int per = (Cin + 3) / 4, i0 = wv * per, i1 = i0 + per < Cin ? i0 + per : Cin;
        double re = 0.0, im = 0.0;
        for (int i = i0; i < i1; ++i) {
            const double w = (double)B.P[(size_t)i * c + lane];
            re = fma(w, (double)v_s[i].x, re);
            im = fma(w, (double)v_s[i].y, im);
        }
        part[wv][lane] = make_double2(re, im);
    }
    __syncthreads();
    if (t < c) {
        double re = 0.0, im = 0.0;
        for (int w = 0; w < 4; ++w) { re += part[w][t].x; im += part[w][t].y; }
        B.q[(size_t)t * bins + bin] = make_float2((float)re, (float)im);
    }
}

// the filter with `padl` conjugate-extended columns on the left: column x >= 0 is v[r][x], -padl <= x < 0 is conj(v[Hf - 1 - r][-x]); zero outside
__device__ inline float2 eci_ext(const float2* v, int r, int x, int Hf, int Wh, int padl) {
    if (r < 0 || r >= Hf || x >= Wh || x < -padl) return make_float2(0.f, 0.f);
    if (x >= 0) return v[r * Wh + x];
    const float2 e = v[(Hf - 1 - r) * Wh - x];
    return make_float2(e.x, -e.y);
}

// grid (ceil(max c bins / 256), blocks), 256 threads.  R = corr(ext, reg) at padding (pad1, pad2), (H1, W1) = (Hf + 2 pad1 - Rh + 1,
// Wh + 3 pad2 - Rw + 1); q_h[r][j] += sum reg[a2][b2] R[r - a2 + pad1][j + 2 pad2 - b2] (the transpose, kept on the non-detached columns).
// lin: ext carries the left extension (the residual itself); else the left columns are zero (the Jacobian of the direction).
// With an unclipped padding (pad1 = Rh - 1, pad2 = Rw - 1: every deployed filter) no index of R that the transpose asks for lies outside
// (H1, W1), so the two correlations are ONE with the reg filter's autocorrelation G (2 Rh - 1, 2 Rw - 1), formed in LDS in double:
// (2 Rh - 1)(2 Rw - 1) taps per coefficient instead of (Rh Rw)^2.  A clipped padding takes the two nested correlations.
__global__ __launch_bounds__(256) void k_eci_reg(InitArgs a, int lin, int gn, int it) {
    __shared__ double G[29 * 29];
    if (!lin && a.flag[gn * 64 + it + 1]) return;
    const InitBlock& B = a.blk[blockIdx.y];
    const int bins = B.Hf * B.Wh, Rh = B.Rh, Rw = B.Rw;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if ((long)blockIdx.x * 256 >= (long)B.c * bins) return;
    const bool full = B.pad1 == Rh - 1 && B.pad2 == Rw - 1;
    const int Gw = 2 * Rw - 1;
    if (full) {
        for (int q = threadIdx.x; q < (2 * Rh - 1) * Gw; q += 256) {
            const int da = q / Gw - (Rh - 1), db = q % Gw - (Rw - 1);
            double s = 0.0;
            for (int a2 = 0; a2 < Rh; ++a2)
                for (int b2 = 0; b2 < Rw; ++b2) {
                    const int a1 = a2 + da, b1 = b2 + db;
                    if (a1 >= 0 && a1 < Rh && b1 >= 0 && b1 < Rw) s = fma((double)B.reg[a2 * Rw + b2], (double)B.reg[a1 * Rw + b1], s);
                }
            G[q] = s;
        }
        __syncthreads();
    }
    if (e >= (long)B.c * bins) return;
    const int k = (int)(e / bins), bin = (int)(e - (long)k * bins), i = bin / B.Wh, j = bin - i * B.Wh;
    const float2* v = (lin ? B.h : B.p) + (size_t)k * bins;
    const int padl = lin ? B.pad2 : 0;
    double re = 0.0, im = 0.0;
    if (full) {
        for (int da = -(Rh - 1); da < Rh; ++da)
            for (int db = -(Rw - 1); db < Rw; ++db) {
                const float2 x = eci_ext(v, i + da, j + db, B.Hf, B.Wh, padl);
                const double g = G[(da + Rh - 1) * Gw + db + Rw - 1];
                re = fma(g, (double)x.x, re);
                im = fma(g, (double)x.y, im);
            }
    } else {
        const int H1 = B.Hf + 2 * B.pad1 - Rh + 1, W1 = B.Wh + 3 * B.pad2 - Rw + 1;
        for (int a2 = 0; a2 < Rh; ++a2)
            for (int b2 = 0; b2 < Rw; ++b2) {
                const int u = i - a2 + B.pad1, w = j + 2 * B.pad2 - b2;
                if (u < 0 || u >= H1 || w < 0 || w >= W1) continue;
                double r1 = 0.0, i1 = 0.0;
                for (int a1 = 0; a1 < Rh; ++a1)
                    for (int b1 = 0; b1 < Rw; ++b1) {
                        const float2 x = eci_ext(v, u + a1 - B.pad1, w + b1 - 2 * B.pad2, B.Hf, B.Wh, padl);
                        const double g = (double)B.reg[a1 * Rw + b1];
                        r1 = fma(g, (double)x.x, r1);
                        i1 = fma(g, (double)x.y, i1);
                    }
                const double g = (double)B.reg[a2 * Rw + b2];
                re = fma(g, r1, re);
                im = fma(g, i1, im);
            }
    }
    const float2 q = B.q[e];
    B.q[e] = make_float2(q.x + (float)re, q.y + (float)im);
    if (lin) B.dx[e] = make_float2(0.f, 0.f);
}

// grid (ceil(max Cin / 64), max c, blocks), 1024 threads: a lane per input channel i, the bins in 16 ranges (one per wave) added in order
__global__ __launch_bounds__(1024) void k_eci_pgrad(InitArgs a, int lin, int gn, int it) {
    __shared__ double part[16][64];
    if (!lin && a.flag[gn * 64 + it + 1]) return;
    const InitBlock& B = a.blk[blockIdx.z];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = blockIdx.x * 64 + lane, cc = blockIdx.y;
    if (cc >= B.c || blockIdx.x * 64 >= B.Cin) return;
    const int bins = B.Hf * B.Wh, per = (bins + 15) / 16, k0 = wv * per, k1 = k0 + per < bins ? k0 + per : bins;
    double acc = 0.0;
    if (i < B.Cin) {
        const float2* hc = B.h + (size_t)cc * bins;
        for (int k = k0; k < k1; ++k) {
            const float2 v = B.V[(size_t)k * B.Cin + i], h = hc[k];
            acc = fma((double)v.x, (double)h.x, fma((double)v.y, (double)h.y, acc));
        }
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv != 0 || i >= B.Cin) return;
    double tot = 0.0;
    for (int w = 0; w < 16; ++w) tot += part[w][lane];
    const size_t o = (size_t)i * B.c + cc;
    B.qP[o] = (float)tot + a.preg * (lin ? B.P[o] : B.pP[o]);
    if (lin) B.dxP[o] = 0.f;
}

// inner_prod_fs weight of a coefficient: 2 <a, b> - <a[.., 0, :], b[.., 0, :]>
__device__ inline double eci_wt(long e, int Wh) { return (e % Wh) == 0 ? 1.0 : 2.0; }

// grid (blocks), 1024 threads
__global__ __launch_bounds__(1024) void k_eci_rho(InitArgs a, int gn, int it) {
    __shared__ double sh[1024];
    int* flag = a.flag + gn * 64;
    if (flag[it]) return;                // raised by an EARLIER iteration: the blocks of one launch never see each other's flag
    const InitBlock& B = a.blk[blockIdx.x];
    const int first = it == 0;
    const long N = (long)B.c * B.Hf * B.Wh, M = (long)B.Cin * B.c;
    const float rho1 = B.scal[0];
    double rz = 0.0;
    for (long e = threadIdx.x; e < N; e += 1024) {
        float2 r;
        if (first) {
            const float2 q = B.q[e];
            r = make_float2(-q.x, -q.y);
            B.r[e] = r;
        } else {
            r = B.r[e];
        }
        const float d = B.dM[e];
        rz += eci_wt(e, B.Wh) * ((double)r.x * (double)(r.x / d) + (double)r.y * (double)(r.y / d));
    }
    for (long e = threadIdx.x; e < M; e += 1024) {
        float r;
        if (first) {
            r = -B.qP[e];
            B.rP[e] = r;
        } else {
            r = B.rP[e];
        }
        rz += (double)r * (double)(r / B.precond);
    }
    rz = eci_block_sum(rz, sh);
    const float rho = (float)rz;
    if (threadIdx.x == 0) {
        B.scal[0] = rho;
        if (rho == 0.f)
            for (int j = it + 1; j < 64; ++j) flag[j] = 1;
    }
    if (rho == 0.f) return;
    float beta = first ? 0.f : rho / rho1;
    beta = beta > 0.f ? beta : 0.f;
    for (long e = threadIdx.x; e < N; e += 1024) {
        const float2 r = B.r[e];
        const float d = B.dM[e];
        float2 z = make_float2(r.x / d, r.y / d);
        if (!first) {
            const float2 p = B.p[e];
            z = make_float2(z.x + p.x * beta, z.y + p.y * beta);
        }
        B.p[e] = z;
    }
    for (long e = threadIdx.x; e < M; e += 1024) {
        float z = B.rP[e] / B.precond;
        if (!first) z += B.pP[e] * beta;
        B.pP[e] = z;
    }
}

// grid (blocks), 1024 threads
__global__ __launch_bounds__(1024) void k_eci_step(InitArgs a, int last, int gn, int it) {
    __shared__ double sh[1024];
    if (a.flag[gn * 64 + it + 1]) return;
    const InitBlock& B = a.blk[blockIdx.x];
    const long N = (long)B.c * B.Hf * B.Wh, M = (long)B.Cin * B.c;
    double pq = 0.0;
    for (long e = threadIdx.x; e < N; e += 1024) {
        const float2 p = B.p[e], q = B.q[e];
        pq += eci_wt(e, B.Wh) * ((double)p.x * q.x + (double)p.y * q.y);
    }
    for (long e = threadIdx.x; e < M; e += 1024) pq += (double)B.pP[e] * (double)B.qP[e];
    pq = eci_block_sum(pq, sh);
    const float alpha = B.scal[0] / (float)pq;
    for (long e = threadIdx.x; e < N; e += 1024) {
        const float2 p = B.p[e];
        const float2 x = B.dx[e];
        B.dx[e] = make_float2(x.x + p.x * alpha, x.y + p.y * alpha);
        if (!last) {
            const float2 q = B.q[e], r = B.r[e];
            B.r[e] = make_float2(r.x - q.x * alpha, r.y - q.y * alpha);
        }
    }
    for (long e = threadIdx.x; e < M; e += 1024) {
        B.dxP[e] += B.pP[e] * alpha;
        if (!last) B.rP[e] -= B.qP[e] * alpha;
    }
}

// grid (ceil(max(2 c bins + Cin c) / 256), blocks), 256 threads
__global__ __launch_bounds__(256) void k_eci_apply(InitArgs a) {
    const InitBlock& B = a.blk[blockIdx.y];
    const long N2 = 2L * B.c * B.Hf * B.Wh, M = (long)B.Cin * B.c, e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < N2) ((float*)B.h)[e] += ((const float*)B.dx)[e];
    else if (e - N2 < M) B.P[e - N2] += B.dxP[e - N2];
}

// grid (ECI_FLAGS / 256), 256 threads: the flag rows of a call, lowered before its first launch reads one
__global__ __launch_bounds__(256) void k_eci_clear(int* flag) { flag[blockIdx.x * 256 + threadIdx.x] = 0; }

bool eci_block_covered(const pt_eco_init_block& s) {
    return s.Cin <= ECI_MAX_CIN && s.c <= ECI_MAX_C && s.n <= ECI_MAX_N && s.Rh <= 15 && s.Rw <= 15 && (long)s.Hf * s.Wh <= (1 << 20);
}
bool eci_block_shaped(const pt_eco_init_block& s) {
    return s.Hf > 0 && s.Wh > 0 && s.Cin > 0 && s.c > 0 && s.n > 0 && s.Rh > 0 && s.Rw > 0 && (s.nw == 1 || s.nw == s.n);
}
inline size_t eci_block_floats(const pt_eco_init_block& s) {
    const size_t K = (size_t)s.Hf * s.Wh, N = (size_t)s.c * K, M = (size_t)s.Cin * s.c;
    return pt_align_floats(2 * K * s.Cin) + 4 * pt_align_floats(2 * N) + 4 * pt_align_floats(M) + 64;
}

}  // namespace

extern "C" size_t pt_eco_joint_init_ws_bytes(const pt_eco_init_block* blk, int nb) {
    if (!blk || nb <= 0 || nb > PT_ECO_MAX_BLOCKS) return 0;
    size_t fl = ECI_FLAGS;
    for (int b = 0; b < nb; ++b) {
        if (!eci_block_shaped(blk[b]) || !eci_block_covered(blk[b])) return 0;
        fl += eci_block_floats(blk[b]);
    }
    return fl * sizeof(float);
}

extern "C" int pt_eco_joint_init_f32(const pt_eco_init_block* blk, int nb, int num_gn_iter, int num_cg_iter, float projection_reg, void* ws,
                                     size_t ws_bytes, void* stream) {
    if (!blk) return PT_ERR_NULL;
    if (nb <= 0 || num_gn_iter < 0 || num_cg_iter < 0) return PT_ERR_SHAPE;
    if (nb > PT_ECO_MAX_BLOCKS || num_gn_iter > ECI_MAX_GN || num_cg_iter > ECI_MAX_CG) return PT_ERR_UNSUPPORTED;
    InitArgs a{};
    int maxbins = 0, maxcin = 0, maxc = 0;
    long maxel = 0, maxall = 0;
    for (int b = 0; b < nb; ++b) {
        const pt_eco_init_block& s = blk[b];
        if (!s.samples || !s.weights_sqrt || !s.yf || !s.reg_filter || !s.diag_M || !s.hf || !s.proj) return PT_ERR_NULL;
        if (!eci_block_shaped(s)) return PT_ERR_SHAPE;
        if (!eci_block_covered(s)) return PT_ERR_UNSUPPORTED;
        InitBlock& B = a.blk[b];
        B.X = (const float2*)s.samples; B.sw = s.weights_sqrt; B.yf = s.yf; B.reg = s.reg_filter; B.dM = s.diag_M;
        B.h = (float2*)s.hf; B.P = s.proj;
        B.Hf = s.Hf; B.Wh = s.Wh; B.Cin = s.Cin; B.c = s.c; B.n = s.n; B.nw = s.nw; B.Rh = s.Rh; B.Rw = s.Rw;
        B.pad1 = s.Rh - 1 < s.Hf - 1 ? s.Rh - 1 : s.Hf - 1;
        B.pad2 = s.Rw - 1 < s.Wh - 1 ? s.Rw - 1 : s.Wh - 1;
        B.precond = s.proj_precond;
        const int bins = s.Hf * s.Wh;
        const long el = (long)s.c * bins, all = 2 * el + (long)s.Cin * s.c;
        if (bins > maxbins) maxbins = bins;
        if (s.Cin > maxcin) maxcin = s.Cin;
        if (s.c > maxc) maxc = s.c;
        if (el > maxel) maxel = el;
        if (all > maxall) maxall = all;
    }
    if (num_gn_iter == 0 || num_cg_iter == 0) return PT_OK;            // the reference's run returns / adds nothing: nothing is touched
    if (!ws) return PT_ERR_NULL;
    if (ws_bytes < pt_eco_joint_init_ws_bytes(blk, nb) || ((uintptr_t)ws & 255)) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    a.flag = (int*)base;
    a.preg = projection_reg;
    base += ECI_FLAGS;
    for (int b = 0; b < nb; ++b) {
        InitBlock& B = a.blk[b];
        const size_t K = (size_t)B.Hf * B.Wh, s2 = pt_align_floats(2 * B.c * K), sM = pt_align_floats((size_t)B.Cin * B.c);
        float* at = base;
        B.V = (float2*)at; at += pt_align_floats(2 * K * B.Cin);
        B.q = (float2*)at; B.r = (float2*)(at + s2); B.p = (float2*)(at + 2 * s2); B.dx = (float2*)(at + 3 * s2); at += 4 * s2;
        B.qP = at; B.rP = at + sM; B.pP = at + 2 * sM; B.dxP = at + 3 * sM; at += 4 * sM;
        B.scal = at;
        base += eci_block_floats(blk[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 gbin(maxbins, nb), gel((unsigned)((maxel + 255) / 256), nb), gall((unsigned)((maxall + 255) / 256), nb);
    const dim3 gpg((maxcin + 63) / 64, maxc, nb);
    hipLaunchKernelGGL(k_eci_clear, dim3(ECI_FLAGS / 256), dim3(256), 0, st, a.flag);
    PT_CHECK_LAUNCH();
    for (int gn = 0; gn < num_gn_iter; ++gn) {
        hipLaunchKernelGGL(k_eci_data, gbin, dim3(256), 0, st, a, 1, gn, 0);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_eci_reg, gel, dim3(256), 0, st, a, 1, gn, 0);
        PT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_eci_pgrad, gpg, dim3(1024), 0, st, a, 1, gn, 0);
        PT_CHECK_LAUNCH();
        for (int it = 0; it < num_cg_iter; ++it) {
            hipLaunchKernelGGL(k_eci_rho, dim3(nb), dim3(1024), 0, st, a, gn, it);
            PT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_eci_data, gbin, dim3(256), 0, st, a, 0, gn, it);
            PT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_eci_reg, gel, dim3(256), 0, st, a, 0, gn, it);
            PT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_eci_pgrad, gpg, dim3(1024), 0, st, a, 0, gn, it);
            PT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_eci_step, dim3(nb), dim3(1024), 0, st, a, it == num_cg_iter - 1 ? 1 : 0, gn, it);
            PT_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_eci_apply, gall, dim3(256), 0, st, a);
        PT_CHECK_LAUNCH();
    }
    return PT_OK;
}
