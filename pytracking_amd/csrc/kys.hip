// KYS state-aware response prediction (pytracking/tracker/kys/kys.py:314 -> ltr/models/kys/predictor_wrapper.py:88-153), fp32, gfx950.
//
//   pt_kys_cost_volume_f32        CostVolume.forward (cost_volume.py:15-26): SpatialCorrelationSampler(3, 2 md + 1, 1, 1) and, for
//                                 abs_coordinate_output, remap_cost_volume fused into the store
//       k_kys_gram                Gt[ks][q][p] = sum_{ch in K slice ks} prev[ch, q] cur[ch, p]     (MFMA, operands read K-major from memory)
//       k_kys_cv_taps             out = sum_ks sum_{i,j in -1..1} Gt[ks][q + (i,j)][p + (i,j)], taps inside the map only, window mask, store
//   pt_kys_predict_response_f32   ResponsePredictor.forward (response_predictor.py:65-159, eval mode) between the two shift_features
//                                 groups of PredictorWrapper.predict_response
//       k_kys_prep                shifted label -> initial state (or state_prev), shifted score, is_target(state_prev)
//       k_kys_cvproc              one workgroup per previous position q: proc1, softmax over p, proc2 (BatchNorm folded)
//       k_kys_propagate           softmax over q, propagation weights, confidence (largest weight, or entropy over all q), propagated state
//       k_kys_head                is_target x2, 10 -> 64 -> 32 -> 1 or 10 -> 16 -> 1 predictor, threshold / window, max-pool concat, ConvGRU,
//                                 shifts back
// Covered structures (a closed list, kys_structure_ok): state_dim 8, gru_ksz 3 and
//     representation dims (64, 32)          conf_measure none / max       two wide maps through global scratch
//     representation dims (16,)  (r1 == 0)  conf_measure none / max / entropy   the 16-channel map stays in LDS; the shipped network
#include "common.h"
#include "pt_internal.h"

namespace {

constexpr int KYS_SD = 8, KYS_R0 = 64, KYS_R1 = 32, KYS_GI = 4, KYS_IT = 4;   // dims the kernels are written for
constexpr int KYS_R16 = 16;                                                   // the one-layer representation stack (rep_dim1 == 0)

// ---------------------------------------------------------------------------------------------------------------------------
// cost volume
// ---------------------------------------------------------------------------------------------------------------------------
// One wavefront = one 32 x 32 tile of Gt for one K slice.  A-operand rows are previous positions q, B-operand columns current
// positions p; both operands are (C, HW) maps, so lane (i, kq) of a 16x16x4 MFMA reads element [k + kq][tile + i] straight from memory
// (16 consecutive floats per k: coalesced, no LDS stage).  The four waves of a workgroup own four consecutive K slices of one tile.
__global__ __launch_bounds__(256) void k_kys_gram(const float* __restrict__ cur, const float* __restrict__ prev, float* __restrict__ Gt,
                                                  int C, int HW, int kchunk, int KS, int zper) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z / zper, ks = (blockIdx.z - b * zper) * 4 + wave;
    if (ks >= KS) return;
    const int q0 = blockIdx.y * 32, p0 = blockIdx.x * 32, li = lane & 15, kq = lane >> 4;
    const float* pc = cur + (long)b * C * HW;
    const float* pp = prev + (long)b * C * HW;
    const int kbeg = ks * kchunk, kend = min(C, kbeg + kchunk);
    const int qa[2] = {q0 + li, q0 + 16 + li}, pa[2] = {p0 + li, p0 + 16 + li};
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = kbeg; k < kend; k += 4) {
        const int kk = k + kq;
        const bool kin = kk < kend;
        const long row = (long)kk * HW;
        float av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            av[t] = (kin && qa[t] < HW) ? pp[row + qa[t]] : 0.f;
            bv[t] = (kin && pa[t] < HW) ? pc[row + pa[t]] : 0.f;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[a][c] = mfma16(av[a], bv[c], acc[a][c]);
    }
    float* g = Gt + ((long)b * KS + ks) * HW * HW;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + a * 16 + 4 * kq + r, p = p0 + c * 16 + li;
                if (q < HW && p < HW) g[(long)q * HW + p] = acc[a][c][r];
            }
}

// One thread per output element, p fastest.  remap: channel = previous position q = (r', c'), zero outside the displacement window.
// Otherwise channel = displacement (di, dj), q = p + (di - md, dj - md), which may lie outside the map while some of its taps do not.
// The 9 KS partial products are summed in double, in a fixed order.
__global__ __launch_bounds__(256) void k_kys_cv_taps(const float* __restrict__ Gt, float* __restrict__ out, int H, int W, int md, int KS,
                                                     int remap, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int HW = H * W, D = 2 * md + 1, nch = remap ? HW : D * D;
    const int p = (int)(idx % HW);
    const long t = idx / HW;
    const int ch = (int)(t % nch), b = (int)(t / nch);
    const int r = p / W, c = p - r * W;
    int rq, cq;
    if (remap) {
        rq = ch / W; cq = ch - rq * W;
        if (abs(rq - r) > md || abs(cq - c) > md) { out[idx] = 0.f; return; }
    } else {
        const int di = ch / D;
        rq = r + di - md; cq = c + (ch - di * D) - md;
    }
    double s = 0.0;
    const long HW2 = (long)HW * HW;
    const float* g = Gt + (long)b * KS * HW2;
#pragma unroll
    for (int i = -1; i <= 1; ++i)
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const int r1 = r + i, c1 = c + j, r2 = rq + i, c2 = cq + j;
            if (r1 < 0 || r1 >= H || c1 < 0 || c1 >= W || r2 < 0 || r2 >= H || c2 < 0 || c2 >= W) continue;
            const float* e = g + (long)(r2 * W + c2) * HW + (r1 * W + c1);
            for (int ks = 0; ks < KS; ++ks) s += (double)e[ks * HW2];
        }
    out[idx] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// response predictor
// ---------------------------------------------------------------------------------------------------------------------------
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2, ACT_TANH = 3 };

__device__ __forceinline__ float kys_act(float v, int act) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_SIGMOID) return 1.f / (1.f + expf(-v));
    if (act == ACT_TANH) return tanhf(v);
    return v;
}

// 3x3 zero-padded convolution over one map set by the whole workgroup: in (Cin, HW), out (Cout, HW), w (Cout, Cin, 3, 3), b (Cout) or null.
// No barrier inside: the caller separates producer and consumer.
__device__ __forceinline__ void kys_conv3(const float* in, int Cin, float* out, int Cout, const float* __restrict__ w,
                                          const float* __restrict__ bias, int H, int W, int act) {
    const int HW = H * W;
    for (int idx = threadIdx.x; idx < Cout * HW; idx += blockDim.x) {
        const int oc = idx / HW, p = idx - oc * HW, y = p / W, x = p - y * W;
        unsigned m = 0u;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            m |= (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (1u << t) : 0u;
        }
        float acc = bias ? bias[oc] : 0.f;
        const float* wp = w + (long)oc * Cin * 9;
        const float* ip = in + p;
        for (int ci = 0; ci < Cin; ++ci, wp += 9, ip += HW) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float v = ((m >> t) & 1u) ? ip[(t / 3 - 1) * W + (t % 3 - 1)] : 0.f;
                acc = fmaf(wp[t], v, acc);
            }
        }
        out[idx] = kys_act(acc, act);
    }
}

// grid_sample(bilinear, zeros, align_corners=False) on affine_grid(identity + translation): a constant pixel offset `s` on both axes
__device__ __forceinline__ float kys_shift_at(const float* m, int H, int W, int y, int x, float s) {
    const float fy = (float)y + s, fx = (float)x + s;
    const float y0f = floorf(fy), x0f = floorf(fx);
    const int y0 = (int)y0f, x0 = (int)x0f;
    const float wy1 = fy - y0f, wx1 = fx - x0f, wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    auto at = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? m[yy * W + xx] : 0.f; };
    return at(y0, x0) * wy0 * wx0 + at(y0, x0 + 1) * wy0 * wx1 + at(y0 + 1, x0) * wy1 * wx0 + at(y0 + 1, x0 + 1) * wy1 * wx1;
}

struct KysW {      // offsets (floats) into the weight pack; layout in include/pt_hot.h
    int p1a_w, p1a_b, p1b_w, p1b_b, p2a_w, p2a_b, p2b_w, p2b_b, init_w, it1_w, it1_b, it2_w, it2_b;
    int r0_w, r0_b, r1_w, r1_b, resp_w, resp_b, gr_w, gr_b, gu_w, gu_b, gn_w, gn_b, total;
};

// r1 == 0: one representation layer of r0 channels, response_predictor reads it
KysW kys_offsets(int with_conf, int r0 = KYS_R0, int r1 = KYS_R1) {
    KysW o{};
    int at = 0;
    auto take = [&](int n) { const int r = at; at += n; return r; };
    o.p1a_w = take(8 * 9); o.p1a_b = take(8); o.p1b_w = take(8 * 9); o.p1b_b = take(1);
    o.p2a_w = take(8 * 9); o.p2a_b = take(8); o.p2b_w = take(8 * 9); o.p2b_b = take(1);
    o.init_w = take(KYS_SD * 9);
    o.it1_w = take(KYS_IT * KYS_SD * 9); o.it1_b = take(KYS_IT); o.it2_w = take(KYS_IT * 9); o.it2_b = take(1);
    const int ci = KYS_SD + 1 + (with_conf ? 1 : 0);
    o.r0_w = take(r0 * ci * 9); o.r0_b = take(r0); o.r1_w = take(r1 * r0 * 9); o.r1_b = take(r1);
    o.resp_w = take((r1 ? r1 : r0) * 9); o.resp_b = take(1);
    const int gi = KYS_GI + KYS_SD;
    o.gr_w = take(KYS_SD * gi * 9); o.gr_b = take(KYS_SD); o.gu_w = take(KYS_SD * gi * 9); o.gu_b = take(KYS_SD);
    o.gn_w = take(KYS_SD * gi * 9); o.gn_b = take(KYS_SD);
    o.total = at;
    return o;
}

// is_target_predictor on `h` (8, HW) -> `it` (HW); `t4` (4, HW) scratch.  Ends with a barrier.
__device__ __forceinline__ void kys_is_target(const float* h, float* t4, float* it, const float* wts, const KysW& o, int H, int W) {
    kys_conv3(h, KYS_SD, t4, KYS_IT, wts + o.it1_w, wts + o.it1_b, H, W, ACT_RELU);
    __syncthreads();
    kys_conv3(t4, KYS_IT, it, 1, wts + o.it2_w, wts + o.it2_b, H, W, ACT_NONE);
    __syncthreads();
}

__device__ __forceinline__ void kys_store_shifted(const float* m, float* dst, int H, int W, float s) {
    for (int p = threadIdx.x; p < H * W; p += blockDim.x) dst[p] = kys_shift_at(m, H, W, p / W, p % W, s);
}

struct KysPrep {
    const float* wts; KysW o;
    const float *state_prev, *label_prev, *score;
    float *hbuf, *sbuf, *is_target;
    int H, W; float shift;
};

__global__ __launch_bounds__(256) void k_kys_prep(KysPrep a) {
    __shared__ float lds[14 * PT_KYS_PRED_MAX_HW];
    const int H = a.H, W = a.W, HW = H * W, b = blockIdx.x;
    float *lab = lds, *h = lab + HW, *t4 = h + KYS_SD * HW, *it = t4 + KYS_IT * HW;
    if (a.state_prev) {
        for (int i = threadIdx.x; i < KYS_SD * HW; i += blockDim.x) h[i] = a.state_prev[(long)b * KYS_SD * HW + i];
    } else {
        kys_store_shifted(a.label_prev + (long)b * HW, lab, H, W, -a.shift);
        __syncthreads();
        kys_conv3(lab, 1, h, KYS_SD, a.wts + a.o.init_w, nullptr, H, W, ACT_TANH);
    }
    kys_store_shifted(a.score + (long)b * HW, a.sbuf + (long)b * HW, H, W, -a.shift);
    __syncthreads();
    for (int i = threadIdx.x; i < KYS_SD * HW; i += blockDim.x) a.hbuf[(long)b * KYS_SD * HW + i] = h[i];
    kys_is_target(h, t4, it, a.wts, a.o, H, W);
    kys_store_shifted(it, a.is_target + (long)b * HW, H, W, a.shift);
}

// workgroup (q, b): the cost-volume map of previous position q over the current positions p
__global__ __launch_bounds__(256) void k_kys_cvproc(const float* __restrict__ cv, const float* __restrict__ wts, KysW o, float* __restrict__ z,
                                                    int H, int W) {
    __shared__ float lds[10 * PT_KYS_PRED_MAX_HW];
    __shared__ float red[4];
    const int HW = H * W;
    const long mapi = (long)blockIdx.y * HW + blockIdx.x;
    float *m0 = lds, *t8 = m0 + HW, *m1 = t8 + 8 * HW;
    for (int p = threadIdx.x; p < HW; p += 256) m0[p] = cv[mapi * HW + p];
    __syncthreads();
    kys_conv3(m0, 1, t8, 8, wts + o.p1a_w, wts + o.p1a_b, H, W, ACT_RELU);
    __syncthreads();
    kys_conv3(t8, 8, m1, 1, wts + o.p1b_w, wts + o.p1b_b, H, W, ACT_NONE);
    __syncthreads();
    float mx = -INFINITY;
    for (int p = threadIdx.x; p < HW; p += 256) mx = fmaxf(mx, m1[p]);
    mx = block_max(mx, red);
    float sm = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) { const float e = expf(m1[p] - mx); m0[p] = e; sm += e; }
    sm = block_sum(sm, red, 256);
    for (int p = threadIdx.x; p < HW; p += 256) m0[p] = m0[p] / sm;
    __syncthreads();
    kys_conv3(m0, 1, t8, 8, wts + o.p2a_w, wts + o.p2a_b, H, W, ACT_RELU);
    __syncthreads();
    kys_conv3(t8, 8, z + mapi * HW, 1, wts + o.p2b_w, wts + o.p2b_b, H, W, ACT_NONE);
}

// workgroup (p tile of 16, b): 16 q groups x 16 positions.  Softmax over q for every p, then w[q, p], conf[p] = max_q w, h'[d, p] = sum_q w h[d, q].
// ENT: conf[p] = -sum_q w[q, p] log(w[q, p] + 1e-4) over ALL previous positions (response_predictor.py:114-116), from the stored w, one
// partial per q group, added in a fixed order through `red`.  logf, not a fast intrinsic: w log(w + 1e-4) at w = 1 is the whole result.
template <bool ENT>
__global__ __launch_bounds__(256) void k_kys_propagate(const float* __restrict__ z, const float* __restrict__ hbuf, float* __restrict__ wout,
                                                       float* __restrict__ conf, float* __restrict__ hprop, int HW) {
    __shared__ float red[16][17];
    __shared__ float hred[KYS_SD][16][17];
    const int pl = threadIdx.x & 15, qg = threadIdx.x >> 4, b = blockIdx.y, p = blockIdx.x * 16 + pl;
    const bool ok = p < HW;
    const float* zb = z + (long)b * HW * HW;
    const float* hb = hbuf + (long)b * KYS_SD * HW;
    float mx = -INFINITY;
    if (ok) for (int q = qg; q < HW; q += 16) mx = fmaxf(mx, zb[(long)q * HW + p]);
    red[qg][pl] = mx;
    __syncthreads();
    mx = red[0][pl];
#pragma unroll
    for (int g = 1; g < 16; ++g) mx = fmaxf(mx, red[g][pl]);
    __syncthreads();
    float sm = 0.f;
    if (ok) for (int q = qg; q < HW; q += 16) sm += expf(zb[(long)q * HW + p] - mx);
    red[qg][pl] = sm;
    __syncthreads();
    sm = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) sm += red[g][pl];
    float hs[KYS_SD];
#pragma unroll
    for (int d = 0; d < KYS_SD; ++d) hs[d] = 0.f;
    float ent = 0.f;
    if (ok) {
        float* wb = wout + (long)b * HW * HW;
        for (int q = qg; q < HW; q += 16) {
            const float wv = expf(zb[(long)q * HW + p] - mx) / sm;
            wb[(long)q * HW + p] = wv;
            if (ENT) ent += wv * logf(wv + 1e-4f);
#pragma unroll
            for (int d = 0; d < KYS_SD; ++d) hs[d] = fmaf(wv, hb[d * HW + q], hs[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < KYS_SD; ++d) hred[d][qg][pl] = hs[d];
    if (ENT) {
        __syncthreads();                                                   // `red` is still being read for the softmax sum
        red[qg][pl] = ent;
    }
    __syncthreads();
    if (ok && qg < KYS_SD) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += hred[qg][g][pl];
        hprop[((long)b * KYS_SD + qg) * HW + p] = t;
    }
    if (ENT) {
        if (ok && qg == KYS_SD) {
            float t = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) t += red[g][pl];
            conf[(long)b * HW + p] = -t;
        }
    } else {
        if (ok && qg == KYS_SD && conf) conf[(long)b * HW + p] = 1.f / sm;     // the largest softmax term is exp(0) / sum
    }
}

struct KysHead {
    const float* wts; KysW o;
    const float *hprop, *conf, *sbuf, *window;
    float *r0buf, *r1buf;
    float *response, *state_cur, *fused_orig, *it_after_prop, *it_new;
    int H, W, with_conf, has_thresh; long window_stride; float thresh, shift;
};

// ONE: the one-layer representation stack.  Its 16-channel map lives in LDS over Y | R (20 HW contiguous floats, dead between the
// is_target pass and the assembly of the GRU input; 16 HW <= 20 HW), response_predictor reads it there; no global round trip.
template <bool ONE>
__global__ __launch_bounds__(1024) void k_kys_head(KysHead a) {
    __shared__ float lds[39 * PT_KYS_PRED_MAX_HW];
    __shared__ float red[16];
    const int H = a.H, W = a.W, HW = H * W, b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int ci = KYS_SD + 1 + (a.with_conf ? 1 : 0), gi = KYS_GI + KYS_SD;
    float *X = lds, *Y = X + 10 * HW, *R = Y + 12 * HW, *U = R + KYS_SD * HW, *f = U + KYS_SD * HW;
    float *t4 = U, *it = U + KYS_IT * HW;                                  // is_target scratch while U is free
    const float* wts = a.wts;
    for (int i = tid; i < KYS_SD * HW; i += nt) X[i] = a.hprop[(long)b * KYS_SD * HW + i];
    for (int p = tid; p < HW; p += nt) {
        X[KYS_SD * HW + p] = a.sbuf[(long)b * HW + p];
        if (a.with_conf) X[(KYS_SD + 1) * HW + p] = a.conf[(long)b * HW + p];
    }
    __syncthreads();
    kys_is_target(X, t4, it, wts, a.o, H, W);
    kys_store_shifted(it, a.it_after_prop + (long)b * HW, H, W, a.shift);
    if (ONE) {
        static_assert(KYS_R16 <= 12 + KYS_SD, "the one-layer map must fit Y | R");
        kys_conv3(X, ci, Y, KYS_R16, wts + a.o.r0_w, wts + a.o.r0_b, H, W, ACT_RELU);
        __syncthreads();
        kys_conv3(Y, KYS_R16, f, 1, wts + a.o.resp_w, wts + a.o.resp_b, H, W, ACT_SIGMOID);
        __syncthreads();
    } else {
        float* r0 = a.r0buf + (long)b * KYS_R0 * HW;
        float* r1 = a.r1buf + (long)b * KYS_R1 * HW;
        kys_conv3(X, ci, r0, KYS_R0, wts + a.o.r0_w, wts + a.o.r0_b, H, W, ACT_RELU);
        __syncthreads();
        kys_conv3(r0, KYS_R0, r1, KYS_R1, wts + a.o.r1_w, wts + a.o.r1_b, H, W, ACT_RELU);
        __syncthreads();
        kys_conv3(r1, KYS_R1, f, 1, wts + a.o.resp_w, wts + a.o.resp_b, H, W, ACT_SIGMOID);
        __syncthreads();
    }
    const float* sc = X + KYS_SD * HW;
    float m0 = -INFINITY, m1 = -INFINITY;
    for (int p = tid; p < HW; p += nt) {
        float v = f[p];
        a.fused_orig[(long)b * HW + p] = v;
        if (a.has_thresh) v *= sc[p] > a.thresh ? 1.f : 0.f;
        if (a.window) v *= a.window[(long)b * a.window_stride + p];
        f[p] = v;
        m0 = fmaxf(m0, sc[p]);
        m1 = fmaxf(m1, v);
    }
    m0 = block_max(m0, red);
    m1 = block_max(m1, red);
    kys_store_shifted(f, a.response + (long)b * HW, H, W, a.shift);
    for (int p = tid; p < HW; p += nt) { Y[p] = sc[p]; Y[HW + p] = f[p]; Y[2 * HW + p] = m0; Y[3 * HW + p] = m1; }
    for (int i = tid; i < KYS_SD * HW; i += nt) Y[KYS_GI * HW + i] = X[i];
    __syncthreads();
    kys_conv3(Y, gi, R, KYS_SD, wts + a.o.gr_w, wts + a.o.gr_b, H, W, ACT_SIGMOID);
    kys_conv3(Y, gi, U, KYS_SD, wts + a.o.gu_w, wts + a.o.gu_b, H, W, ACT_SIGMOID);
    __syncthreads();
    for (int i = tid; i < KYS_SD * HW; i += nt) Y[KYS_GI * HW + i] = R[i] * X[i];
    __syncthreads();
    kys_conv3(Y, gi, R, KYS_SD, wts + a.o.gn_w, wts + a.o.gn_b, H, W, ACT_TANH);
    __syncthreads();
    for (int i = tid; i < KYS_SD * HW; i += nt) {
        const float u = U[i], s = (1.f - u) * X[i] + u * R[i];
        R[i] = s;
        a.state_cur[(long)b * KYS_SD * HW + i] = s;
    }
    __syncthreads();
    kys_is_target(R, t4, it, wts, a.o, H, W);
    kys_store_shifted(it, a.it_new + (long)b * HW, H, W, a.shift);
}

struct CvPlan { int kchunk, KS; };
CvPlan cv_plan(int C) {
    int kchunk = ((C + 7) / 8 + 3) / 4 * 4;                      // at most 8 K slices, each a multiple of 4 channels and >= 64
    if (kchunk < 64) kchunk = 64;
    return {kchunk, (C + kchunk - 1) / kchunk};
}

// The closed list of covered structures (include/pt_hot.h).  (64, 32) with entropy stays refused: tests/test_gpu_kys.py pins that.
bool kys_structure_ok(int state_dim, int r0, int r1, int gru_ksz, int conf) {
    if (state_dim != KYS_SD || gru_ksz != 3) return false;
    if (r0 == KYS_R0 && r1 == KYS_R1) return conf == PT_KYS_CONF_NONE || conf == PT_KYS_CONF_MAX;
    if (r0 == KYS_R16 && r1 == 0) return conf == PT_KYS_CONF_NONE || conf == PT_KYS_CONF_MAX || conf == PT_KYS_CONF_ENTROPY;
    return false;
}

}  // namespace

extern "C" size_t pt_kys_cost_volume_ws_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (long)H * W > PT_KYS_CV_MAX_HW) return 0;
    const long HW = (long)H * W;
    return (size_t)B * cv_plan(C).KS * HW * HW * sizeof(float);
}

extern "C" int pt_kys_cost_volume_f32(const float* feat_cur, const float* feat_prev, int B, int C, int H, int W, int kernel_size,
                                      int max_displacement, int stride, int remap, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!feat_cur || !feat_prev || !out || !ws) return PT_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || max_displacement < 1) return PT_ERR_SHAPE;
    if (kernel_size != 3 || stride != 1 || (long)H * W > PT_KYS_CV_MAX_HW || B > 1024 || max_displacement > 1024) return PT_ERR_UNSUPPORTED;
    const size_t need = pt_kys_cost_volume_ws_bytes(B, C, H, W);
    if (need >= ((size_t)1 << 31)) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < need) return PT_ERR_WORKSPACE;
    const int HW = H * W, D = 2 * max_displacement + 1;
    const long total = (long)B * (remap ? HW : D * D) * HW;
    if (total >= (1L << 31)) return PT_ERR_UNSUPPORTED;
    const CvPlan pl = cv_plan(C);
    const int zper = (pl.KS + 3) / 4, tiles = (HW + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_kys_gram, dim3(tiles, tiles, B * zper), dim3(256), 0, st, feat_cur, feat_prev, (float*)ws, C, HW, pl.kchunk, pl.KS, zper);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_kys_cv_taps, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)ws, out, H, W, max_displacement,
                       pl.KS, remap ? 1 : 0, total);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" size_t pt_kys_weight_floats(int state_dim, int rep_dim0, int rep_dim1, int gru_ksz, int with_conf) {
    if (!kys_structure_ok(state_dim, rep_dim0, rep_dim1, gru_ksz, with_conf)) return 0;
    return (size_t)kys_offsets(with_conf, rep_dim0, rep_dim1).total;
}

extern "C" size_t pt_kys_predict_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long)H * W > PT_KYS_PRED_MAX_HW) return 0;
    const size_t HW = (size_t)H * W;
    return (size_t)B * (HW * HW + (KYS_SD + 1 + KYS_R0 + KYS_R1) * HW) * sizeof(float);
}

extern "C" int pt_kys_predict_response_f32(const pt_kys_predict_params* p, const float* weights, const float* cost_volume,
                                           const float* state_prev, const float* label_prev, const float* dimp_score, const float* window,
                                           float* response, float* state_cur, float* propagation_weights, float* propagated_h,
                                           float* propagation_conf, float* fused_score_orig, float* is_target, float* is_target_after_prop,
                                           float* is_target_new, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !weights || !cost_volume || !dimp_score || !response || !state_cur || !propagation_weights || !propagated_h ||
        !fused_score_orig || !is_target || !is_target_after_prop || !is_target_new || !ws)
        return PT_ERR_NULL;
    if (!state_prev && !label_prev) return PT_ERR_NULL;
    if (p->with_conf && !propagation_conf) return PT_ERR_NULL;
    if (p->B <= 0 || p->H <= 0 || p->W <= 0) return PT_ERR_SHAPE;
    if (!kys_structure_ok(p->state_dim, p->rep_dim0, p->rep_dim1, p->gru_ksz, p->with_conf)) return PT_ERR_UNSUPPORTED;
    if ((long)p->H * p->W > PT_KYS_PRED_MAX_HW || p->B > 1024) return PT_ERR_UNSUPPORTED;
    if (p->weight_floats < pt_kys_weight_floats(p->state_dim, p->rep_dim0, p->rep_dim1, p->gru_ksz, p->with_conf)) return PT_ERR_SHAPE;
    const int B = p->B, H = p->H, W = p->W, HW = H * W;
    if (window && p->window_stride != 0 && p->window_stride != HW) return PT_ERR_SHAPE;
    if (ws_bytes < pt_kys_predict_ws_bytes(B, H, W)) return PT_ERR_WORKSPACE;
    const KysW o = kys_offsets(p->with_conf, p->rep_dim0, p->rep_dim1);
    const bool one = p->rep_dim1 == 0, ent = p->with_conf == PT_KYS_CONF_ENTROPY;
    float* z = (float*)ws;
    float* hbuf = z + (size_t)B * HW * HW;
    float* sbuf = hbuf + (size_t)B * KYS_SD * HW;
    float* r0 = sbuf + (size_t)B * HW;
    float* r1 = r0 + (size_t)B * KYS_R0 * HW;
    hipStream_t st = (hipStream_t)stream;
    KysPrep pa{weights, o, state_prev, label_prev, dimp_score, hbuf, sbuf, is_target, H, W, p->shift_px};
    hipLaunchKernelGGL(k_kys_prep, dim3(B), dim3(256), 0, st, pa);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_kys_cvproc, dim3(HW, B), dim3(256), 0, st, cost_volume, weights, o, z, H, W);
    PT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ent ? k_kys_propagate<true> : k_kys_propagate<false>, dim3((HW + 15) / 16, B), dim3(256), 0, st, (const float*)z,
                       (const float*)hbuf, propagation_weights, p->with_conf ? propagation_conf : nullptr, propagated_h, HW);
    PT_CHECK_LAUNCH();
    KysHead ha{weights, o, propagated_h, propagation_conf, sbuf, window, r0, r1, response, state_cur, fused_score_orig, is_target_after_prop,
               is_target_new, H, W, p->with_conf ? 1 : 0, p->has_thresh ? 1 : 0, p->window_stride, p->dimp_thresh, p->shift_px};
    hipLaunchKernelGGL(one ? k_kys_head<true> : k_kys_head<false>, dim3(B), dim3(1024), 0, st, ha);
    PT_CHECK_LAUNCH();
    return PT_OK;
}
