// Target-candidate matching (KeepTrack, reference: pytracking/tracker/keep_track/keep_track.py:437-475) on gfx950:
//   k_tcm_peaks          local maxima of a score map (ltr/data/processing_utils.py:669-705), bit-exact
//   k_tcm_desc           DescriptorExtractor.get_descriptors (target_candidate_matching.py:28-36) at the P requested points only:
//   k_tcm_desc_combine   an NT GEMM over K = C*16 (the 4x4xC patch of a point against the K-contiguous conv weight), K split over
//                        workgroups, the split partials summed in a fixed order by the second launch (no atomics)
//   k_tcm_kenc           SuperGlue keypoint encoder (superglue.py:109-117) + the descriptor add, both token sets in one launch
//   k_tcm_linear         1x1 convolutions of the GNN layers and the final projection (bias, folded BatchNorm, ReLU, residual)
//   k_tcm_attn           4-head attention of one GNN layer (superglue.py:120-139), head channels interleaved (c = 4*d + head)
//   k_tcm_sinkhorn       scores / 16, dustbins, log-Sinkhorn, Z - norm, mutual nearest check, threshold (superglue.py:183-216, 346-361)
// Weight pack of the matcher: include/pt_hot.h (pt_tcm_match_f32).
#include "common.h"
#include "pt_internal.h"

#define PT_TCM_MAP_MAX 64          // peaks: H, W <= 64 (one map per workgroup, held in LDS)
#define PT_TCM_DESC_KC 256         // descriptors: K per workgroup (16 channels x 4 x 4)
#define PT_TCM_DESC_PT 16          // descriptors: points per pass of a workgroup
#define PT_TCM_MAX_TOK PT_TCM_MAX_POINTS   // matcher: M, N <= 64
#define PT_TCM_D 256               // matcher: descriptor dim
#define PT_TCM_LIN_TT 16           // linear: tokens per workgroup
#define PT_TCM_LIN_KMAX 512

// ---------------------------------------------------------------------------------------------------------------------------
// Local maxima.  One workgroup per map.  m = max over the ks x ks window clipped to the map (F.max_pool2d pads with -inf, so
// padding never wins; a NaN in the window makes the max NaN as in PyTorch); hit = (v == m) & (v > th).  Hits are compacted in
// raster order by a ballot prefix sum, then each hit's output slot is its rank: the number of hits with a larger value, or the same
// value and a smaller raster index.  So the order is value-descending with ties in ascending raster order (the reference's argsort
// leaves the order of ties unspecified).
__global__ __launch_bounds__(1024) void k_tcm_peaks(const float* __restrict__ scores, int H, int W, int ks, float th,
                                                    int* __restrict__ count, long long* __restrict__ coords,
                                                    float* __restrict__ values) {
    __shared__ float m[PT_TCM_MAP_MAX * PT_TCM_MAP_MAX];
    __shared__ int hit[PT_TCM_MAP_MAX * PT_TCM_MAP_MAX];
    __shared__ int wcount[16];
    __shared__ int base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int HW = H * W, r = ks / 2;
    const float* s = scores + (long)b * HW;
    for (int i = tid; i < HW; i += 1024) m[i] = s[i];
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < HW; i0 += 1024) {
        const int i = i0 + tid;
        bool pk = false;
        if (i < HW) {
            const int y = i / W, x = i - (i / W) * W;
            const float v = m[i];
            float mx = -INFINITY;
            bool nan = false;
            for (int yy = max(y - r, 0); yy <= min(y + r, H - 1); ++yy)
                for (int xx = max(x - r, 0); xx <= min(x + r, W - 1); ++xx) {
                    const float w = m[yy * W + xx];
                    nan |= (w != w);
                    mx = fmaxf(mx, w);
                }
            pk = !nan && v == mx && v > th;
        }
        const unsigned long long bal = __ballot(pk);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[wid] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wid; ++w) off += wcount[w];
        if (pk) hit[off + pre] = i;
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < 16; ++w) tot += wcount[w];
            base += tot;
        }
        __syncthreads();
    }
    const int n = base;
    for (int j = tid; j < n; j += 1024) {
        const int idx = hit[j];
        const float v = m[idx];
        int rank = 0;
        for (int q = 0; q < n; ++q) {
            const float v2 = m[hit[q]];
            rank += (v2 > v) || (v2 == v && q < j);
        }
        const long o = (long)b * HW + rank;
        coords[2 * o] = idx / W;
        coords[2 * o + 1] = idx % W;
        values[o] = v;
    }
    if (tid == 0) count[b] = n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Descriptors at P points: part[ks][bp][d] = sum over this workgroup's K slice of W[d][k] * patch[bp][k],
//   k = c*16 + u*4 + v,  patch[bp][k] = x[b][c][y+u-2][x+v-2] (zero outside the map; the output map is (H+1) x (W+1)).
// grid (D/64, C/16): each workgroup streams 64 weight rows x 256 K (its slice of the 4*C*16*D-byte weight exactly once, held in
// registers), four waves over four 64-wide quarters of the slice, lane = output channel; the four wave partials are summed in a
// fixed order through LDS.  Points are processed PT_TCM_DESC_PT at a time from an LDS patch tile.
__global__ __launch_bounds__(256) void k_tcm_desc(const float* __restrict__ x, const float* __restrict__ wt,
                                                  const long long* __restrict__ coords, int C, int H, int W, int BP, int P, int D,
                                                  float* __restrict__ part) {
    __shared__ float patch[PT_TCM_DESC_PT][PT_TCM_DESC_KC];
    __shared__ float red[3][PT_TCM_DESC_PT][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int d = blockIdx.x * 64 + lane, ks = blockIdx.y, c0 = ks * 16;
    const f32x4* wrow = (const f32x4*)(wt + (long)d * C * 16 + (long)ks * PT_TCM_DESC_KC + w * 64);
    f32x4 wr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) wr[q] = wrow[q];
    for (int p0 = 0; p0 < BP; p0 += PT_TCM_DESC_PT) {
        const int np = min(PT_TCM_DESC_PT, BP - p0);
        __syncthreads();
        for (int e = tid; e < PT_TCM_DESC_PT * PT_TCM_DESC_KC; e += 256) {
            const int pp = e / PT_TCM_DESC_KC, kk = e % PT_TCM_DESC_KC;
            float val = 0.f;
            if (pp < np) {
                const int gp = p0 + pp, b = gp / P;
                const int yy = (int)coords[2 * gp] + ((kk >> 2) & 3) - 2, xx = (int)coords[2 * gp + 1] + (kk & 3) - 2;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) val = x[(((long)b * C + c0 + (kk >> 4)) * H + yy) * W + xx];
            }
            patch[pp][kk] = val;
        }
        __syncthreads();
        float acc[PT_TCM_DESC_PT];
#pragma unroll
        for (int pp = 0; pp < PT_TCM_DESC_PT; ++pp) acc[pp] = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
#pragma unroll
            for (int pp = 0; pp < PT_TCM_DESC_PT; ++pp) {
                const f32x4 pv = *(const f32x4*)&patch[pp][w * 64 + q * 4];
                acc[pp] = fmaf(wr[q].x, pv.x, acc[pp]);
                acc[pp] = fmaf(wr[q].y, pv.y, acc[pp]);
                acc[pp] = fmaf(wr[q].z, pv.z, acc[pp]);
                acc[pp] = fmaf(wr[q].w, pv.w, acc[pp]);
            }
        }
        if (w > 0) {
#pragma unroll
            for (int pp = 0; pp < PT_TCM_DESC_PT; ++pp) red[w - 1][pp][lane] = acc[pp];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int pp = 0; pp < PT_TCM_DESC_PT; ++pp)
                if (pp < np)
                    part[((long)ks * BP + p0 + pp) * D + d] = ((acc[pp] + red[0][pp][lane]) + red[1][pp][lane]) + red[2][pp][lane];
        }
    }
}

// out[b][d][p] = bias[d] + sum_{s < KS} part[s][b*P+p][d], s ascending
__global__ __launch_bounds__(256) void k_tcm_desc_combine(const float* __restrict__ part, const float* __restrict__ bias, int KS,
                                                          int BP, int P, int D, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)BP * D) return;
    const int gp = (int)(i / D), d = (int)(i % D);
    float s = 0.f;
    for (int k = 0; k < KS; ++k) s += part[((long)k * BP + gp) * D + d];
    const int b = gp / P, p = gp % P;
    out[((long)b * D + d) * P + p] = s + bias[d];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Matcher.  Activations are token-major: X[t][256], t < M side 0, M <= t < M+N side 1.

struct TcmKencArgs {
    const float* w;                    // pack offset 0: the five encoder layers
    const float *kp0, *kp1, *sc0, *sc1, *desc0, *desc1;
    float c0x, c0y, f0, c1x, c1y, f1;  // normalize_keypoints: (k - c) / f per side
    int M, N;
    float* X;
};

// one token per workgroup: in = ((k0 - cx) / f, (k1 - cy) / f, score) -> 32 -> 64 -> 128 -> 256 (folded BN + ReLU) -> 256;
// X[t][o] = desc[o][j] + enc[o]
__global__ __launch_bounds__(256) void k_tcm_kenc(TcmKencArgs a) {
    __shared__ float h[2][256];
    const int t = blockIdx.x, o = threadIdx.x;
    const bool s1 = t >= a.M;
    const int j = s1 ? t - a.M : t;
    if (o == 0) {
        const float* kp = s1 ? a.kp1 : a.kp0;
        h[0][0] = (kp[2 * j] - (s1 ? a.c1x : a.c0x)) / (s1 ? a.f1 : a.f0);
        h[0][1] = (kp[2 * j + 1] - (s1 ? a.c1y : a.c0y)) / (s1 ? a.f1 : a.f0);
        h[0][2] = (s1 ? a.sc1 : a.sc0)[j];
    }
    __syncthreads();
    const int dims[6] = {3, 32, 64, 128, 256, 256};
    const float* w = a.w;
    int cur = 0;
    for (int l = 0; l < 5; ++l) {
        const int I = dims[l], O = dims[l + 1];
        const float* bias = w + (long)O * I;
        if (o < O) {
            float acc = 0.f;
            for (int i = 0; i < I; ++i) acc = fmaf(w[(long)o * I + i], h[cur][i], acc);
            acc += bias[o];
            h[cur ^ 1][o] = l < 4 ? fmaxf(acc, 0.f) : acc;
        }
        w = bias + O;
        cur ^= 1;
        __syncthreads();
    }
    const float* desc = s1 ? a.desc1 : a.desc0;
    const int n = s1 ? a.N : a.M;
    a.X[(long)t * PT_TCM_D + o] = desc[(long)o * n + j] + h[cur][o];
}

struct TcmLinArgs {
    const float *W, *b;                // W (O, K0 + K1) row-major, b (O)
    const float *A0, *A1;              // input token rows: A0[t][0..K0) then A1[t][0..K1)
    int K0, K1, O, T, relu;
    const float* R;                    // optional residual R[t][o] (may equal Y: read and written by the same thread)
    float* Y;
};

// Y[t][o] = R[t][o] + act(b[o] + sum_k W[o][k] A[t][k]).  grid (O/64, ceil(T/16)): lane = output row o, wave w = tokens 4w..4w+3
// of the tile, the token rows in LDS (broadcast reads), the weight row in 16-byte loads.
__global__ __launch_bounds__(256) void k_tcm_linear(TcmLinArgs a) {
    __shared__ float xa[PT_TCM_LIN_TT][PT_TCM_LIN_KMAX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int o = blockIdx.x * 64 + lane, t0 = blockIdx.y * PT_TCM_LIN_TT;
    const int K = a.K0 + a.K1;
    for (int e = tid; e < PT_TCM_LIN_TT * K; e += 256) {
        const int tt = e / K, k = e % K, t = t0 + tt;
        float v = 0.f;
        if (t < a.T) v = k < a.K0 ? a.A0[(long)t * a.K0 + k] : a.A1[(long)t * a.K1 + k - a.K0];
        xa[tt][k] = v;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const f32x4* wr = (const f32x4*)(a.W + (long)o * K);
    for (int k4 = 0; k4 < K / 4; ++k4) {
        const f32x4 wv = wr[k4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 xv = *(const f32x4*)&xa[w * 4 + q][k4 * 4];
            acc[q] = fmaf(wv.x, xv.x, acc[q]);
            acc[q] = fmaf(wv.y, xv.y, acc[q]);
            acc[q] = fmaf(wv.z, xv.z, acc[q]);
            acc[q] = fmaf(wv.w, xv.w, acc[q]);
        }
    }
    const float bo = a.b[o];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = t0 + w * 4 + q;
        if (t >= a.T) continue;
        float y = acc[q] + bo;
        if (a.relu) y = fmaxf(y, 0.f);
        const long i = (long)t * a.O + o;
        if (a.R) y = a.R[i] + y;
        a.Y[i] = y;
    }
}

__device__ __forceinline__ float tcm_wave_max(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ float tcm_wave_sum(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// grid (T, 4 heads), one wave.  qkv[t] = (q[256], k[256], v[256]); head h owns channels 4*d + h (view(b, 64, 4, n)).
// Source tokens: the own side (self) or the other side (cross).  lane = source token for the scores and the softmax, then
// lane = d for the weighted sum; msg[t][4*d + h].
__global__ __launch_bounds__(64) void k_tcm_attn(const float* __restrict__ qkv, float* __restrict__ msg, int M, int N, int cross) {
    __shared__ float qs[64], pr[64];
    const int t = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int side = t >= M ? 1 : 0, src = cross ? 1 - side : side;
    const int s0 = src ? M : 0, ns = src ? N : M;
    qs[lane] = qkv[(long)t * 768 + 4 * lane + h];
    __syncthreads();
    float sc = -INFINITY;
    if (lane < ns) {
        const float* kr = qkv + (long)(s0 + lane) * 768 + 256 + h;
        float acc = 0.f;
        for (int d = 0; d < 64; ++d) acc = fmaf(qs[d], kr[4 * d], acc);
        sc = acc / 8.0f;
    }
    const float mx = tcm_wave_max(sc);
    const float e = lane < ns ? expf(sc - mx) : 0.f;
    const float sum = tcm_wave_sum(e);
    pr[lane] = e / sum;
    __syncthreads();
    const float* vr = qkv + (long)s0 * 768 + 512 + 4 * lane + h;
    float acc = 0.f;
    for (int m = 0; m < ns; ++m) acc = fmaf(pr[m], vr[(long)m * 768], acc);
    msg[(long)t * PT_TCM_D + 4 * lane + h] = acc;
}

struct TcmSinkArgs {
    const float* md;                   // (M+N, 256) final projections
    const float* bin_score;
    int M, N, iters;
    float thr;
    float* la;                         // (M+1, N+1)
    long long *m0, *m1;
    float *ms0, *ms1;
};

// logsumexp over one wave's operands (up to two per lane), torch.logsumexp's form: m = max (0 if infinite), log(sum exp(x - m)) + m
__device__ __forceinline__ float tcm_wave_lse(float x0, float x1) {
    float m = tcm_wave_max(fmaxf(x0, x1));
    if (isinf(m)) m = 0.f;
    const float s = tcm_wave_sum(expf(x0 - m) + expf(x1 - m));
    return logf(s) + m;
}

// one workgroup of 16 waves.  Z = [scores/16, bin; bin, bin]; u = v = 0; iters x (u = log_mu - lse_rows(Z + v),
// v = log_nu - lse_cols(Z + u)); Z' = Z + u + v - norm; row / column arg-max over the M x N block (first index on ties),
// mutual check, exp, threshold.
__global__ __launch_bounds__(1024) void k_tcm_sinkhorn(TcmSinkArgs a) {
    constexpr int LD = PT_TCM_MAX_TOK + 1;
    __shared__ float Z[LD * LD];
    __shared__ float u[LD], v[LD];
    __shared__ float rmax[PT_TCM_MAX_TOK];
    __shared__ int ridx[PT_TCM_MAX_TOK], cidx[PT_TCM_MAX_TOK], valid0[PT_TCM_MAX_TOK];
    __shared__ float msc0[PT_TCM_MAX_TOK];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int M = a.M, N = a.N, R = M + 1, Cc = N + 1;
    const float alpha = *a.bin_score;
    for (int e = tid; e < R * Cc; e += 1024) {
        const int i = e / Cc, j = e % Cc;
        float z = alpha;
        if (i < M && j < N) {
            const f32x4* p0 = (const f32x4*)(a.md + (long)i * PT_TCM_D);
            const f32x4* p1 = (const f32x4*)(a.md + (long)(M + j) * PT_TCM_D);
            float acc = 0.f;
            for (int q = 0; q < PT_TCM_D / 4; ++q) {
                const f32x4 x = p0[q], y = p1[q];
                acc = fmaf(x.x, y.x, acc);
                acc = fmaf(x.y, y.y, acc);
                acc = fmaf(x.z, y.z, acc);
                acc = fmaf(x.w, y.w, acc);
            }
            z = acc / 16.0f;
        }
        Z[i * LD + j] = z;
    }
    if (tid < LD) u[tid] = v[tid] = 0.f;
    const float norm = -logf((float)M + (float)N);
    const float mu_bin = logf((float)N) + norm, nu_bin = logf((float)M) + norm;
    __syncthreads();
    for (int it = 0; it < a.iters; ++it) {
        for (int i = wid; i < R; i += 16) {
            const float x0 = lane < Cc ? Z[i * LD + lane] + v[lane] : -INFINITY;
            const float x1 = lane + 64 < Cc ? Z[i * LD + lane + 64] + v[lane + 64] : -INFINITY;
            const float l = tcm_wave_lse(x0, x1);
            if (lane == 0) u[i] = (i < M ? norm : mu_bin) - l;
        }
        __syncthreads();
        for (int j = wid; j < Cc; j += 16) {
            const float x0 = lane < R ? Z[lane * LD + j] + u[lane] : -INFINITY;
            const float x1 = lane + 64 < R ? Z[(lane + 64) * LD + j] + u[lane + 64] : -INFINITY;
            const float l = tcm_wave_lse(x0, x1);
            if (lane == 0) v[j] = (j < N ? norm : nu_bin) - l;
        }
        __syncthreads();
    }
    for (int e = tid; e < R * Cc; e += 1024) {
        const int i = e / Cc, j = e % Cc;
        const float z = ((Z[i * LD + j] + u[i]) + v[j]) - norm;
        Z[i * LD + j] = z;
        a.la[e] = z;
    }
    __syncthreads();
    // arg-max: (value, index) reduced over the wave, the larger value or on equal values the smaller index
    for (int r = wid; r < M + N; r += 16) {
        const bool row = r < M;
        const int i = row ? r : r - M, n = row ? N : M;
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int q = lane; q < n; q += 64) {
            const float z = row ? Z[i * LD + q] : Z[q * LD + i];
            if (z > best || bi == 0x7fffffff) { best = z; bi = q; }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float ob = __shfl_xor(best, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            if (row) { rmax[i] = best; ridx[i] = bi; }
            else cidx[i] = bi;
        }
    }
    __syncthreads();
    if (tid < M) {
        const int j = ridx[tid];
        const bool mutual = cidx[j] == tid;
        const float s = mutual ? expf(rmax[tid]) : 0.f;
        const bool ok = mutual && s > a.thr;
        msc0[tid] = s;
        valid0[tid] = ok;
        a.ms0[tid] = s;
        a.m0[tid] = ok ? j : -1;
    }
    __syncthreads();
    if (tid < N) {
        const int i = cidx[tid];
        const bool mutual = ridx[i] == tid;
        a.ms1[tid] = mutual ? msc0[i] : 0.f;
        a.m1[tid] = (mutual && valid0[i]) ? i : -1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int pt_tcm_peaks_f32(const float* scores, int B, int H, int W, int ks, float th, int* count, long long* coords,
                                float* values, void* stream) {
    if (!scores || !count || !coords || !values) return PT_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || ks <= 0) return PT_ERR_SHAPE;
    if (ks % 2 == 0 || ks > 2 * PT_TCM_MAP_MAX - 1) return PT_ERR_UNSUPPORTED;
    if (H > PT_TCM_MAP_MAX || W > PT_TCM_MAP_MAX || B > 65535) return PT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_tcm_peaks, dim3(B), dim3(1024), 0, (hipStream_t)stream, scores, H, W, ks, th, count, coords, values);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

static size_t tcm_desc_part_floats(int B, int P, int C, int D) { return (size_t)(C / 16) * B * P * D; }

extern "C" size_t pt_tcm_desc_ws_bytes(int B, int P, int C, int D) {
    if (B <= 0 || P <= 0 || C <= 0 || D <= 0) return 0;
    return tcm_desc_part_floats(B, P, C, D) * sizeof(float);
}

extern "C" int pt_tcm_desc_f32(const float* x, const float* weight, const float* bias, const long long* coords, int B, int C, int H,
                               int W, int P, int D, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !weight || !bias || !coords || !out || !ws) return PT_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || D <= 0) return PT_ERR_SHAPE;
    if (C % 16 != 0 || D % 64 != 0 || C / 16 > 65535 || (long)B * P > (1L << 20)) return PT_ERR_UNSUPPORTED;
    if (((uintptr_t)weight & 15) != 0 || ((uintptr_t)ws & 15) != 0) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < pt_tcm_desc_ws_bytes(B, P, C, D)) return PT_ERR_WORKSPACE;
    float* part = (float*)ws;
    const int BP = B * P, KS = C / 16;
    hipLaunchKernelGGL(k_tcm_desc, dim3(D / 64, KS), dim3(256), 0, (hipStream_t)stream, x, weight, coords, C, H, W, BP, P, D, part);
    PT_CHECK_LAUNCH();
    const long n = (long)BP * D;
    hipLaunchKernelGGL(k_tcm_desc_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, bias, KS, BP,
                       P, D, out);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

static const size_t TCM_KENC_FLOATS = 32 * 3 + 32 + 64 * 32 + 64 + 128 * 64 + 128 + 256 * 128 + 256 + 256 * 256 + 256;
static const size_t TCM_LAYER_FLOATS = 768 * 256 + 768 + 256 * 256 + 256 + 512 * 512 + 512 + 256 * 512 + 256;
static const size_t TCM_FINAL_FLOATS = 256 * 256 + 256;

extern "C" size_t pt_tcm_match_weight_floats(int n_layers) {
    if (n_layers < 0) return 0;
    return TCM_KENC_FLOATS + (size_t)n_layers * TCM_LAYER_FLOATS + TCM_FINAL_FLOATS;
}

// workspace: X (T, 256), QKV (T, 768), MSG (T, 256), MRG (T, 256), H1 (T, 512), MD (T, 256)
extern "C" size_t pt_tcm_match_ws_bytes(const pt_tcm_match_params* p) {
    if (!p || p->M <= 0 || p->N <= 0) return 0;
    return (size_t)(p->M + p->N) * (256 + 768 + 256 + 256 + 512 + 256) * sizeof(float);
}

static int tcm_linear(const float* W, const float* b, const float* A0, int K0, const float* A1, int K1, int O, int T, int relu,
                      const float* R, float* Y, hipStream_t st) {
    TcmLinArgs a{W, b, A0, A1, K0, K1, O, T, relu, R, Y};
    hipLaunchKernelGGL(k_tcm_linear, dim3(O / 64, (T + PT_TCM_LIN_TT - 1) / PT_TCM_LIN_TT), dim3(256), 0, st, a);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" int pt_tcm_match_f32(const pt_tcm_match_params* p, const float* weights, const float* bin_score, const float* desc0,
                                const float* desc1, const float* kpts0, const float* kpts1, const float* scores0,
                                const float* scores1, float* log_assignment, long long* matches0, long long* matches1,
                                float* match_scores0, float* match_scores1, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !weights || !bin_score || !desc0 || !desc1 || !kpts0 || !kpts1 || !scores0 || !scores1 || !log_assignment ||
        !matches0 || !matches1 || !match_scores0 || !match_scores1 || !ws)
        return PT_ERR_NULL;
    if (p->M <= 0 || p->N <= 0 || p->n_layers < 0 || p->sinkhorn_iters < 0) return PT_ERR_SHAPE;
    if (p->M > PT_TCM_MAX_TOK || p->N > PT_TCM_MAX_TOK || p->n_layers > PT_TCM_MAX_LAYERS || p->sinkhorn_iters > 100000)
        return PT_ERR_UNSUPPORTED;
    if (p->weight_floats < pt_tcm_match_weight_floats(p->skip_gnn ? 0 : p->n_layers)) return PT_ERR_SHAPE;
    if (((uintptr_t)weights & 15) != 0 || ((uintptr_t)ws & 15) != 0) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < pt_tcm_match_ws_bytes(p)) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int M = p->M, N = p->N, T = M + N;
    float* X = (float*)ws;
    float* QKV = X + (size_t)T * 256;
    float* MSG = QKV + (size_t)T * 768;
    float* MRG = MSG + (size_t)T * 256;
    float* H1 = MRG + (size_t)T * 256;
    float* MD = H1 + (size_t)T * 512;
    TcmKencArgs ka{weights, kpts0, kpts1, scores0, scores1, desc0, desc1,
                   p->kpt_center0[0], p->kpt_center0[1], p->kpt_scale0, p->kpt_center1[0], p->kpt_center1[1], p->kpt_scale1, M, N, X};
    hipLaunchKernelGGL(k_tcm_kenc, dim3(T), dim3(256), 0, st, ka);
    PT_CHECK_LAUNCH();
    const float* w = weights + TCM_KENC_FLOATS;
    const int L = p->skip_gnn ? 0 : p->n_layers;
    for (int l = 0; l < L; ++l) {
        const float *Wqkv = w, *bqkv = Wqkv + 768 * 256, *Wm = bqkv + 768, *bm = Wm + 256 * 256, *W1 = bm + 256, *b1 = W1 + 512 * 512,
                    *W2 = b1 + 512, *b2 = W2 + 256 * 512;
        int rc = tcm_linear(Wqkv, bqkv, X, 256, nullptr, 0, 768, T, 0, nullptr, QKV, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_tcm_attn, dim3(T, 4), dim3(64), 0, st, QKV, MSG, M, N, (int)((p->layer_types >> l) & 1u));
        PT_CHECK_LAUNCH();
        if ((rc = tcm_linear(Wm, bm, MSG, 256, nullptr, 0, 256, T, 0, nullptr, MRG, st))) return rc;
        if ((rc = tcm_linear(W1, b1, X, 256, MRG, 256, 512, T, 1, nullptr, H1, st))) return rc;
        if ((rc = tcm_linear(W2, b2, H1, 512, nullptr, 0, 256, T, 0, X, X, st))) return rc;
        w += TCM_LAYER_FLOATS;
    }
    int rc = tcm_linear(w, w + 256 * 256, X, 256, nullptr, 0, 256, T, 0, nullptr, MD, st);
    if (rc) return rc;
    TcmSinkArgs sa{MD, bin_score, M, N, p->sinkhorn_iters, p->filter_threshold, log_assignment, matches0, matches1, match_scores0,
                   match_scores1};
    hipLaunchKernelGGL(k_tcm_sinkhorn, dim3(1), dim3(1024), 0, st, sa);
    PT_CHECK_LAUNCH();
    return PT_OK;
}
