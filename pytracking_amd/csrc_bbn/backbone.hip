// libpt_bbn.so: the ResNet backbone forward of the trackers (include/pt_bbn.h).
//
//   k_conv<BM, STEM>  implicit GEMM over tokens on v_mfma_f32_16x16x4_f32: BM x 64 output tile per workgroup of 4 waves (2 x 2), K in steps
//                     of 32 through double-buffered LDS (one barrier per step, the next step's global loads in flight over the MFMAs).
//                     Operand A is gathered from the tokens x channels activation of the previous layer (16 bytes = 4 input channels of
//                     one tap per load; a tap outside its image is an out-of-range buffer offset, which the hardware answers with 0), so a
//                     tile that spans two images takes each pixel's halo from that pixel's own image.  STEM: the 7x7 gather from the NCHW
//                     input, one scalar load per K index.
//   k_reduce          sums the K-split partial tiles in the order z = 0, 1, ... and applies the epilogue.
//   k_pool            3/2/1 max-pool on tokens x channels; the input is post-ReLU, so padding with 0 equals padding with -inf.
//
// Every load and store of a kernel goes through a buffer resource whose size is the exact size of the view: an index that left the view
// would read 0 or be dropped.  The host checks every view against PT_BBN_MAX_VIEW_BYTES (32-bit byte offsets).
#include <vector>
#include "../csrc/common.h"
#include "../../include/pt_bbn.h"

#define PT_BBN_CHECK_LAUNCH()                                          \
    do {                                                               \
        if (hipGetLastError() != hipSuccess) return PT_BBN_ERR_LAUNCH; \
    } while (0)

namespace {

constexpr unsigned OOB = 0xFFFFFFF0u;
constexpr int BN = 64, BK = 32, LS = BK + 4, THREADS = 256;

struct ConvArgs {
    const float* A; unsigned a_bytes;          // tokens x Cin activation (STEM: the NCHW input)
    const float* Wt; unsigned w_bytes;         // (N, K)
    const float* scale; const float* shift;    // (N)
    const float* R;                            // residual, tokens x N, or null
    float* Y; unsigned y_bytes;                // tokens x N (split: gridDim.z partial matrices of M x N), or null
    float* O; unsigned o_bytes;                // NCHW output, or null
    int M, N, K, Cin, H, W, Ho, Wo, ks, stride, pad, relu, ksteps;
};

__device__ __forceinline__ void bstore1(float v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, 0);
}
__device__ __forceinline__ void bstore4(f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, 0, 0);
}

// what every output element goes through, in k_conv and in k_reduce alike
__device__ __forceinline__ float epilogue(float acc, float sc, float sh, float res, int relu) {
    const float v = __builtin_fmaf(acc, sc, sh) + res;
    return relu ? fmaxf(v, 0.f) : v;
}

template <int BM, bool STEM>
__global__ __launch_bounds__(THREADS) void k_conv(ConvArgs g) {
    constexpr int AL = BM / 32, BL = BN / 32, MT = BM / 32, NT = 2;      // loader rows per thread; 16 x 16 fragments per wave
    __shared__ __attribute__((aligned(16))) float As[2][BM * LS];
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, z = blockIdx.z;
    const int lrow = tid >> 3, lq = (tid & 7) * 4;                        // loader: 8 threads x 16 bytes cover one row of a K-step
    const __amdgpu_buffer_rsrc_t rsA = pt_rsrc(g.A, g.a_bytes), rsW = pt_rsrc(g.Wt, g.w_bytes);
    const int HWo = g.Ho * g.Wo;

    int iy0[AL], ix0[AL];
    unsigned ibase[AL];                                                   // first element of the row's image
    unsigned woff[BL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int row = m0 + lrow + 32 * i;
        const int rc = min(row, g.M - 1);
        const int img = rc / HWo, p = rc - img * HWo, oy = p / g.Wo, ox = p - oy * g.Wo;
        iy0[i] = row < g.M ? oy * g.stride - g.pad : -(1 << 20);          // a row outside the matrix: every tap falls outside the map
        ix0[i] = ox * g.stride - g.pad;
        ibase[i] = (unsigned)img * (unsigned)(g.H * g.W) * (unsigned)(STEM ? 3 : g.Cin);
    }
#pragma unroll
    for (int i = 0; i < BL; ++i) {
        const int n = n0 + lrow + 32 * i;
        woff[i] = n < g.N ? (unsigned)n * (unsigned)g.K * 4u : OOB;
    }

    f32x4 ra[AL], rb[BL];
    auto fetch = [&](int kt) {
        const int k = kt * BK + lq;
        const bool kin = k < g.K;
        if constexpr (!STEM) {
            const int tap = k / g.Cin, c = k - tap * g.Cin, dy = tap / g.ks, dx = tap - dy * g.ks;
#pragma unroll
            for (int i = 0; i < AL; ++i) {
                const int iy = iy0[i] + dy, ix = ix0[i] + dx;
                const bool in = kin && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                const unsigned off = (ibase[i] + (unsigned)(iy * g.W + ix) * (unsigned)g.Cin + (unsigned)c) * 4u;
                ra[i] = pt_bload4(rsA, in ? off : OOB);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = k + e, c = kk / 49, r = kk - c * 49, dy = r / 7, dx = r - dy * 7;
#pragma unroll
                for (int i = 0; i < AL; ++i) {
                    const int iy = iy0[i] + dy, ix = ix0[i] + dx;
                    const bool in = c < 3 && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                    const unsigned off = (ibase[i] + (unsigned)((c * g.H + iy) * g.W + ix)) * 4u;
                    ra[i][e] = pt_bload1(rsA, in ? off : OOB);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) rb[i] = pt_bload4(rsW, (kin && woff[i] != OOB) ? woff[i] + (unsigned)k * 4u : OOB);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AL; ++i) *reinterpret_cast<f32x4*>(&As[buf][(lrow + 32 * i) * LS + lq]) = ra[i];
#pragma unroll
        for (int i = 0; i < BL; ++i) *reinterpret_cast<f32x4*>(&Bs[buf][(lrow + 32 * i) * LS + lq]) = rb[i];
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ktotal = (g.K + BK - 1) / BK;
    const int kbeg = z * g.ksteps, kend = min(kbeg + g.ksteps, ktotal);
    fetch(kbeg);
    stage(0);
    __syncthreads();
    // Lane (i, kq) reads 16 bytes of row i per half step: K indices h * 16 + kq * 4 + e, e = 0..3, and MFMA e takes element e of both
    // operands: a permutation of K inside the step, the same one for A and B.
    const int arow = (wm * (BM / 2) + (lane & 15)) * LS + (lane >> 4) * 4, brow = (wn * 32 + (lane & 15)) * LS + (lane >> 4) * 4;
    for (int kt = kbeg; kt < kend; ++kt) {
        const int buf = (kt - kbeg) & 1;
        if (kt + 1 < kend) fetch(kt + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 a[MT], b[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(&As[buf][arow + mt * 16 * LS + h * 16]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = *reinterpret_cast<const f32x4*>(&Bs[buf][brow + nt * 16 * LS + h * 16]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(a[mt][e], b[nt][e], acc[mt][nt]);
        }
        if (kt + 1 < kend) stage(buf ^ 1);
        __syncthreads();
    }

    // lane (kq, j) holds rows 4 kq + r, r = 0..3, of column j of every 16 x 16 fragment
    const bool split = gridDim.z > 1;
    const __amdgpu_buffer_rsrc_t rsY = pt_rsrc(g.Y ? g.Y : g.O, g.Y ? g.y_bytes : 0u), rsO = pt_rsrc(g.O ? g.O : g.Y, g.O ? g.o_bytes : 0u);
    const __amdgpu_buffer_rsrc_t rsR = pt_rsrc(g.R ? g.R : g.A, g.R ? g.y_bytes : 0u);
    const unsigned zoff = split ? (unsigned)z * (unsigned)g.M * (unsigned)g.N * 4u : 0u;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + wn * 32 + nt * 16 + (lane & 15);
        const bool cok = col < g.N;
        const float sc = (cok && !split) ? g.scale[col] : 0.f, sh = (cok && !split) ? g.shift[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row0 = m0 + wm * (BM / 2) + mt * 16 + 4 * (lane >> 4);
            float res[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = cok && row0 + r < g.M;
                res[r] = pt_bload1(rsR, ok ? ((unsigned)(row0 + r) * (unsigned)g.N + (unsigned)col) * 4u : OOB);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + r;
                const bool ok = cok && row < g.M;
                const unsigned yoff = ok ? ((unsigned)row * (unsigned)g.N + (unsigned)col) * 4u + zoff : OOB;
                if (split) {
                    bstore1(acc[mt][nt][r], rsY, yoff);
                } else {
                    const float v = epilogue(acc[mt][nt][r], sc, sh, res[r], g.relu);
                    bstore1(v, rsY, yoff);
                    const int rc = min(row, g.M - 1), img = rc / HWo, p = rc - img * HWo;
                    bstore1(v, rsO, ok ? (((unsigned)img * (unsigned)g.N + (unsigned)col) * (unsigned)HWo + (unsigned)p) * 4u : OOB);
                }
            }
        }
    }
}

struct ReduceArgs {
    const float* P; unsigned p_bytes;          // split partial matrices of M x N
    const float* scale; const float* shift; const float* R;
    float* Y; unsigned y_bytes; float* O; unsigned o_bytes;
    int M, N, HWo, split, relu;
};

// one thread per 4 consecutive channels of a token
__global__ __launch_bounds__(THREADS) void k_reduce(ReduceArgs g) {
    const unsigned q = blockIdx.x * THREADS + threadIdx.x, nq = (unsigned)g.N / 4u;
    const unsigned row = q / nq, c4 = (q - row * nq) * 4u;
    if (row >= (unsigned)g.M) return;
    const __amdgpu_buffer_rsrc_t rsP = pt_rsrc(g.P, g.p_bytes), rsY = pt_rsrc(g.Y ? g.Y : g.O, g.Y ? g.y_bytes : 0u),
                                 rsO = pt_rsrc(g.O ? g.O : g.Y, g.O ? g.o_bytes : 0u), rsR = pt_rsrc(g.R ? g.R : g.P, g.R ? g.y_bytes : 0u);
    const unsigned off = (row * (unsigned)g.N + c4) * 4u, zstride = (unsigned)g.M * (unsigned)g.N * 4u;
    f32x4 s = pt_bload4(rsP, off);
    for (int z = 1; z < g.split; ++z) s += pt_bload4(rsP, off + (unsigned)z * zstride);
    const f32x4 res = pt_bload4(rsR, off);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(g.scale + c4), sh = *reinterpret_cast<const f32x4*>(g.shift + c4);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = epilogue(s[e], sc[e], sh[e], res[e], g.relu);
    bstore4(v, rsY, off);
    const unsigned img = row / (unsigned)g.HWo, p = row - img * (unsigned)g.HWo;
#pragma unroll
    for (int e = 0; e < 4; ++e) bstore1(v[e], rsO, ((img * (unsigned)g.N + c4 + e) * (unsigned)g.HWo + p) * 4u);
}

struct PoolArgs {
    const float* A; unsigned a_bytes; float* Y; unsigned y_bytes; float* O; unsigned o_bytes;
    int M, C, H, W, Ho, Wo;
};

// one thread per 4 consecutive channels of an output token
__global__ __launch_bounds__(THREADS) void k_pool(PoolArgs g) {
    const unsigned q = blockIdx.x * THREADS + threadIdx.x, nq = (unsigned)g.C / 4u;
    const unsigned row = q / nq, c4 = (q - row * nq) * 4u;
    if (row >= (unsigned)g.M) return;
    const __amdgpu_buffer_rsrc_t rsA = pt_rsrc(g.A, g.a_bytes), rsY = pt_rsrc(g.Y, g.y_bytes), rsO = pt_rsrc(g.O ? g.O : g.Y, g.O ? g.o_bytes : 0u);
    const int HWo = g.Ho * g.Wo, img = (int)row / HWo, p = (int)row - img * HWo, oy = p / g.Wo, ox = p - oy * g.Wo;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};                                      // the input is >= 0 (post-ReLU): 0 is the padding's -inf
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int iy = 2 * oy - 1 + dy, ix = 2 * ox - 1 + dx;
            const bool in = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const f32x4 t = pt_bload4(rsA, in ? (((unsigned)img * (unsigned)(g.H * g.W) + (unsigned)(iy * g.W + ix)) * (unsigned)g.C + c4) * 4u : OOB);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], t[e]);
        }
    bstore4(v, rsY, (row * (unsigned)g.C + c4) * 4u);
#pragma unroll
    for (int e = 0; e < 4; ++e) bstore1(v[e], rsO, (((unsigned)img * (unsigned)g.C + c4 + e) * (unsigned)HWo + (unsigned)p) * 4u);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: the one walk that the pack layout, the plan query, the workspace size and the forward all read
// ---------------------------------------------------------------------------------------------------------------------------------
enum { B_X = 0, B_Y = 1, B_T1 = 2, B_T2 = 3, B_D = 4, B_COUNT = 5, B_INPUT = -1, B_NONE = -2 };

struct Op {
    pt_bbn_launch pub;
    int in, out, res;                 // workspace buffers (B_*); a reduce reads the partial area
    int Cin;
    size_t w_off, s_off;              // weights and scale in the pack (shift = scale + N)
};

struct Walk {
    std::vector<Op> ops;
    size_t pack_floats = 0, act_floats = 0, part_floats = 0;
    int C[PT_BBN_OUT_COUNT], Ho[PT_BBN_OUT_COUNT], Wo[PT_BBN_OUT_COUNT];
};

bool desc_ok(const pt_bbn_desc* d) {
    if (d->block != PT_BBN_BASIC && d->block != PT_BBN_BOTTLENECK) return false;
    if (d->inplanes < 8 || d->inplanes > PT_BBN_MAX_INPLANES || d->inplanes % 8) return false;
    for (int l = 0; l < 4; ++l)
        if (d->blocks[l] < 1 || d->blocks[l] > PT_BBN_MAX_BLOCKS || (d->stride[l] != 1 && d->stride[l] != 2)) return false;
    if (d->stride_conv != 1 && d->stride_conv != 2) return false;
    if (d->block == PT_BBN_BASIC && d->stride_conv != 1) return false;
    return d->conv1_after_pool == 0 || d->conv1_after_pool == 1;
}

// tile and K-split of one convolution (include/pt_bbn.h, "Launch filling")
void pick(pt_bbn_launch& r, bool stem) {
    const int nt = pt_ceil_div(r.N, BN), ktotal = pt_ceil_div(r.K, BK);
    r.split = 1;
    if (stem) {
        r.bm = 64;
        r.route = PT_BBN_R_STEM;
    } else {
        r.bm = 32;
        r.route = PT_BBN_R_T32;
        for (int bm = 128; bm >= 64; bm /= 2)
            if ((long)pt_ceil_div(r.M, bm) * nt >= PT_BBN_FILL_WGS) {
                r.bm = bm;
                r.route = bm == 128 ? PT_BBN_R_T128 : PT_BBN_R_T64;
                break;
            }
        if (r.bm == 32) {
            const long wgs = (long)pt_ceil_div(r.M, 32) * nt;
            while (r.split < 8 && wgs * r.split * 2 <= PT_BBN_FILL_WGS && ktotal / (r.split * 2) >= PT_BBN_MIN_KSTEPS) r.split *= 2;
            r.route = r.split == 1 ? PT_BBN_R_T32 : r.split == 2 ? PT_BBN_R_T32_S2 : r.split == 4 ? PT_BBN_R_T32_S4 : PT_BBN_R_T32_S8;
        }
    }
    r.ksteps = pt_ceil_div(ktotal, r.split);
    r.grid_x = pt_ceil_div(r.M, r.bm);
    r.grid_y = nt;
    r.grid_z = r.split;
}

// -> PT_BBN_OK or a status; `w` is complete only on PT_BBN_OK
int walk(const pt_bbn_desc* d, int n, int H, int W, int mask, Walk& w) {
    if (!d) return PT_BBN_ERR_NULL;
    if (n < 1 || H < 1 || W < 1 || mask < 1 || mask >= (1 << PT_BBN_OUT_COUNT)) return PT_BBN_ERR_SHAPE;
    if (!desc_ok(d)) return PT_BBN_ERR_UNSUPPORTED;
    if ((double)n * 3.0 * H * W * 4.0 > (double)PT_BBN_MAX_VIEW_BYTES) return PT_BBN_ERR_UNSUPPORTED;
    bool fits = true;
    auto view = [&](double floats) { fits = fits && floats * 4.0 <= (double)PT_BBN_MAX_VIEW_BYTES; };
    auto out_of = [&](int o, int C, int Ho, int Wo) { w.C[o] = C; w.Ho[o] = Ho; w.Wo[o] = Wo; };
    int deepest = 0;
    for (int o = 0; o < PT_BBN_OUT_COUNT; ++o)
        if (mask >> o & 1) deepest = o;
    const int exp = d->block == PT_BBN_BOTTLENECK ? 4 : 1;

    auto conv = [&](int layer, int block, int cv, int in, int out, int res, int Cin, int Cout, int ks, int stride, int Hin, int Win, int relu,
                    int o, bool emit) {
        const int K = layer == 0 ? PT_BBN_STEM_K : ks * ks * Cin;
        const size_t w_off = w.pack_floats;
        w.pack_floats += (size_t)Cout * K + 2 * (size_t)Cout;
        const int Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
        if (!emit) return;
        Op op = {};
        pt_bbn_launch& r = op.pub;
        r.kernel = layer == 0 ? PT_BBN_K_STEM : PT_BBN_K_CONV;
        r.layer = layer; r.block = block; r.conv = cv;
        const double M = (double)n * Ho * Wo;
        view(M * Cout);
        view((double)Cout * K);
        if (!fits) return;
        r.M = (int)M; r.N = Cout; r.K = K;
        r.Hin = Hin; r.Win = Win; r.Hout = Ho; r.Wout = Wo; r.ksize = ks; r.stride = stride;
        r.residual = res != B_NONE; r.relu = relu; r.out = o;
        pick(r, layer == 0);
        view(M * Cout * r.split);
        if (!fits) return;
        op.in = in; op.out = out; op.res = res; op.Cin = Cin; op.w_off = w_off; op.s_off = w_off + (size_t)Cout * K;
        w.act_floats = std::max(w.act_floats, (size_t)r.M * Cout);
        if (r.split > 1) {
            w.part_floats = std::max(w.part_floats, (size_t)r.M * Cout * r.split);
            Op red = op;
            r.residual = 0; r.relu = 0; r.out = -1;                       // the split launch leaves the epilogue to the reduction
            pt_bbn_launch& q = red.pub;
            q.kernel = PT_BBN_K_REDUCE; q.route = PT_BBN_R_REDUCE;
            q.bm = 0; q.ksteps = 0;
            q.grid_x = pt_ceil_div(q.M * (q.N / 4), THREADS); q.grid_y = 1; q.grid_z = 1;
            w.ops.push_back(op);
            w.ops.push_back(red);
        } else {
            w.ops.push_back(op);
        }
    };

    // stem and pool
    const int H1 = (H - 1) / 2 + 1, W1 = (W - 1) / 2 + 1, Hp = (H1 - 1) / 2 + 1, Wp = (W1 - 1) / 2 + 1, C0 = d->inplanes;
    const bool want0 = mask & 1;
    conv(0, 0, 1, B_INPUT, B_T1, B_NONE, 3, C0, 7, 2, H, W, 1, (want0 && !d->conv1_after_pool) ? PT_BBN_OUT_CONV1 : -1, true);
    if (!fits) return PT_BBN_ERR_UNSUPPORTED;
    if (d->conv1_after_pool) out_of(0, C0, Hp, Wp); else out_of(0, C0, H1, W1);
    const bool pool = deepest > 0 || d->conv1_after_pool;
    if (pool) {
        Op op = {};
        pt_bbn_launch& r = op.pub;
        r.kernel = PT_BBN_K_POOL; r.route = PT_BBN_R_POOL;
        r.M = n * Hp * Wp; r.N = C0; r.K = 9;
        r.Hin = H1; r.Win = W1; r.Hout = Hp; r.Wout = Wp; r.ksize = 3; r.stride = 2; r.split = 1;
        r.out = (want0 && d->conv1_after_pool) ? PT_BBN_OUT_CONV1 : -1;
        r.grid_x = pt_ceil_div(r.M * (C0 / 4), THREADS); r.grid_y = 1; r.grid_z = 1;
        op.in = B_T1; op.out = B_X; op.res = B_NONE; op.Cin = C0;
        w.ops.push_back(op);
    }
    int C = C0, Hc = Hp, Wc = Wp, cur = B_X, other = B_Y;
    for (int L = 1; L <= 4; ++L) {
        const bool emit = L <= deepest;
        const int planes = C0 << (L - 1), Cout = planes * exp;
        for (int b = 0; b < d->blocks[L - 1]; ++b) {
            const int stride = b == 0 ? d->stride[L - 1] : 1;
            const bool ds = b == 0 && (stride != 1 || C != Cout);
            const int Hn = (Hc - 1) / stride + 1, Wn = (Wc - 1) / stride + 1;
            const int o = (b == d->blocks[L - 1] - 1 && (mask >> L & 1)) ? L : -1;
            const int res = ds ? B_D : cur;
            if (d->block == PT_BBN_BOTTLENECK) {
                const int s1 = d->stride_conv == 1 ? stride : 1, s2 = d->stride_conv == 2 ? stride : 1;
                const int Ha = (Hc - 1) / s1 + 1, Wa = (Wc - 1) / s1 + 1;
                conv(L, b, 1, cur, B_T1, B_NONE, C, planes, 1, s1, Hc, Wc, 1, -1, emit);
                conv(L, b, 2, B_T1, B_T2, B_NONE, planes, planes, 3, s2, Ha, Wa, 1, -1, emit);
                // pack order conv1, conv2, conv3, downsample; launch order: the downsample in front of conv3, which adds it
                const size_t at = w.pack_floats;
                w.pack_floats += (size_t)Cout * planes + 2 * (size_t)Cout;
                if (ds) conv(L, b, 0, cur, B_D, B_NONE, C, Cout, 1, stride, Hc, Wc, 0, -1, emit);
                const size_t end = w.pack_floats;
                w.pack_floats = at;
                conv(L, b, 3, B_T2, other, res, planes, Cout, 1, 1, Hn, Wn, 1, o, emit);
                w.pack_floats = end;
            } else {
                conv(L, b, 1, cur, B_T1, B_NONE, C, planes, 3, stride, Hc, Wc, 1, -1, emit);
                const size_t at = w.pack_floats;
                w.pack_floats += (size_t)Cout * 9 * planes + 2 * (size_t)Cout;
                if (ds) conv(L, b, 0, cur, B_D, B_NONE, C, Cout, 1, stride, Hc, Wc, 0, -1, emit);
                const size_t end = w.pack_floats;
                w.pack_floats = at;
                conv(L, b, 2, B_T1, other, res, planes, Cout, 3, 1, Hn, Wn, 1, o, emit);
                w.pack_floats = end;
            }
            if (!fits) return PT_BBN_ERR_UNSUPPORTED;
            std::swap(cur, other);
            C = Cout; Hc = Hn; Wc = Wn;
        }
        out_of(L, C, Hc, Wc);
    }
    if ((int)w.ops.size() > PT_BBN_MAX_LAUNCHES) return PT_BBN_ERR_UNSUPPORTED;
    return PT_BBN_OK;
}

size_t align64(size_t floats) { return (floats + 63) & ~(size_t)63; }

template <int BM, bool STEM>
void launch_conv(const ConvArgs& a, const pt_bbn_launch& r, hipStream_t st) {
    hipLaunchKernelGGL((k_conv<BM, STEM>), dim3(r.grid_x, r.grid_y, r.grid_z), dim3(THREADS), 0, st, a);
}

}  // namespace

extern "C" const char* pt_bbn_strerror(int status) {
    switch (status) {
        case PT_BBN_OK: return "ok";
        case PT_BBN_ERR_NULL: return "required pointer is NULL";
        case PT_BBN_ERR_SHAPE: return "non-positive dimension or empty / unknown output mask";
        case PT_BBN_ERR_UNSUPPORTED: return "request outside the limits of include/pt_bbn.h";
        case PT_BBN_ERR_WORKSPACE: return "workspace too small or misaligned";
        case PT_BBN_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown status";
    }
}

extern "C" int pt_bbn_abi_version(void) { return 1; }

extern "C" size_t pt_bbn_pack_floats(const pt_bbn_desc* desc) {
    Walk w;
    return walk(desc, 1, 32, 32, 1, w) == PT_BBN_OK ? w.pack_floats : 0;
}

extern "C" size_t pt_bbn_ws_bytes(const pt_bbn_desc* desc, int n, int H, int W, int out_mask) {
    Walk w;
    if (walk(desc, n, H, W, out_mask, w) != PT_BBN_OK) return 0;
    return (B_COUNT * align64(w.act_floats) + align64(w.part_floats)) * sizeof(float);
}

extern "C" int pt_bbn_plan(const pt_bbn_desc* desc, int n, int H, int W, int out_mask, pt_bbn_launch* rows) {
    Walk w;
    const int rc = walk(desc, n, H, W, out_mask, w);
    if (rc != PT_BBN_OK) return rc;
    if (rows)
        for (size_t i = 0; i < w.ops.size(); ++i) rows[i] = w.ops[i].pub;
    return (int)w.ops.size();
}

extern "C" int pt_bbn_forward_f32(const pt_bbn_desc* desc, const float* pack, const float* x, int n, int H, int W, int out_mask,
                                  float* const outs[5], void* ws, size_t ws_bytes, void* stream) {
    if (!desc || !pack || !x || !outs || !ws) return PT_BBN_ERR_NULL;
    Walk w;
    const int rc = walk(desc, n, H, W, out_mask, w);
    if (rc != PT_BBN_OK) return rc;
    for (int o = 0; o < PT_BBN_OUT_COUNT; ++o)
        if ((out_mask >> o & 1) && !outs[o]) return PT_BBN_ERR_NULL;
    const size_t act = align64(w.act_floats);
    if (((uintptr_t)ws % 256) != 0 || ((uintptr_t)pack % 16) != 0 || ws_bytes < (B_COUNT * act + align64(w.part_floats)) * sizeof(float))
        return PT_BBN_ERR_WORKSPACE;
    float* base = (float*)ws;
    float* part = base + B_COUNT * act;
    hipStream_t st = (hipStream_t)stream;
    auto bytes = [](size_t floats) { return (unsigned)(floats * 4); };
    for (const Op& op : w.ops) {
        const pt_bbn_launch& r = op.pub;
        float* O = r.out >= 0 ? outs[r.out] : nullptr;
        const size_t mn = (size_t)r.M * r.N;
        if (r.kernel == PT_BBN_K_POOL) {
            PoolArgs a = {base + op.in * act, bytes((size_t)n * r.Hin * r.Win * r.N), base + op.out * act, bytes(mn), O, bytes(O ? mn : 0),
                          r.M, r.N, r.Hin, r.Win, r.Hout, r.Wout};
            hipLaunchKernelGGL(k_pool, dim3(r.grid_x), dim3(THREADS), 0, st, a);
        } else if (r.kernel == PT_BBN_K_REDUCE) {
            ReduceArgs a = {part, bytes(mn * r.split), pack + op.s_off, pack + op.s_off + r.N, op.res == B_NONE ? nullptr : base + op.res * act,
                            base + op.out * act, bytes(mn), O, bytes(O ? mn : 0), r.M, r.N, r.Hout * r.Wout, r.split, r.relu};
            hipLaunchKernelGGL(k_reduce, dim3(r.grid_x), dim3(THREADS), 0, st, a);
        } else {
            const bool stem = r.kernel == PT_BBN_K_STEM, split = r.split > 1;
            ConvArgs a = {};
            a.A = stem ? x : base + op.in * act;
            a.a_bytes = bytes((size_t)n * r.Hin * r.Win * op.Cin);
            a.Wt = pack + op.w_off; a.w_bytes = bytes((size_t)r.N * r.K);
            a.scale = pack + op.s_off; a.shift = pack + op.s_off + r.N;
            a.R = (split || op.res == B_NONE) ? nullptr : base + op.res * act;
            a.Y = split ? part : base + op.out * act;
            a.y_bytes = bytes(split ? mn * r.split : mn);
            a.O = split ? nullptr : O; a.o_bytes = bytes(a.O ? mn : 0);
            a.M = r.M; a.N = r.N; a.K = r.K; a.Cin = op.Cin; a.H = r.Hin; a.W = r.Win; a.Ho = r.Hout; a.Wo = r.Wout;
            a.ks = r.ksize; a.stride = r.stride; a.pad = r.ksize / 2; a.relu = r.relu; a.ksteps = r.ksteps;
            if (stem) launch_conv<64, true>(a, r, st);
            else if (r.bm == 128) launch_conv<128, false>(a, r, st);
            else if (r.bm == 64) launch_conv<64, false>(a, r, st);
            else launch_conv<32, false>(a, r, st);
        }
        PT_BBN_CHECK_LAUNCH();
    }
    return PT_BBN_OK;
}
