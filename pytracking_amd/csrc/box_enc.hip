// Box label encoders of LWL and RTS (ltr/models/lwl/label_encoder.py:58-216 = ltr/models/rts/label_encoder.py:106-265): the box-to-mask
// initialisation of STAHelper.predict_mask (RTS) and of lwl_boxinit (LWL).
//
//   ResidualDS16FeatSWBox    box -> binary mask (n,1,H,W), never stored -> DS16 trunk (stem, pool, two stride-2 blocks)   label_enc.hip x 5
//                            -> BasicBlock(c2 + feat_dim -> c3, stride 1) over cat(trunk, feat)                           k_bx_conv x 2
//                            -> label_pred | samp_w_pred                                                                  k_bx_conv x 1
//   ResidualDS16FeatSWBoxCatMultiBlock
//                            box -> binary mask -> bilinear resize to the feature size (n,1,h,w)                          k_bx_mask
//                            -> 1..4 BasicBlocks (stride 1, eval BatchNorm) over cat(feat, mask)                          k_bx_conv x 2 each
//                            -> label_pred                                                                                k_bx_conv x 1
//
// k_bx_conv<T> (exact fp32 MFMA 16x16x4, implicit GEMM, stride 1, zero padding 1): one workgroup of 4 waves = 4 output rows x 16 output
//   columns of one image x 16T output channels; wave w owns row w and holds T accumulator tiles D[channel][pixel].  The input channels
//   come from TWO tensors -- source A (n, CA, H, W), a caller tensor with its own image stride, and source B (n, CB, H, W) in the
//   workspace -- and the concatenation is never written: the weights' input channels are ordered [A | B] by the host packer and padded
//   with zeros to Cinp = ceil16(CA + CB), and a staged channel at or beyond CA + CB is zero in LDS (its load is redirected to the
//   last real channel and dropped).  Per 16 input channels the 6 x 18 input tile with its halo is staged in LDS (zero outside the
//   map = the padding); the next chunk's input values (7 per thread) and weight pieces (9 T 16-byte loads per lane) are fetched into
//   registers before the current chunk's 36 T MFMAs per wave, so both fetches run under them and the MFMA loop reads registers and
//   LDS only.  Operand pairing, the 16-byte weight pieces (w[co][tap][ci0 + 4*(l>>4) .. + 3]) and the 8 mod 16 plane padding are
//   k_le_conv's (label_enc.hip).
//   Epilogue = Ds16Conv's: y = acc * scale[co] + shift[co] (+ residual[co]) (ReLU for co < relu_n), to out0 (co < csplit) or out1.
//   K is not split and there are no atomics: repeated calls are bit-identical.
// k_bx_mask: the Cat encoder's mask plane, F.interpolate(bilinear, align_corners=False) of the box mask evaluated from the box itself
//   (four comparisons per tap); the identity when the image size is the feature size.
#include <algorithm>
#include <math.h>
#include "common.h"
#include "pt_internal.h"
#include "ds16_enc.h"
#include "box_slice.h"

namespace {

constexpr int BX_MAX_C = 128, BX_MAX_FEAT = 1024, BX_MAX_DIM = 1024, BX_MAX_N = 1024, BX_MAX_IMAGE = 8192, BX_MAX_BLOCKS = 4;
constexpr int BX_TR = 6, BX_TC = 18, BX_RAW = BX_TR * BX_TC, BX_PL = 120;           // 4 + 2 rows, 16 + 2 columns; plane 108 -> 8 mod 16
constexpr int BX_ELEMS = 16 * BX_RAW, BX_LD = (BX_ELEMS + 255) / 256;              // 1728 staged values, 7 per thread (the last: 192 threads)
static_assert(BX_PL >= BX_RAW && BX_PL % 16 == 8, "plane padding");

struct BxConv {
    const float* a; long a_img;                  // source A (n, CA, H, W): image stride in floats, dense channel planes
    const float* b; long b_img;                  // source B (n, CB, H, W); not read when CB = 0
    const float* w; const float* scale; const float* shift;      // (Cout, 3, 3, Cinp), (Cout), (Cout)
    const float* res; long res_img;              // optional residual (n, Cout, H, W) view
    float* out0; long out0_img; float* out1; long out1_img;      // channels < csplit -> out0[co], the others -> out1[co - csplit]
    int csplit, CA, CB, Cinp, Cout, H, W, relu_n, groups;
};

// grid (groups * ceil(W/16), ceil(H/4), n), 256 threads; groups = Cout / (16 T).  The channel group is the fastest-running part of the
// workgroup number: workgroups are dealt round-robin over the 8 XCDs, so with 8 groups the workgroups of one XCD share ONE group's
// weights (663 KB of the deployed 5.3 MB).  Nothing depends on the placement, and the per-call time did not move with it.
template <int T>
__global__ __launch_bounds__(256) void k_bx_conv(BxConv a) {
    __shared__ float tile[16 * BX_PL];
    const int img = blockIdx.z, g = blockIdx.x % a.groups, oy0 = blockIdx.y * 4, ox0 = (blockIdx.x / a.groups) * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, j = lane & 15;
    const long plane = (long)a.H * a.W;
    const float* srcA = a.a + (long)img * a.a_img;
    const float* srcB = a.b + (long)img * a.b_img;
    const int Cin = a.CA + a.CB;
    // the staged values of this thread: channel within the chunk, LDS slot, pixel offset in the plane (-1: padding, or no such value)
    int sc[BX_LD], sl[BX_LD], sp[BX_LD];
#pragma unroll
    for (int i = 0; i < BX_LD; ++i) {
        const int e = threadIdx.x + 256 * i, c = e / BX_RAW, rem = e - c * BX_RAW, r = rem / BX_TC, col = rem - r * BX_TC;
        const int iy = oy0 - 1 + r, ix = ox0 - 1 + col;
        sc[i] = c;
        sl[i] = e < BX_ELEMS ? c * BX_PL + rem : -1;
        sp[i] = (e < BX_ELEMS && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? iy * a.W + ix : -1;
    }
    // Every load is issued unconditionally from an address inside the tensors (the channel clamped to the last one, the pixel to the
    // plane's first) and the value is dropped when it is stored: a load under a divergent branch is waited for at the branch's end,
    // which would put the memory latency of every staged value in front of the MFMAs.
    float pre[BX_LD];
    auto fetch = [&](int ci0) {
#pragma unroll
        for (int i = 0; i < BX_LD; ++i) {
            const int ch = min(ci0 + sc[i], Cin - 1), pix = max(sp[i], 0);
            const float* p = ch < a.CA ? srcA + ch * plane : srcB + (ch - a.CA) * plane;
            pre[i] = p[pix];
        }
    };
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wl = a.w + ((long)(g * T * 16 + j) * 9) * a.Cinp + 4 * kq;             // + (t * 16 * 9 + tap) * Cinp + ci0
    // the 9 T weight pieces of a chunk, fetched one chunk ahead like the input values: nothing in the MFMA loop waits for memory
    f32x4 wv[9][T], wn[9][T];
    auto wfetch = [&](f32x4 (&dst)[9][T], int ci0) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int t = 0; t < T; ++t) dst[tap][t] = *(const f32x4*)(wl + ((long)t * 16 * 9 + tap) * a.Cinp + ci0);
    };
    fetch(0);
    wfetch(wv, 0);
    for (int ci0 = 0; ci0 < a.Cinp; ci0 += 16) {
        if (ci0) __syncthreads();                                        // every wave is done with the previous chunk
#pragma unroll
        for (int i = 0; i < BX_LD; ++i)
            if (sl[i] >= 0) tile[sl[i]] = (sp[i] >= 0 && ci0 + sc[i] < Cin) ? pre[i] : 0.f;
        __syncthreads();
        const bool more = ci0 + 16 < a.Cinp;
        if (more) {
            fetch(ci0 + 16);
            wfetch(wn, ci0 + 16);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float b = tile[(4 * kq + s) * BX_PL + (wave + ky) * BX_TC + j + kx];
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] = mfma16(wv[tap][t][s], b, acc[t]);
            }
        }
        if (more) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int t = 0; t < T; ++t) wv[tap][t] = wn[tap][t];
        }
    }
    const int oy = oy0 + wave, ox = ox0 + j;
    if (oy >= a.H || ox >= a.W) return;                                  // behind the last barrier
    const long pix = (long)oy * a.W + ox;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = (g * T + t) * 16 + 4 * kq + r;
            float v = fmaf(acc[t][r], a.scale[co], a.shift[co]);
            if (a.res) v += a.res[(long)img * a.res_img + co * plane + pix];
            if (co < a.relu_n) v = fmaxf(v, 0.f);
            if (co < a.csplit) a.out0[(long)img * a.out0_img + co * plane + pix] = v;
            else a.out1[(long)img * a.out1_img + (co - a.csplit) * plane + pix] = v;
        }
}

// The channel tile from the shape alone: the largest T (16 T output channels per workgroup, fewest passes over the input) that still
// gives one workgroup per CU; below that T = 1 (most workgroups).
int bx_conv(BxConv a, int n, hipStream_t st) {
    const int ct = a.Cout / 16;
    const long tiles = (long)pt_ceil_div(a.W, 16) * pt_ceil_div(a.H, 4) * n;
    int T = 1;
    for (int c : {4, 2})
        if (ct % c == 0 && tiles * (ct / c) >= 256) { T = c; break; }
    a.groups = ct / T;
    if (a.CB == 0) { a.b = a.a; a.b_img = a.a_img; }                     // never read
    const dim3 grid(pt_ceil_div(a.W, 16) * a.groups, pt_ceil_div(a.H, 4), n);            // x <= 64 * 16, y <= 256, z <= BX_MAX_N
    switch (T) {
        case 4: hipLaunchKernelGGL((k_bx_conv<4>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_bx_conv<2>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_bx_conv<1>), grid, dim3(256), 0, st, a); break;
    }
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// out (n, h, w) = bilinear resize (align_corners = False) of the H x W box mask of ResidualDS16FeatSWBoxCatMultiBlock.bbox_to_mask
// (no start clamp), each tap evaluated from the box.  grid (ceil(n h w / 256)), 256 threads
__global__ __launch_bounds__(256) void k_bx_mask(const float* __restrict__ boxes, float* __restrict__ out, int n, int H, int W, int h, int w) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * h * w) return;
    const int img = (int)(e / ((long)h * w)), rem = (int)(e - (long)img * h * w), y = rem / w, x = rem - y * w;
    const PtBoxRect box = pt_box_rect(boxes + 4 * (long)img, H, W, false);
    auto at = [&](int iy, int ix) { return (iy >= box.y0 && iy < box.y1 && ix >= box.x0 && ix < box.x1) ? 1.f : 0.f; };
    if (H == h && W == w) {
        out[e] = at(y, x);
        return;
    }
    const float sy = fmaxf((y + 0.5f) * ((float)H / (float)h) - 0.5f, 0.f), sx = fmaxf((x + 0.5f) * ((float)W / (float)w) - 0.5f, 0.f);
    const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1), y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    out[e] = (1.f - ly) * ((1.f - lx) * at(y0, x0) + lx * at(y0, x1)) + ly * ((1.f - lx) * at(y1, x0) + lx * at(y1, x1));
}

struct BxLayer { int Cin, Cinp, Cout; size_t w_off, s_off, b_off; };

size_t bx_layer(BxLayer& L, size_t at, int cin, int cout) {
    L.Cin = cin; L.Cinp = (cin + 15) / 16 * 16; L.Cout = cout;
    L.w_off = at; at += (size_t)cout * 9 * L.Cinp;
    L.s_off = at; at += cout;
    L.b_off = at; at += cout;
    return at;
}

BxConv bx_conv_args(const BxLayer& L, const float* pack, int H, int W) {
    BxConv a{};
    a.w = pack + L.w_off; a.scale = pack + L.s_off; a.shift = pack + L.b_off;
    a.Cinp = L.Cinp; a.Cout = L.Cout; a.csplit = L.Cout; a.H = H; a.W = W;
    a.out0_img = (long)L.Cout * H * W;
    return a;
}

bool bx_dim_ok(int c) { return c % 16 == 0 && c <= BX_MAX_C; }

// ---------------------------------------------------------------------------------------------------------------------------
// ResidualDS16FeatSWBox
struct BoxEncPlan {
    Ds16Plan trunk;
    BxLayer l[3];                                // res3.conv1 | downsample, res3.conv2, label_pred [| samp_w_pred]
    size_t trunk_pack, t3, r3, ws_floats, pack_floats;
};

int box_enc_plan(int n, int H, int W, int h, int w, int c0, int c1, int c2, int c3, int f, int feat_dim, int with_sw, BoxEncPlan* out) {
    if (n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || c0 <= 0 || c1 <= 0 || c2 <= 0 || c3 <= 0 || f <= 0 || feat_dim <= 0) return PT_ERR_SHAPE;
    BoxEncPlan p{};
    int rc = pt_le_box_trunk_plan(n, H, W, c0, c1, c2, &p.trunk);
    if (rc) return rc;
    if (!bx_dim_ok(c3) || !bx_dim_ok(f) || feat_dim % 16 || feat_dim > BX_MAX_FEAT || n > BX_MAX_N || h > BX_MAX_DIM || w > BX_MAX_DIM)
        return PT_ERR_UNSUPPORTED;
    if (h != p.trunk.H[4] || w != p.trunk.W[4]) return PT_ERR_UNSUPPORTED;          // the feature map is the trunk's output size
    p.trunk_pack = ds16_trunk_pack_floats(p.trunk);
    size_t at = p.trunk_pack;
    at = bx_layer(p.l[0], at, feat_dim + c2, 2 * c3);
    at = bx_layer(p.l[1], at, c3, c3);
    at = bx_layer(p.l[2], at, c3, with_sw ? 2 * f : f);
    p.pack_floats = at;
    size_t ws = p.trunk.ws_floats;
    p.t3 = ws; ws += pt_align_floats((size_t)n * 2 * c3 * h * w);
    p.r3 = ws; ws += pt_align_floats((size_t)n * c3 * h * w);
    p.ws_floats = ws;
    if (out) *out = p;
    return PT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// ResidualDS16FeatSWBoxCatMultiBlock
struct BoxCatPlan {
    int nb, F;
    BxLayer c1[BX_MAX_BLOCKS], c2[BX_MAX_BLOCKS], head;
    size_t mask, t[BX_MAX_BLOCKS], r[BX_MAX_BLOCKS], ws_floats, pack_floats;
};

// dims: the nblocks block widths, then label_pred's F
int box_cat_plan(int n, int H, int W, int h, int w, int nblocks, const int* dims, int feat_dim, BoxCatPlan* out) {
    if (n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || nblocks <= 0 || feat_dim <= 0) return PT_ERR_SHAPE;
    if (nblocks > BX_MAX_BLOCKS) return PT_ERR_UNSUPPORTED;
    for (int k = 0; k <= nblocks; ++k)
        if (dims[k] <= 0) return PT_ERR_SHAPE;
    for (int k = 0; k <= nblocks; ++k)
        if (!bx_dim_ok(dims[k])) return PT_ERR_UNSUPPORTED;
    if (feat_dim % 16 || feat_dim > BX_MAX_FEAT || n > BX_MAX_N || h > BX_MAX_DIM || w > BX_MAX_DIM || H > BX_MAX_IMAGE || W > BX_MAX_IMAGE)
        return PT_ERR_UNSUPPORTED;
    BoxCatPlan p{};
    p.nb = nblocks; p.F = dims[nblocks];
    size_t at = 0, ws = 0;
    const size_t hw = (size_t)h * w;
    p.mask = ws; ws += pt_align_floats((size_t)n * hw);
    for (int b = 0; b < nblocks; ++b) {
        at = bx_layer(p.c1[b], at, b ? dims[b - 1] : feat_dim + 1, 2 * dims[b]);
        at = bx_layer(p.c2[b], at, dims[b], dims[b]);
        p.t[b] = ws; ws += pt_align_floats((size_t)n * 2 * dims[b] * hw);
        p.r[b] = ws; ws += pt_align_floats((size_t)n * dims[b] * hw);
    }
    at = bx_layer(p.head, at, dims[nblocks - 1], p.F);
    p.pack_floats = at;
    p.ws_floats = ws;
    if (out) *out = p;
    return PT_OK;
}

// conv1 | downsample of a block into t (ReLU on the conv1 half), then conv2 + residual (the downsample half of t) + ReLU into r
int bx_block(const BxLayer& l1, const BxLayer& l2, const float* pack, const float* srcA, long a_img, int CA, const float* srcB, int CB,
             float* t, float* r, int n, int h, int w, hipStream_t st) {
    const int c = l2.Cout;
    const long hw = (long)h * w;
    BxConv a = bx_conv_args(l1, pack, h, w);
    a.a = srcA; a.a_img = a_img; a.CA = CA; a.b = srcB; a.b_img = CB * hw; a.CB = CB;
    a.out0 = t; a.relu_n = c;
    int rc = bx_conv(a, n, st);
    if (rc) return rc;
    a = bx_conv_args(l2, pack, h, w);
    a.a = t; a.a_img = 2 * c * hw; a.CA = c;
    a.res = t + c * hw; a.res_img = 2 * c * hw; a.out0 = r; a.relu_n = c;
    return bx_conv(a, n, st);
}

}  // namespace

int pt_box_slice_impl(int start, int extent, int len, int clamp_start, int* lo, int* hi) {
    if (!lo || !hi) return PT_ERR_NULL;
    const int lim = 1 << 29;
    if (len <= 0) return PT_ERR_SHAPE;
    if (len > lim || start < -lim || start > lim || extent < -lim || extent > lim) return PT_ERR_UNSUPPORTED;
    pt_box_slice_rule(start, extent, len, clamp_start != 0, lo, hi);
    return PT_OK;
}

size_t pt_box_enc_pack_floats_impl(int c0, int c1, int c2, int c3, int f, int feat_dim, int with_sw) {
    BoxEncPlan p;
    if (box_enc_plan(1, 1, 1, 1, 1, c0, c1, c2, c3, f, feat_dim, with_sw, &p) != PT_OK) return 0;
    return p.pack_floats;
}

size_t pt_box_enc_ws_bytes_impl(int n, int H, int W, int h, int w, int c0, int c1, int c2, int c3, int f, int feat_dim) {
    BoxEncPlan p;
    if (box_enc_plan(n, H, W, h, w, c0, c1, c2, c3, f, feat_dim, 1, &p) != PT_OK) return 0;
    return p.ws_floats * sizeof(float);
}

int pt_box_enc_impl(const float* boxes, const float* feat, long feat_img, const float* pack, float* label_enc, float* sample_w, int n,
                    int H, int W, int h, int w, int c0, int c1, int c2, int c3, int f, int feat_dim, int final_relu, void* ws,
                    size_t ws_bytes, hipStream_t st) {
    if (!boxes || !feat || !pack || !label_enc || !ws) return PT_ERR_NULL;
    BoxEncPlan p;
    int rc = box_enc_plan(n, H, W, h, w, c0, c1, c2, c3, f, feat_dim, sample_w != nullptr, &p);
    if (rc == PT_ERR_SHAPE) return rc;
    if (feat_img < (long)feat_dim * h * w) return PT_ERR_SHAPE;
    if (rc) return rc;
    if ((uintptr_t)pack % 16) return PT_ERR_UNSUPPORTED;                 // 16-byte weight loads
    for (const void* q : {(const void*)boxes, (const void*)feat, (const void*)label_enc, (const void*)sample_w})
        if ((uintptr_t)q % 4) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < p.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    if ((rc = pt_le_box_trunk_launch(boxes, pack, p.trunk, base, st))) return rc;
    // res3 over [A = feature | B = trunk output]; the packer has put the weights' input channels in that order
    if ((rc = bx_block(p.l[0], p.l[1], pack, feat, feat_img, feat_dim, base + p.trunk.r2, c2, base + p.t3, base + p.r3, n, h, w, st))) return rc;
    // heads: label_pred | samp_w_pred as one convolution, ReLU on label_pred's half where the module has one
    const long hw = (long)h * w;
    BxConv a = bx_conv_args(p.l[2], pack, h, w);
    a.a = base + p.r3; a.a_img = c3 * hw; a.CA = c3;
    a.csplit = f; a.out0 = label_enc; a.out0_img = f * hw; a.out1 = sample_w; a.out1_img = f * hw; a.relu_n = final_relu ? f : 0;
    return bx_conv(a, n, st);
}

size_t pt_box_cat_enc_pack_floats_impl(int nblocks, const int* dims, int feat_dim) {
    BoxCatPlan p;
    if (!dims || box_cat_plan(1, 1, 1, 1, 1, nblocks, dims, feat_dim, &p) != PT_OK) return 0;
    return p.pack_floats;
}

size_t pt_box_cat_enc_ws_bytes_impl(int n, int H, int W, int h, int w, int nblocks, const int* dims, int feat_dim) {
    BoxCatPlan p;
    if (!dims || box_cat_plan(n, H, W, h, w, nblocks, dims, feat_dim, &p) != PT_OK) return 0;
    return p.ws_floats * sizeof(float);
}

int pt_box_cat_enc_impl(const float* boxes, const float* feat, long feat_img, const float* pack, float* label_enc, int n, int H, int W,
                        int h, int w, int nblocks, const int* dims, int feat_dim, int final_relu, void* ws, size_t ws_bytes,
                        hipStream_t st) {
    if (!boxes || !feat || !pack || !label_enc || !dims || !ws) return PT_ERR_NULL;
    BoxCatPlan p;
    int rc = box_cat_plan(n, H, W, h, w, nblocks, dims, feat_dim, &p);
    if (rc == PT_ERR_SHAPE) return rc;
    if (feat_img < (long)feat_dim * h * w) return PT_ERR_SHAPE;
    if (rc) return rc;
    if ((uintptr_t)pack % 16) return PT_ERR_UNSUPPORTED;
    for (const void* q : {(const void*)boxes, (const void*)feat, (const void*)label_enc})
        if ((uintptr_t)q % 4) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < p.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    const long hw = (long)h * w, total = (long)n * hw;
    hipLaunchKernelGGL(k_bx_mask, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, boxes, base + p.mask, n, H, W, h, w);
    PT_CHECK_LAUNCH();
    // the first block reads [A = feature | B = mask plane] (the reference's order), the others the block before them
    const float* src = feat;
    long src_img = feat_img;
    int CA = feat_dim;
    for (int b = 0; b < nblocks; ++b) {
        if ((rc = bx_block(p.c1[b], p.c2[b], pack, src, src_img, CA, base + p.mask, b ? 0 : 1, base + p.t[b], base + p.r[b], n, h, w, st)))
            return rc;
        src = base + p.r[b]; CA = dims[b]; src_img = CA * hw;
    }
    BxConv a = bx_conv_args(p.head, pack, h, w);
    a.a = src; a.a_img = src_img; a.CA = CA;
    a.out0 = label_enc; a.relu_n = final_relu ? p.F : 0;
    return bx_conv(a, n, st);
}
