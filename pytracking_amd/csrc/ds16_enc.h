// Host side shared by the DS16 encoders -- ResidualDS16SW (label_enc.hip, stride 2), ResidualDS16SW_Clf (rts_fusion.hip, stride 1) and the
// mask trunk of ResidualDS16FeatSWBox (box_enc.hip through label_enc.hip, stride 2): one network at two strides, so one plan (pack
// layout, map sizes, workspace layout) and one driver (argument checks, then the chain
// stem -> conv1|downsample -> conv2 + residual -> conv1|downsample -> conv2 + residual -> label_pred|samp_w_pred).  The kernels, their
// argument structs and the tile choice stay with each source: the driver describes a convolution as a Ds16Conv and hands it to the
// launcher the source supplies.
#pragma once
#include <stdint.h>
#include "common.h"
#include "pt_internal.h"

struct Ds16Limits { int max_c, max_dim, max_n; };
struct Ds16Layer { int Cin, Cout; size_t w_off, s_off, b_off; };         // offsets into the pack, floats
struct Ds16Plan {
    int n, C[4], H[5], W[5];                     // H[0] input, H[1] stem conv, H[2] pool, H[3] block 1, H[4] block 2 and the heads
    Ds16Layer stem, conv[5];                     // conv: res1.conv1|downsample, res1.conv2, res2.conv1|downsample, res2.conv2, heads
    size_t s0, t1, r1, t2, r2, ws_floats, pack_floats;                   // workspace offsets, floats
};

// One 3x3 convolution of the chain: y = conv(in) * scale + shift (+ res) (ReLU for co < relu_n), channels < csplit to out0, the others
// to out1.  Views are (n, C, H, W) with the image stride in floats and dense channel planes.
struct Ds16Conv {
    const float* in; long in_img;
    const float* w; const float* scale; const float* shift;      // (Cout, 3, 3, Cin), (Cout), (Cout)
    const float* res; long res_img;
    float* out0; long out0_img; float* out1; long out1_img;
    int csplit, Cin, Cout, Hi, Wi, Ho, Wo, relu_n, stride;
};

// stride 2: every stage halves the map ((x - 1) / 2 + 1); stride 1: all five sizes are the input's
static inline int ds16_plan(int stride, const Ds16Limits& lim, int n, int H, int W, int c0, int c1, int c2, int f, Ds16Plan* out) {
    if (n <= 0 || H <= 0 || W <= 0 || c0 <= 0 || c1 <= 0 || c2 <= 0 || f <= 0) return PT_ERR_SHAPE;
    for (int c : {c0, c1, c2, f})
        if (c % 16 || c > lim.max_c) return PT_ERR_UNSUPPORTED;
    if (n > lim.max_n || H > lim.max_dim || W > lim.max_dim) return PT_ERR_UNSUPPORTED;
    Ds16Plan p{};
    p.n = n; p.C[0] = c0; p.C[1] = c1; p.C[2] = c2; p.C[3] = f;
    p.H[0] = H; p.W[0] = W;
    for (int k = 1; k < 5; ++k) { p.H[k] = (p.H[k - 1] - 1) / stride + 1; p.W[k] = (p.W[k - 1] - 1) / stride + 1; }
    size_t pk = 0;
    auto layer = [&](Ds16Layer& L, int cin, int cout) {
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

static inline size_t ds16_pack_floats(int stride, const Ds16Limits& lim, int c0, int c1, int c2, int f) {
    Ds16Plan p;
    return ds16_plan(stride, lim, 1, 1, 1, c0, c1, c2, f, &p) == PT_OK ? p.pack_floats : 0;
}

static inline size_t ds16_ws_bytes(int stride, const Ds16Limits& lim, int n, int H, int W, int c0, int c1, int c2, int f) {
    Ds16Plan p;
    return ds16_plan(stride, lim, n, H, W, c0, c1, c2, f, &p) == PT_OK ? p.ws_floats * sizeof(float) : 0;
}

// One convolution of the chain as a Ds16Conv: layer k of the plan from map level `level_in` to `level_out`, reading `src`.
static inline Ds16Conv ds16_layer(const Ds16Plan& p, int stride, const float* pack, int k, int level_in, int level_out, const float* src,
                                  int src_channels) {
    const Ds16Layer& L = p.conv[k];
    Ds16Conv a{};
    a.in = src; a.in_img = (long)src_channels * p.H[level_in] * p.W[level_in];
    a.w = pack + L.w_off; a.scale = pack + L.s_off; a.shift = pack + L.b_off;
    a.Cin = L.Cin; a.Cout = L.Cout;
    a.Hi = p.H[level_in]; a.Wi = p.W[level_in]; a.Ho = p.H[level_out]; a.Wo = p.W[level_out];
    a.stride = level_in == level_out ? 1 : stride;
    a.csplit = L.Cout; a.out0_img = (long)L.Cout * a.Ho * a.Wo;
    return a;
}

// The trunk of a checked plan: stem, then the two BasicBlocks (five launches); the result is (n, C2, H[4], W[4]) at base + p.r2.  The
// pack needs no more than its first `ds16_trunk_pack_floats` floats (the heads' layer comes last).  Used by ds16_encode below and, on
// its own, by the box label encoder (box_enc.hip), whose heads sit behind a third block.
template <class Stem, class Conv>
int ds16_trunk(int stride, const Ds16Plan& p, const float* pack, float* base, Stem stem, Conv conv) {
    int rc;
    const int n = p.n, c0 = p.C[0], c1 = p.C[1], c2 = p.C[2];
    if ((rc = stem(p, pack, base + p.s0))) return rc;
    const long hw3 = (long)p.H[3] * p.W[3], hw4 = (long)p.H[4] * p.W[4];
    // block 1: conv1 | downsample as one convolution with 2 C1 outputs (ReLU on the conv1 half), then conv2 + residual + ReLU
    Ds16Conv a = ds16_layer(p, stride, pack, 0, 2, 3, base + p.s0, c0);
    a.out0 = base + p.t1; a.relu_n = c1;
    if ((rc = conv(a, n))) return rc;
    a = ds16_layer(p, stride, pack, 1, 3, 3, base + p.t1, 2 * c1);
    a.res = base + p.t1 + c1 * hw3; a.res_img = 2 * c1 * hw3; a.out0 = base + p.r1; a.relu_n = c1;
    if ((rc = conv(a, n))) return rc;
    // block 2
    a = ds16_layer(p, stride, pack, 2, 3, 4, base + p.r1, c1);
    a.out0 = base + p.t2; a.relu_n = c2;
    if ((rc = conv(a, n))) return rc;
    a = ds16_layer(p, stride, pack, 3, 4, 4, base + p.t2, 2 * c2);
    a.res = base + p.t2 + c2 * hw4; a.res_img = 2 * c2 * hw4; a.out0 = base + p.r2; a.relu_n = c2;
    return conv(a, n);
}

static inline size_t ds16_trunk_pack_floats(const Ds16Plan& p) { return p.conv[4].w_off; }

// Checks everything before anything is queued, then runs the six launches.  `stem(plan, pack, out)` launches the source's stem kernel into
// the workspace, `conv(a, n)` one convolution; both return a PT_* code.  `sample_w_optional`: a null sample_w is allowed and skips that
// half of the heads (only label_pred's F channels -- the leading rows of the weights, scales and shifts -- are computed).
template <class Stem, class Conv>
int ds16_encode(int stride, const Ds16Limits& lim, bool sample_w_optional, const float* in, const float* pack, float* label_enc,
                float* sample_w, int n, int H, int W, int c0, int c1, int c2, int f, void* ws, size_t ws_bytes, Stem stem, Conv conv) {
    if (!in || !pack || !label_enc || (!sample_w && !sample_w_optional) || !ws) return PT_ERR_NULL;
    Ds16Plan p;
    int rc = ds16_plan(stride, lim, n, H, W, c0, c1, c2, f, &p);
    if (rc) return rc;
    if ((uintptr_t)pack % 16) return PT_ERR_UNSUPPORTED;                 // 16-byte weight loads
    for (const void* q : {(const void*)in, (const void*)label_enc, (const void*)sample_w})
        if ((uintptr_t)q % 4) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < p.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    float* base = (float*)ws;
    if ((rc = ds16_trunk(stride, p, pack, base, stem, conv))) return rc;
    // heads: label_pred | samp_w_pred as one convolution with 2 F outputs, ReLU on label_pred's half, written to the two results
    const long hw4 = (long)p.H[4] * p.W[4];
    Ds16Conv a = ds16_layer(p, stride, pack, 4, 4, 4, base + p.r2, c2);
    if (!sample_w) a.Cout = f;
    a.csplit = f; a.out0 = label_enc; a.out0_img = f * hw4; a.out1 = sample_w; a.out1_img = f * hw4; a.relu_n = f;
    return conv(a, n);
}

// The stride-2 mask trunk fed from boxes instead of masks (label_enc.hip: k_le_stem<true> and k_le_conv), for box_enc.hip.  `plan` checks
// the sizes against the label encoder's limits and lays the workspace out; `launch` queues the five launches of a checked plan.
int pt_le_box_trunk_plan(int n, int H, int W, int c0, int c1, int c2, Ds16Plan* p);
int pt_le_box_trunk_launch(const float* boxes, const float* pack, const Ds16Plan& p, float* ws, hipStream_t st);
