// IoU modulation vectors: AtomIoUNet.get_modulation (ltr/models/bbreg/atom_iou_net.py:138-170) in one call.
//
//   c3 = conv3_1r(feat3), c4 = conv4_1r(feat4)             Conv2d(3x3, pad 1, bias) -> BatchNorm2d (eval) -> ReLU (atom_iou_net.py:7-12)
//   roi3 = PrRoIPool(3x3, s3)(c3, roi), roi4 = PrRoIPool(1x1, s4)(c4, roi),  roi = (image, x, y, x + w, y + h)
//   fc3 = fc3_1r(roi3)                                     3x3 VALID convolution over the 3x3 pooled map: a linear map 9 A -> B
//   out3 = fc34_3r([fc3, roi4]), out4 = fc34_4r([fc3, roi4])      1x1 convolutions, (B + D) -> P3 / P4
// DiMP, PrDiMP, SuperDiMP, DiMP-simple, KeepTrack, KYS and ATOM run it once, in init_iou_net, on the augmented first-frame images.
//
// PrRoIPool reads c3 / c4 only under the box, so the two convolutions are computed only there: per image and level the pixel window of
// iou_window.h (ONE definition for k_iou_mod_conv, k_iou_mod_pool and pt_iou_mod_window), read from the box on the device.
//
//   k_iou_mod_conv   both levels in one launch.  A workgroup (8 waves) owns 16 window-relative positions x 32 output channels of one image
//                    and level and walks K = 9 Cin itself on the fp32 MFMA (16x16x4): K is cut into groups of 16 input channels x 9 taps,
//                    wave w takes groups w, w + 8, ..., the eight partial tiles are added in wave order through LDS, then
//                    relu(sum * scale + shift).
//                    (A first-frame window is ~80 / ~25 positions per image, so the live workgroups are few: their length, not their
//                    number, is the time of the launch -- hence the small channel tile and the 8-way split.)  The grid is sized for a window
//                    equal to the whole map; a workgroup whose tile lies beyond its image's window returns in front of the barrier
//                    (workgroup-uniform).  Taps outside the map read 0, taps outside the window read the map.  Image i's result is stored
//                    as a (C, y1 + 1, x1 + 1) map -- row pitch x1 + 1 -- written only inside the window [x0, x1] x [y0, y1].
//   k_iou_mod_pool   prroi_fwd_elem of prroi_dev.h on that map, given as its H x W: make_bin then clamps every bin to the window's last
//                    row and column itself (in fp32 the end of the last bin, xs + bw, may lie an ulp beyond x1 * s; the pixel that
//                    would add carries a weight below 1e-13), and its first row and column are floor(x0 * s), the window's own.  So the
//                    pooling never reads what the convolution did not write.  -> roi3 tap-major (9 A) and roi4 straight into `cat`.
//   k_iou_mod_linear fc3 (-> `cat`) in one launch, then fc34_3r and fc34_4r in one launch: one wave per output channel, 16-byte weight loads, plain
//                    fp32 FMA, eight images per pass over the row, wave_sum.  Weight-bandwidth-bound at n <= 32.
// Four launches, no atomics, fixed summation order: repeated calls are bit-identical.  No host synchronisation, graph-capturable.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "pt_internal.h"
#include "prroi_dev.h"
#include "iou_window.h"

namespace {

constexpr int MOD_MAX_N = 32, MOD_MAX_HW = 4096, MOD_MAX_C = 4096;
constexpr int MOD_TP = 16, MOD_TC = 32, MOD_PAD = 17;        // positions, channels of a workgroup's tile; LDS pitch of a channel's row
constexpr int MOD_WAVES = 8;                                  // waves of a workgroup: the split of K

struct ModLevel { int Cin, Cout, H, W; size_t w_off, s_off, b_off, map; };              // pack offsets; workspace offset of the maps
struct ModLin { int K, O; size_t w_off, s_off, b_off; };
struct ModPlan { int n, A, B, D; ModLevel lv[2]; ModLin fc3, fc34[2]; size_t r3, cat, ws_floats, pack_floats; };

struct ModConv { const float* feat; const float* boxes; const float* w; const float* scale; const float* shift; float* out;
                 int Cin, Cout, H, W; float s; };

struct ModConv2 { ModConv lv[2]; int n; };

// grid (max over the levels of ceil(H W / 16), of ceil(Cout / 32), 2 n), 512 threads; blockIdx.z = level * n + image
__global__ __launch_bounds__(MOD_WAVES * 64) void k_iou_mod_conv(ModConv2 both) {
    __shared__ float red[MOD_WAVES][MOD_TC][MOD_PAD];
    const int level = (int)blockIdx.z >= both.n, img = blockIdx.z - level * both.n, tile = blockIdx.x, co = blockIdx.y * MOD_TC;
    const ModConv a = both.lv[level];
    const PtIouWin win = pt_iou_window(a.boxes + 4 * img, a.s, a.H, a.W);
    const int wW = win.x1 - win.x0 + 1, wH = win.y1 - win.y0 + 1;
    if (co >= a.Cout || wW <= 0 || wH <= 0 || tile * MOD_TP >= wW * wH) return;          // workgroup-uniform, in front of the barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int HW = a.H * a.W, nj = min(MOD_TC / 16, (a.Cout - co) / 16);
    const int pos = tile * MOD_TP + col;
    const bool live = pos < wW * wH;
    const int py = live ? win.y0 + pos / wW : win.y0, px = live ? win.x0 + pos % wW : win.x0;
    // per tap: the offset of the input pixel, clamped into the map so that every load is in bounds, and whether it counts
    int off[9];
    bool ok[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int y = py + tap / 3 - 1, x = px + tap % 3 - 1;
        ok[tap] = live && y >= 0 && y < a.H && x >= 0 && x < a.W;
        off[tap] = min(max(y, 0), a.H - 1) * a.W + min(max(x, 0), a.W - 1);
    }
    const float* fimg = a.feat + (long)img * a.Cin * HW + (long)(4 * g) * HW;
    const float* wrow[MOD_TC / 16];
#pragma unroll
    for (int j = 0; j < MOD_TC / 16; ++j) wrow[j] = a.w + (long)(co + min(j, nj - 1) * 16 + col) * 9 * a.Cin + 4 * g;
    f32x4 acc[MOD_TC / 16];
#pragma unroll
    for (int j = 0; j < MOD_TC / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K = 9 Cin in groups of 16 input channels x 9 taps; wave w takes groups w, w + 8, ...  Inside a group lane group g supplies input
    // channels c0 + 4 g .. + 3 (as A[position][k] and B[k][channel]): one 16-byte weight load serves four MFMA steps.  All 36 + 18 loads
    // of a group are independent and branch-free, so they are in flight together: a group costs ONE memory latency, not one per tap.
    for (int c0 = wave * 16; c0 < a.Cin; c0 += MOD_WAVES * 16) {
        float av[9][4];
        f32x4 bv[9][MOD_TC / 16];
        const float* p = fimg + (long)c0 * HW;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int s = 0; s < 4; ++s) av[tap][s] = p[(long)s * HW + off[tap]];
#pragma unroll
            for (int j = 0; j < MOD_TC / 16; ++j) bv[tap][j] = *(const f32x4*)(wrow[j] + tap * a.Cin + c0);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int j = 0; j < MOD_TC / 16; ++j) {
                if (j < nj) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[j] = mfma16(ok[tap] ? av[tap][s] : 0.f, bv[tap][j][s], acc[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MOD_TC / 16; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][j * 16 + col][4 * g + r] = acc[j][r];      // D[position 4 g + r][channel col]
    __syncthreads();
    const int tp = threadIdx.x & 15, ch = threadIdx.x >> 4, tpos = tile * MOD_TP + tp;
    if (tpos >= wW * wH || ch >= nj * 16) return;
    const int oy = win.y0 + tpos / wW, ox = win.x0 + tpos % wW, pitch = win.x1 + 1, plane = (win.y1 + 1) * pitch;
    float s = red[0][ch][tp];
#pragma unroll
    for (int w = 1; w < MOD_WAVES; ++w) s += red[w][ch][tp];                             // fixed order
    a.out[(long)img * a.Cout * HW + (long)(co + ch) * plane + oy * pitch + ox] = fmaxf(fmaf(s, a.scale[co + ch], a.shift[co + ch]), 0.f);
}

struct ModPool { const float* boxes; const float* map[2]; float* out[2]; long out_stride[2]; int C[2], H[2], W[2], P[2]; float s[2]; };

// grid (ceil(max(9 A, D) / 256), n, 2 levels), 256 threads; element e of level 0 = bin e / A of channel e % A (tap-major, as fc3's weights)
__global__ __launch_bounds__(256) void k_iou_mod_pool(ModPool a) {
    const int lv = blockIdx.z, img = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    const int C = a.C[lv], P = a.P[lv];
    if (e >= P * P * C) return;
    const float* bb = a.boxes + 4 * img;
    const PtIouWin win = pt_iou_window(bb, a.s[lv], a.H[lv], a.W[lv]);
    const float roi[5] = {0.f, bb[0], bb[1], bb[0] + bb[2], bb[1] + bb[3]};
    const int bin = e / C, c = e % C;
    const float* m = a.map[lv] + (long)img * C * a.H[lv] * a.W[lv];
    a.out[lv][img * a.out_stride[lv] + e] = prroi_fwd_elem(m, roi, 0, c, bin / P, bin % P, 1, C, win.y1 + 1, win.x1 + 1, P, P, a.s[lv]);
}

struct ModHead { const float* w; const float* scale; const float* shift; float* out; int O; long out_stride; };
struct ModLinArgs { ModHead h[2]; const float* x; long x_stride; int K, n; };

// grid (ceil((O0 + O1) / 4)), 256 threads: one wave per output channel (O0 % 4 == 0), out[i][o] = relu(dot(w[o], x[i]) * scale + shift)
__global__ __launch_bounds__(256) void k_iou_mod_linear(ModLinArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int o = blockIdx.x * 4 + wave;
    const int second = o >= a.h[0].O;
    const ModHead h = a.h[second];
    if (second) o -= a.h[0].O;
    if (o >= h.O) return;                                               // wave-uniform; the kernel has no barrier
    const float* w = h.w + (long)o * a.K;
    const float sc = h.scale[o], sh = h.shift[o];
    for (int i0 = 0; i0 < a.n; i0 += 8) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = lane * 4; k < a.K; k += 256) {
            const f32x4 wv = *(const f32x4*)(w + k);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i0 + i < a.n) {
                    const f32x4 xv = *(const f32x4*)(a.x + (i0 + i) * a.x_stride + k);
                    acc[i] = fmaf(wv[3], xv[3], fmaf(wv[2], xv[2], fmaf(wv[1], xv[1], fmaf(wv[0], xv[0], acc[i]))));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s = wave_sum(acc[i]);
            if (lane == 0 && i0 + i < a.n) h.out[(i0 + i) * h.out_stride + o] = fmaxf(fmaf(s, sc, sh), 0.f);
        }
    }
}

int mod_plan(int n, int Cin3, int A, int B, int Cin4, int D, int P3, int P4, int H3, int W3, int H4, int W4, ModPlan* out) {
    for (int v : {n, Cin3, A, B, Cin4, D, P3, P4, H3, W3, H4, W4})
        if (v <= 0) return PT_ERR_SHAPE;
    if (n > MOD_MAX_N || (long)H3 * W3 > MOD_MAX_HW || (long)H4 * W4 > MOD_MAX_HW) return PT_ERR_UNSUPPORTED;
    if (Cin3 % 64 || Cin4 % 64 || A % 16 || B % 16 || D % 16 || P3 % 16 || P4 % 16) return PT_ERR_UNSUPPORTED;
    for (int v : {Cin3, A, B, Cin4, D, P3, P4})
        if (v > MOD_MAX_C) return PT_ERR_UNSUPPORTED;
    ModPlan p{};
    p.n = n; p.A = A; p.B = B; p.D = D;
    size_t pk = 0, ws = 0;
    auto take = [&](size_t k) { size_t r = ws; ws += pt_align_floats(k); return r; };
    auto layer = [&](size_t cout, size_t k, size_t* w, size_t* s, size_t* b) {
        *w = pk; pk += cout * k;
        *s = pk; pk += cout;
        *b = pk; pk += cout;
    };
    const int lv[2][4] = {{Cin3, A, H3, W3}, {Cin4, D, H4, W4}};
    for (int t = 0; t < 2; ++t) {
        ModLevel& L = p.lv[t];
        L.Cin = lv[t][0]; L.Cout = lv[t][1]; L.H = lv[t][2]; L.W = lv[t][3];
        layer(L.Cout, (size_t)9 * L.Cin, &L.w_off, &L.s_off, &L.b_off);
        L.map = take((size_t)n * L.Cout * L.H * L.W);
    }
    p.fc3.K = 9 * A; p.fc3.O = B;
    layer(B, p.fc3.K, &p.fc3.w_off, &p.fc3.s_off, &p.fc3.b_off);
    const int P[2] = {P3, P4};
    for (int t = 0; t < 2; ++t) {
        p.fc34[t].K = B + D; p.fc34[t].O = P[t];
        layer(P[t], p.fc34[t].K, &p.fc34[t].w_off, &p.fc34[t].s_off, &p.fc34[t].b_off);
    }
    p.r3 = take((size_t)n * 9 * A);
    p.cat = take((size_t)n * (B + D));
    p.ws_floats = ws; p.pack_floats = pk;
    if (out) *out = p;
    return PT_OK;
}

}  // namespace

extern "C" size_t pt_iou_mod_pack_floats(int Cin3, int A, int B, int Cin4, int D, int P3, int P4) {
    ModPlan p;
    return mod_plan(1, Cin3, A, B, Cin4, D, P3, P4, 1, 1, 1, 1, &p) == PT_OK ? p.pack_floats : 0;
}

extern "C" size_t pt_iou_mod_ws_bytes(int n, int Cin3, int A, int B, int Cin4, int D, int P3, int P4, int H3, int W3, int H4, int W4) {
    ModPlan p;
    return mod_plan(n, Cin3, A, B, Cin4, D, P3, P4, H3, W3, H4, W4, &p) == PT_OK ? p.ws_floats * sizeof(float) : 0;
}

extern "C" int pt_iou_mod_window(const float* box_xywh, float scale, int H, int W, int* out_x0y0x1y1) {
    if (!box_xywh || !out_x0y0x1y1) return PT_ERR_NULL;
    if (H <= 0 || W <= 0 || !(scale > 0.f)) return PT_ERR_SHAPE;
    const PtIouWin w = pt_iou_window(box_xywh, scale, H, W);
    out_x0y0x1y1[0] = w.x0; out_x0y0x1y1[1] = w.y0; out_x0y0x1y1[2] = w.x1; out_x0y0x1y1[3] = w.y1;
    return pt_iou_win_empty(w) ? 1 : PT_OK;
}

extern "C" int pt_iou_mod_f32(const float* feat3, const float* feat4, const float* boxes, const float* pack, float* out3, float* out4,
                              int n, int Cin3, int A, int B, int Cin4, int D, int P3, int P4, int H3, int W3, int H4, int W4, float s3,
                              float s4, void* ws, size_t ws_bytes, void* stream) {
    if (!feat3 || !feat4 || !boxes || !pack || !out3 || !out4 || !ws) return PT_ERR_NULL;
    ModPlan p;
    int rc = mod_plan(n, Cin3, A, B, Cin4, D, P3, P4, H3, W3, H4, W4, &p);
    if (rc) return rc;
    if (!(s3 > 0.f) || !(s4 > 0.f)) return PT_ERR_SHAPE;
    for (const void* q : {(const void*)feat3, (const void*)feat4, (const void*)boxes, (const void*)pack, (const void*)out3, (const void*)out4})
        if ((uintptr_t)q % 16) return PT_ERR_UNSUPPORTED;
    if (ws_bytes < p.ws_floats * sizeof(float) || ((uintptr_t)ws % 256) != 0) return PT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)ws;
    const float* feat[2] = {feat3, feat4};
    const float sc[2] = {s3, s4};
    ModConv2 cv{};
    cv.n = n;
    unsigned tiles = 0, groups = 0;
    for (int t = 0; t < 2; ++t) {
        const ModLevel& L = p.lv[t];
        cv.lv[t] = ModConv{feat[t], boxes, pack + L.w_off, pack + L.s_off, pack + L.b_off, base + L.map, L.Cin, L.Cout, L.H, L.W, sc[t]};
        tiles = std::max(tiles, (unsigned)((L.H * L.W + MOD_TP - 1) / MOD_TP));
        groups = std::max(groups, (unsigned)((L.Cout + MOD_TC - 1) / MOD_TC));
    }
    hipLaunchKernelGGL(k_iou_mod_conv, dim3(tiles, groups, 2 * n), dim3(MOD_WAVES * 64), 0, st, cv);
    PT_CHECK_LAUNCH();
    ModPool pl{};
    pl.boxes = boxes;
    for (int t = 0; t < 2; ++t) {
        const ModLevel& L = p.lv[t];
        pl.map[t] = base + L.map; pl.C[t] = L.Cout; pl.H[t] = L.H; pl.W[t] = L.W; pl.s[t] = sc[t];
    }
    pl.P[0] = 3; pl.out[0] = base + p.r3; pl.out_stride[0] = 9 * A;
    pl.P[1] = 1; pl.out[1] = base + p.cat + B; pl.out_stride[1] = B + D;
    hipLaunchKernelGGL(k_iou_mod_pool, dim3((std::max(9 * A, D) + 255) / 256, n, 2), dim3(256), 0, st, pl);
    PT_CHECK_LAUNCH();
    ModLinArgs l{};
    l.h[0] = ModHead{pack + p.fc3.w_off, pack + p.fc3.s_off, pack + p.fc3.b_off, base + p.cat, B, (long)(B + D)};
    l.x = base + p.r3; l.x_stride = 9 * A; l.K = 9 * A; l.n = n;
    hipLaunchKernelGGL(k_iou_mod_linear, dim3(B / 4), dim3(256), 0, st, l);
    PT_CHECK_LAUNCH();
    float* outs[2] = {out3, out4};
    for (int t = 0; t < 2; ++t)
        l.h[t] = ModHead{pack + p.fc34[t].w_off, pack + p.fc34[t].s_off, pack + p.fc34[t].b_off, outs[t], p.fc34[t].O, (long)p.fc34[t].O};
    l.x = base + p.cat; l.x_stride = B + D; l.K = B + D;
    hipLaunchKernelGGL(k_iou_mod_linear, dim3((P3 + P4) / 4), dim3(256), 0, st, l);
    PT_CHECK_LAUNCH();
    return PT_OK;
}
