// libpt_mot: the per-frame multi-object read-out of TaMOs on the device (include/pt_mot.h).
//   TaMOs.localize_target / localize_advanced   pytracking/tracker/tamos/tamos.py:324-429
//   TaMOs.direct_bbox_regression                tamos.py:248-280
//   TaMOs.clip_bbox_to_image_area               tamos.py:106-112
//   the bicubic upsample of classify_target     tamos.py:319-320
//   TaMOs.encode_bbox / get_label_function      tamos.py:114-153, 582-592; dcf.gauss_spatial, dcf.py:48-59
// The reference does all of this per object on the host: two max2d's, a clone, a masked fill and about eight .item() / .cpu() round trips
// in localize_advanced, a copy of the object's whole ltrb map for four numbers in direct_bbox_regression.  Here one workgroup per object
// stages the object's map in LDS once, finds both peaks with max2d's tie order (localize_dev.h), decides the outcome, reads the four
// ltrb values of the chosen cell and leaves one record per object; the host waits once per frame.
//
// Arithmetic types follow what the reference's expressions evaluate to under torch, as in csrc/localize.hip: `tensor.item() < python
// float` compares doubles, `python float * float32 tensor` and `float32 tensor > python float` are float32 operations with the scalar
// rounded to float32 first, Python's round() on doubles is rint.  The decision and the box keep the reference's operation order with
// every product, quotient and sum rounded on its own (__fmul_rn / __fdiv_rn / __fadd_rn): no FMA contraction.
#include <chrono>
#include <math.h>
#include "../csrc/pt_internal.h"
#include "../csrc/localize_dev.h"
#include "../../include/pt_mot.h"

static_assert(PT_MOT_NORMAL == PT_LOC_NORMAL && PT_MOT_HARD_NEGATIVE == PT_LOC_HARD_NEGATIVE && PT_MOT_UNCERTAIN == PT_LOC_UNCERTAIN &&
              PT_MOT_NOT_FOUND == PT_LOC_NOT_FOUND, "the flags of both libraries are one set");

#define PT_MOT_CHECK_LAUNCH()                                          \
    do {                                                               \
        if (hipGetLastError() != hipSuccess) return PT_MOT_ERR_LAUNCH; \
    } while (0)

namespace {

struct MotArgs {
    const float *scores, *ltrb;
    float *map_out, *rec;
    int Hs, Ws, H, W, upsample, normalize;
    float seq;
    double th_not_found, th_uncertain, th_hard_sample;
    float th_distractor, th_hard_negative, th_not_found_f32;
    float train_w, train_h;            // train_img_sample_sz[1], [0]
    float sample_w, sample_h;          // img_sample_sz[1], [0]
    float sc[4];                       // sample_coords[0]: y0, x0, y1, x1
    float image_w, image_h, min_w, min_h;
    int stride;
    int active[PT_MOT_MAX_OBJECTS];
    pt_mot_consts c[PT_MOT_MAX_OBJECTS];
};

// torch's bicubic coefficients (UpSample.h: cubic_convolution1 / cubic_convolution2 with A = -0.75) for the taps at floor(x) - 1 .. + 2
__device__ __forceinline__ void cubic_coeffs(float t, float w[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void k_mot_readout(MotArgs a) {
    __shared__ float map[PT_MOT_MAX_CELLS];
    __shared__ Peak sh[4];
    const int obj = a.active[blockIdx.x];
    const pt_mot_consts q = a.c[blockIdx.x];
    const int H = a.H, W = a.W, HW = H * W;
    const float* src = a.scores + (long)obj * a.Hs * a.Ws;

    // ---- the map at (H, W): as it is, or F.interpolate(mode='bicubic') (align_corners=False: src = scale * (dst + 0.5) - 0.5) ----
    const float scale_h = (float)a.Hs / (float)H, scale_w = (float)a.Ws / (float)W;
    for (int i = threadIdx.x; i < HW; i += 256) {
        float v;
        if (!a.upsample) {
            v = src[i];
        } else {
            const int oy = i / W, ox = i - oy * W;
            const float sy = scale_h * ((float)oy + 0.5f) - 0.5f, sx = scale_w * ((float)ox + 0.5f) - 0.5f;
            const float fy = floorf(sy), fx = floorf(sx);
            float wy[4], wx[4];
            cubic_coeffs(sy - fy, wy);
            cubic_coeffs(sx - fx, wx);
            const int iy = (int)fy, ix = (int)fx;
            v = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* row = src + (long)clampi(iy - 1 + u, 0, a.Hs - 1) * a.Ws;
                float r = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) r += wx[k] * row[clampi(ix - 1 + k, 0, a.Ws - 1)];
                v += wy[u] * r;
            }
        }
        if (a.normalize) v = 1.f / (1.f + expf(-v));
        map[i] = v;
        if (a.map_out) a.map_out[(long)obj * HW + i] = v;
    }
    __syncthreads();

    // ---- localize_advanced (tamos.py:366-429), one scale, no output window ----
    const Peak p1 = block_peak(scan_map(map, H, W, 0, 0, 0, 0), sh);
    const double m1 = (double)p1.v;
    int code = -1;
    if (m1 < a.th_not_found) code = PT_MOT_NOT_FOUND;
    else if (m1 < a.th_uncertain) code = PT_MOT_UNCERTAIN;
    else if (m1 < a.th_hard_sample) code = PT_MOT_HARD_NEGATIVE;
    Peak p2{0.f, 0, 0};
    const bool second = code < 0;                                        // the same in every thread: p1 is
    if (second) {
        const double nr = (double)q.neigh[0], nc = (double)q.neigh[1];
        const int top = max((int)rint((double)p1.r - nr / 2), 0);
        const int bottom = min((int)rint((double)p1.r + nr / 2 + 1), H);
        const int left = max((int)rint((double)p1.c - nc / 2), 0);
        const int right = min((int)rint((double)p1.c + nc / 2 + 1), W);
        p2 = block_peak(scan_map(map, H, W, top, bottom, left, right), sh);
    }
    if (threadIdx.x != 0) return;

    int pick = 1;
    if (second) {
        if (p2.v > __fmul_rn(a.th_distractor, p1.v)) {
            // target_disp = max_disp - score_center; the norms of (target_disp - prev_target_vec)
            const float e1r = __fsub_rn(__fsub_rn((float)p1.r, q.center[0]), q.prev[0]), e1c = __fsub_rn(__fsub_rn((float)p1.c, q.center[1]), q.prev[1]);
            const float e2r = __fsub_rn(__fsub_rn((float)p2.r, q.center[0]), q.prev[0]), e2c = __fsub_rn(__fsub_rn((float)p2.c, q.center[1]), q.prev[1]);
            const float n1 = __fsqrt_rn(__fadd_rn(__fmul_rn(e1r, e1r), __fmul_rn(e1c, e1c)));
            const float n2 = __fsqrt_rn(__fadd_rn(__fmul_rn(e2r, e2r), __fmul_rn(e2c, e2c)));
            const bool far1 = n1 > q.disp_threshold, near1 = n1 < q.disp_threshold;
            const bool far2 = n2 > q.disp_threshold, near2 = n2 < q.disp_threshold;
            if (far2 && near1) code = PT_MOT_HARD_NEGATIVE;
            else if (near2 && far1) { code = PT_MOT_HARD_NEGATIVE; pick = 2; }
            else code = PT_MOT_UNCERTAIN;
        } else if (p2.v > __fmul_rn(a.th_hard_negative, p1.v) && p2.v > a.th_not_found_f32) {
            code = PT_MOT_HARD_NEGATIVE;
        } else {
            code = PT_MOT_NORMAL;
        }
    }
    // an all-NaN map leaves the scan's start value (row H, col W): keep the ltrb read inside the map
    const int r = clampi(pick == 1 ? p1.r : p2.r, 0, H - 1), c = clampi(pick == 1 ? p1.c : p2.c, 0, W - 1);

    // ---- direct_bbox_regression (tamos.py:248-280) at (r, c): locations = shifts + stride // 2 ----
    const float* lt = a.ltrb + (long)obj * 4 * HW + (long)r * W + c;
    const float l = lt[0], t = lt[HW], rr = lt[2 * HW], b = lt[3 * HW];
    const float xs = (float)(c * a.stride + a.stride / 2), ys = (float)(r * a.stride + a.stride / 2);
    const float xs1 = __fsub_rn(xs, __fmul_rn(l, a.train_w)), xs2 = __fadd_rn(xs, __fmul_rn(rr, a.train_w));
    const float ys1 = __fsub_rn(ys, __fmul_rn(t, a.train_h)), ys2 = __fadd_rn(ys, __fmul_rn(b, a.train_h));
    const float dx = __fsub_rn(a.sc[3], a.sc[1]), dy = __fsub_rn(a.sc[2], a.sc[0]);
    const float x1 = __fadd_rn(__fmul_rn(__fdiv_rn(xs1, a.sample_w), dx), a.sc[1]);
    const float y1 = __fadd_rn(__fmul_rn(__fdiv_rn(ys1, a.sample_h), dy), a.sc[0]);
    const float x2 = __fadd_rn(__fmul_rn(__fdiv_rn(xs2, a.sample_w), dx), a.sc[1]);
    const float y2 = __fadd_rn(__fmul_rn(__fdiv_rn(ys2, a.sample_h), dy), a.sc[0]);
    const float bw = __fsub_rn(x2, x1), bh = __fsub_rn(y2, y1);
    // ---- clip_bbox_to_image_area (tamos.py:106-112) ----
    const float cx1 = fmaxf(0.f, fminf(x1, __fsub_rn(a.image_w, a.min_w)));
    const float cy1 = fmaxf(0.f, fminf(y1, __fsub_rn(a.image_h, a.min_h)));
    const float cx2 = fmaxf(__fadd_rn(cx1, a.min_w), fminf(__fadd_rn(x1, bw), a.image_w));
    const float cy2 = fmaxf(__fadd_rn(cy1, a.min_h), fminf(__fadd_rn(y1, bh), a.image_h));

    float* o = a.rec + (long)obj * PT_MOT_REC_FLOATS;
    o[PT_MOT_R_FLAG] = (float)code; o[PT_MOT_R_PICK] = (float)pick; o[PT_MOT_R_ROW] = (float)r; o[PT_MOT_R_COL] = (float)c;
    o[PT_MOT_R_MAX1] = p1.v; o[PT_MOT_R_ROW1] = (float)p1.r; o[PT_MOT_R_COL1] = (float)p1.c;
    o[PT_MOT_R_MAX2] = p2.v; o[PT_MOT_R_ROW2] = (float)p2.r; o[PT_MOT_R_COL2] = (float)p2.c;
    o[PT_MOT_R_PRESENCE] = p1.v;
    o[PT_MOT_R_RAW_BOX] = x1; o[PT_MOT_R_RAW_BOX + 1] = y1; o[PT_MOT_R_RAW_BOX + 2] = bw; o[PT_MOT_R_RAW_BOX + 3] = bh;
    o[PT_MOT_R_BOX] = cx1; o[PT_MOT_R_BOX + 1] = cy1; o[PT_MOT_R_BOX + 2] = __fsub_rn(cx2, cx1); o[PT_MOT_R_BOX + 3] = __fsub_rn(cy2, cy1);
    o[PT_MOT_R_LTRB] = l; o[PT_MOT_R_LTRB + 1] = t; o[PT_MOT_R_LTRB + 2] = rr; o[PT_MOT_R_LTRB + 3] = b;
    o[PT_MOT_R_OBJECT] = (float)obj; o[PT_MOT_R_SECOND] = second ? 1.f : 0.f;
    for (int k = PT_MOT_R_SECOND + 1; k < PT_MOT_R_SEQ; ++k) o[k] = 0.f;
    __threadfence_system();                                              // the record is visible before its sequence word
    __hip_atomic_store(o + PT_MOT_R_SEQ, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct TargetArgs {
    const float* boxes;
    float *ltrb_out, *label_out;
    int nb, H3, W3, stride, n_centres, LH, LW;
    float out_w, out_h;
    float coef[2], k0[2];              // -1 / (2 sigma^2) and the first sample position -(sz - 1) / 2, [row, col]
    float centres[2 * PT_MOT_MAX_CENTRES];
};

// one output element per thread: first the nb * 4 * H3 * W3 ltrb targets, then the n_centres * LH * LW label cells
__global__ __launch_bounds__(256) void k_mot_targets(TargetArgs a) {
    const long n_ltrb = (long)a.nb * 4 * a.H3 * a.W3, n_lab = (long)a.n_centres * a.LH * a.LW;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_ltrb) {
        const int c = (int)(i % a.W3), r = (int)((i / a.W3) % a.H3), k = (int)((i / ((long)a.W3 * a.H3)) % 4);
        const long bi = i / ((long)4 * a.W3 * a.H3);
        const float x0 = a.boxes[4 * bi], y0 = a.boxes[4 * bi + 1], w = a.boxes[4 * bi + 2], h = a.boxes[4 * bi + 3];
        float v = 0.f;
        if (w > 0.f && h > 0.f) {
            const float xs = (float)(c * a.stride + a.stride / 2), ys = (float)(r * a.stride + a.stride / 2);
            if (k == 0) v = __fdiv_rn(__fsub_rn(xs, x0), a.out_w);
            else if (k == 1) v = __fdiv_rn(__fsub_rn(ys, y0), a.out_h);
            else if (k == 2) v = __fdiv_rn(__fsub_rn(__fadd_rn(x0, w), xs), a.out_w);
            else v = __fdiv_rn(__fsub_rn(__fadd_rn(y0, h), ys), a.out_h);
        }
        a.ltrb_out[i] = v;
        return;
    }
    i -= n_ltrb;
    if (i >= n_lab) return;
    const int c = (int)(i % a.LW), r = (int)((i / a.LW) % a.LH), m = (int)(i / ((long)a.LW * a.LH));
    const float dr = __fsub_rn(__fadd_rn(a.k0[0], (float)r), a.centres[2 * m]);
    const float dc = __fsub_rn(__fadd_rn(a.k0[1], (float)c), a.centres[2 * m + 1]);
    const float gr = expf(__fmul_rn(a.coef[0], __fmul_rn(dr, dr))), gc = expf(__fmul_rn(a.coef[1], __fmul_rn(dc, dc)));
    a.label_out[i] = __fmul_rn(gr, gc);
}

bool even_kernel(const pt_mot_frame* f) {
    return fmodf(f->kernel_size[0] + 1.0f, 2.0f) != 0.0f || fmodf(f->kernel_size[1] + 1.0f, 2.0f) != 0.0f;
}

}  // namespace

extern "C" const char* pt_mot_strerror(int status) {
    switch (status) {
        case PT_MOT_OK: return "ok";
        case PT_MOT_ERR_NULL: return "required pointer is NULL";
        case PT_MOT_ERR_SHAPE: return "non-positive or inconsistent dimension";
        case PT_MOT_ERR_UNSUPPORTED: return "configuration not covered by the gfx950 read-out";
        case PT_MOT_ERR_WORKSPACE: return "workspace too small or misaligned";
        case PT_MOT_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown status";
    }
}

extern "C" int pt_mot_abi_version(void) { return 1; }

// Every product / quotient below is a float32 operation in the reference (float32 CPU tensors; Python scalars are rounded to float32 by
// torch's binary ops), so plain `float` arithmetic with contraction off reproduces the values bit for bit.
#pragma clang fp contract(off)
extern "C" int pt_mot_constants_f32(const pt_mot_frame* f, const pt_mot_object* ob, int H, int W, pt_mot_consts* q) {
    if (!f || !ob || !q) return PT_MOT_ERR_NULL;
    if (H <= 0 || W <= 0) return PT_MOT_ERR_SHAPE;
    if (even_kernel(f)) return PT_MOT_ERR_UNSUPPORTED;
    const int dim[2] = {H, W};
    const float sf = (float)f->scale_factor, tns = (float)f->target_neighborhood_scale;
    for (int d = 0; d < 2; ++d) {
        const float out = (float)dim[d] - fmodf(f->kernel_size[d] + 1.0f, 2.0f);   // output_sz = score_sz - (kernel_size + 1) % 2
        const float ratio = (f->img_support_sz[d] / out) / sf;                     // (img_support_sz / output_sz) / scale_factor
        q->center[d] = ob->pos[d] / ratio;                                         // tamos.py:372
        q->neigh[d] = (ob->target_sz[d] / ratio) * tns;                            // tamos.py:394
        q->prev[d] = (ob->pos[d] - ob->pos_prev[d]) / ratio;                       // tamos.py:408
    }
    q->disp_threshold = (float)(f->dispalcement_scale * sqrt((double)(H * W)) / 2);  // tamos.py:414
    q->reserved = 0.f;
    return PT_MOT_OK;
}

extern "C" int pt_mot_readout_f32(const float* scores, int Hs, int Ws, const float* ltrb, int H, int W, int T, const int* active,
                                  int n_active, const pt_mot_object* objects, const pt_mot_frame* f, float* map_out, float* rec, float seq,
                                  void* stream) {
    if (!scores || !ltrb || !active || !objects || !f || !rec) return PT_MOT_ERR_NULL;
    if (Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || f->stride <= 0 || f->image_h <= 0 || f->image_w <= 0) return PT_MOT_ERR_SHAPE;
    if (T < 1 || T > PT_MOT_MAX_OBJECTS || n_active < 1 || n_active > T) return PT_MOT_ERR_UNSUPPORTED;
    if ((long)H * W > PT_MOT_MAX_CELLS || (long)Hs * Ws > (1L << 24)) return PT_MOT_ERR_UNSUPPORTED;
    if (f->score_preprocess != 0 || f->score_filter_ksz > 1 || f->window_output || !f->advanced_localization || even_kernel(f))
        return PT_MOT_ERR_UNSUPPORTED;
    if ((Hs == H) != (Ws == W)) return PT_MOT_ERR_SHAPE;
    unsigned seen = 0;
    for (int i = 0; i < n_active; ++i) {
        if (active[i] < 0 || active[i] >= T || (seen >> active[i] & 1u)) return PT_MOT_ERR_SHAPE;
        seen |= 1u << active[i];
    }
    // xs.reshape(s1, s2) of direct_bbox_regression: the location grid of the stride has the map's size
    if ((int)ceilf(f->img_sample_sz[0] / (float)f->stride) != H || (int)ceilf(f->img_sample_sz[1] / (float)f->stride) != W)
        return PT_MOT_ERR_SHAPE;
    MotArgs a{};
    a.scores = scores; a.ltrb = ltrb; a.map_out = map_out; a.rec = rec;
    a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.upsample = Hs != H; a.normalize = f->normalize_scores != 0;
    a.seq = seq;
    a.th_not_found = f->target_not_found_threshold; a.th_uncertain = f->uncertain_threshold; a.th_hard_sample = f->hard_sample_threshold;
    a.th_distractor = (float)f->distractor_threshold; a.th_hard_negative = (float)f->hard_negative_threshold;
    a.th_not_found_f32 = (float)f->target_not_found_threshold;
    a.train_w = f->train_img_sample_sz[1]; a.train_h = f->train_img_sample_sz[0];
    a.sample_w = f->img_sample_sz[1]; a.sample_h = f->img_sample_sz[0];
    for (int k = 0; k < 4; ++k) a.sc[k] = f->sample_coords[k];
    a.image_w = (float)f->image_w; a.image_h = (float)f->image_h; a.min_w = (float)f->min_width; a.min_h = (float)f->min_height;
    a.stride = f->stride;
    for (int i = 0; i < n_active; ++i) {
        a.active[i] = active[i];
        const int rc = pt_mot_constants_f32(f, objects + i, H, W, &a.c[i]);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_mot_readout, dim3(n_active), dim3(256), 0, (hipStream_t)stream, a);
    PT_MOT_CHECK_LAUNCH();
    return PT_MOT_OK;
}

extern "C" int pt_mot_wait_f32(const float* rec_host, const int* active, int n_active, float seq, void* stream) {
    if (!rec_host || !active) return PT_MOT_ERR_NULL;
    if (n_active < 1 || n_active > PT_MOT_MAX_OBJECTS) return PT_MOT_ERR_SHAPE;
    for (int i = 0; i < n_active; ++i)
        if (active[i] < 0 || active[i] >= PT_MOT_MAX_OBJECTS) return PT_MOT_ERR_SHAPE;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n_active;) {
        const volatile float* word = rec_host + (long)active[i] * PT_MOT_REC_FLOATS + PT_MOT_R_SEQ;
        if (__atomic_load_n((const volatile int*)word, __ATOMIC_ACQUIRE) == __builtin_bit_cast(int, seq)) { ++i; continue; }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return PT_MOT_ERR_LAUNCH;
            break;
        }
    }
    return PT_MOT_OK;
}

extern "C" int pt_mot_targets_f32(const float* boxes, int nb, int out_h, int out_w, int stride, float* ltrb_out, const pt_mot_label* label,
                                  const float* centres, int n_centres, float* label_out, void* stream) {
    if (nb < 0 || n_centres < 0 || (nb == 0 && n_centres == 0)) return PT_MOT_ERR_SHAPE;
    if (nb > 0 && (!boxes || !ltrb_out)) return PT_MOT_ERR_NULL;
    if (n_centres > 0 && (!label || !centres || !label_out)) return PT_MOT_ERR_NULL;
    TargetArgs a{};
    if (nb > 0) {
        if (out_h <= 0 || out_w <= 0 || stride <= 0) return PT_MOT_ERR_SHAPE;
        if (out_h % stride || out_w % stride || nb > (1 << 16)) return PT_MOT_ERR_UNSUPPORTED;
        a.boxes = boxes; a.ltrb_out = ltrb_out; a.nb = nb; a.H3 = out_h / stride; a.W3 = out_w / stride; a.stride = stride;
        a.out_w = (float)out_w; a.out_h = (float)out_h;
    }
    if (n_centres > 0) {
        if (n_centres > PT_MOT_MAX_CENTRES) return PT_MOT_ERR_UNSUPPORTED;
        int L[2];
        for (int d = 0; d < 2; ++d) {
            const double sz = label->sz[d], ep = label->end_pad[d];
            if (!(sz >= 1) || !(ep >= 0) || !(label->sigma[d] > 0) || sz > 4096 || ep > 4096) return PT_MOT_ERR_SHAPE;
            const double start = -(sz - 1) / 2, end = (sz + 1) / 2 + ep;              // torch.arange(start, end): ceil(end - start) samples
            L[d] = (int)ceil(end - start);
            a.k0[d] = (float)start;
            a.coef[d] = (float)(-1.0 / (2 * pow(label->sigma[d], 2.0)));
        }
        a.LH = L[0]; a.LW = L[1]; a.n_centres = n_centres; a.label_out = label_out;
        for (int i = 0; i < 2 * n_centres; ++i) a.centres[i] = centres[i];
    }
    const long total = (long)a.nb * 4 * a.H3 * a.W3 + (long)a.n_centres * a.LH * a.LW;
    if (total <= 0 || total > (1L << 30)) return PT_MOT_ERR_SHAPE;
    hipLaunchKernelGGL(k_mot_targets, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PT_MOT_CHECK_LAUNCH();
    return PT_MOT_OK;
}
