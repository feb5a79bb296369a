// Gauss-Newton steepest descent on the hinge residual (reference: ltr/models/meta/steepestdescent.py:32-105 driving
// ltr/models/target_classifier/residual_modules.py:LinearFilterHinge, forward :109-135) for one sequence.
//
// The recurrence is DiMPSteepestDescentGN's (optimizer.py:85-170) with step length 1, reg = filter_reg^2 (no min_filter_reg) and
// alpha_eps = steplength_reg; only the maps differ: label and mask come from the caller's label map instead of the radial look-up
// tables,
//   m = min((label > hinge_threshold) + activation_leak, 1);  label <- m * label;  sws = sqrt(sample_weight) (sqrt(1/n) when none).
// The derivatives autograd takes of LeakyReluPar / BentIdentPar are the reference's *Deriv modules (sign(0) = 0), so every pass of the
// DiMP kind (k_corr2, k_adj2, k_fast_sgq2, k_fast_final; k_sd_pw on the generic route) runs unchanged on these operands.  New here:
//   k_gn_hinge_init2   fast-route init stage: s_0 from the slices + maps + the packed operands k_adj2 / k_fast_sgq2 read
//   k_gn_hinge_maps    generic-route maps (the role of k_sd_maps)
//   k_gn_hinge_loss    the GN loss normalisation  loss_t = (sum r^2 + reg |w_t|^2) / (n*OH*OW + C*K*K)   (steepestdescent.py:27-28)
#include "common.h"
#include "pt_internal.h"
#include "sd_common.h"

#define PT_GH_MAXKS 16

// one element of the hinge maps (residual_modules.py:128-130)
__device__ __forceinline__ void gn_hinge_elem(float lab, float thr, float leak, float& lb, float& m) {
    m = fminf((lab > thr ? 1.0f : 0.0f) + leak, 1.0f);
    lb = m * lab;
}

struct GnHingeOut { float *s, *label, *mask, *sws, *lms, *pk; };

// s_0 = sum of the KS channel-range slices (fixed order, as k_fast_init2); maps; packed operands in the DiMP kind's packing
// (PReg, fast_passes.hip): bentpar {s, 0, label, mask}, relu {sws^2 s, 0, sws^2 label, mask}.  One element per thread; the map element,
// the sample weight and the slice partials are requested together before the first wait.
//   pa = n | OO << 16;   pb = KS | bentpar << 8
__global__ __launch_bounds__(1024) void k_gn_hinge_init2(const float* __restrict__ spart, const float* __restrict__ lab_in,
                                                         const float* __restrict__ swp, unsigned pa, unsigned pb, float thr, float leak,
                                                         GnHingeOut out) {
    const int n = (int)(pa & 0xffffu), OO = (int)(pa >> 16);
    const int KS = (int)(pb & 255u);
    const bool bent = ((pb >> 8) & 1u) != 0;
    const int i = blockIdx.x, o = threadIdx.x;
    if (o >= OO) return;
    const long q = (long)i * OO + o;
    float v[PT_GH_MAXKS];
    {
        const float* p = spart + q;
        const long st = (long)n * OO;
#pragma unroll
        for (int k = 0; k < PT_GH_MAXKS; ++k) v[k] = p[(long)min(k, KS - 1) * st];
    }
    const float lab = lab_in[q];
    const float swv = swp ? swp[i] : 1.0f / (float)n;
    float s0 = 0.f;
#pragma unroll
    for (int k = 0; k < PT_GH_MAXKS; ++k) s0 += k < KS ? v[k] : 0.f;
    float lb, m;
    gn_hinge_elem(lab, thr, leak, lb, m);
    const float sw = sqrtf(swv);
    out.s[q] = s0;
    out.label[q] = lb;
    out.mask[q] = m;
    out.sws[q] = sw;
    ((f32x4*)out.lms)[q] = (f32x4){lb, m, sw, 0.f};
    f32x4 pk;
    if (bent) pk = (f32x4){s0, 0.f, lb, m};
    else { const float w2 = sw * sw; pk = (f32x4){w2 * s0, w2 * 0.f, w2 * lb, m}; }
    ((f32x4*)out.pk)[q] = pk;
}

// generic route: label / mask / weight maps of sample blockIdx.x (what k_sd_maps writes for the DiMP kind)
__global__ void k_gn_hinge_maps(const float* __restrict__ lab_in, const float* __restrict__ swp, int n, int OO, float thr, float leak,
                                float* __restrict__ label, float* __restrict__ mask, float* __restrict__ sws) {
    const int i = blockIdx.x;
    const float sw = sqrtf(swp ? swp[i] : 1.0f / (float)n);
    for (int o = threadIdx.x; o < OO; o += blockDim.x) {
        const long q = (long)i * OO + o;
        float lb, m;
        gn_hinge_elem(lab_in[q], thr, leak, lb, m);
        label[q] = lb;
        mask[q] = m;
        sws[q] = sw;
    }
}

// losses[t] /= numel of the residual vector (steepestdescent.py:27-28: sum(r*r) / sum(numel))
__global__ void k_gn_hinge_loss(float* __restrict__ losses, int count, float numel) {
    for (int t = threadIdx.x; t < count; t += blockDim.x) losses[t] = losses[t] / numel;
}

int pt_launch_gn_hinge_init2(const SdArgs& a, const PtLabelMap& lm, hipStream_t st) {
    if (a.KS > PT_GH_MAXKS || a.OO > 1024 || a.n > 65535 || a.OO > 65535 || !a.lms || !a.pk) return PT_ERR_UNSUPPORTED;
    const int threads = ((a.OO + 63) / 64) * 64;
    const GnHingeOut out = {a.s, a.label, a.mask, a.sws, a.lms, a.pk};
    hipLaunchKernelGGL(k_gn_hinge_init2, dim3(a.n), dim3(threads), 0, st, (const float*)a.spart, lm.label, a.has_sw ? a.sw : (const float*)nullptr,
                       (unsigned)a.n | ((unsigned)a.OO << 16), (unsigned)a.KS | ((unsigned)(a.score_act == PT_ACT_BENTPAR ? 1 : 0) << 8),
                       lm.thr, lm.leak, out);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

int pt_launch_gn_hinge_maps(const SdArgs& a, const PtLabelMap& lm, hipStream_t st) {
    hipLaunchKernelGGL(k_gn_hinge_maps, dim3(a.n), dim3(256), 0, st, lm.label, a.has_sw ? a.sw : (const float*)nullptr, a.n, a.OO,
                       lm.thr, lm.leak, a.label, a.mask, a.sws);
    PT_CHECK_LAUNCH();
    return PT_OK;
}

extern "C" size_t pt_gn_hinge_ws_bytes(int n, int C, int H, int W, int K) { return pt_sd_ws_bytes(n, C, H, W, K); }

extern "C" int pt_gn_hinge_solve_f32(const pt_gn_hinge_params* p, const float* w_in, const float* feat, long feat_stride_n,
                                     const float* label, const float* sample_weight, int n, int C, int H, int W, int K, int num_iter,
                                     float* w_iters, float* losses, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w_in || !feat || !label || !w_iters || !ws) return PT_ERR_NULL;
    if (n <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0 || num_iter < 0) return PT_ERR_SHAPE;
    if (feat_stride_n < (long)C * H * W) return PT_ERR_SHAPE;
    if (K * K > 16 || num_iter > PT_SD_MAX_ITER) return PT_ERR_UNSUPPORTED;
    if (p->score_act != PT_ACT_RELU && p->score_act != PT_ACT_BENTPAR) return PT_ERR_UNSUPPORTED;
    const int OH = H + (K + 1) % 2, OW = W + (K + 1) % 2;
    if ((long)n * OH * OW > (1L << 30) || n > 65535) return PT_ERR_UNSUPPORTED;   // (checked here: nothing may be queued before a refusal)
    if (ws_bytes < pt_gn_hinge_ws_bytes(n, C, H, W, K)) return PT_ERR_WORKSPACE;
    pt_sd_params sp = {};
    sp.kind = PT_SD_DIMP;                  // the DiMP kind's passes; its look-up tables are replaced by the label map
    sp.step_length = 1.0f;
    sp.reg = p->filter_reg * p->filter_reg;
    sp.alpha_eps = p->steplength_reg;
    sp.score_act = p->score_act;
    sp.act_param = p->act_param;
    sp.mask_act = PT_MASK_LINEAR;
    const PtLabelMap lm = {label, p->hinge_threshold, p->activation_leak};
    hipStream_t st = (hipStream_t)stream;
    const int rc = pt_sd_solve_impl(&sp, w_in, feat, feat_stride_n, /*bb=*/nullptr, sample_weight, n, C, H, W, K, num_iter, w_iters, losses,
                                    ws, ws_bytes, st, /*copy_w0=*/true, /*w_final=*/nullptr, /*cls=*/nullptr, /*src=*/nullptr, nullptr, false,
                                    &lm);
    if (rc || !losses) return rc;
    hipLaunchKernelGGL(k_gn_hinge_loss, dim3(1), dim3(64), 0, st, losses, num_iter + 1, (float)((long)n * OH * OW + (long)C * K * K));
    PT_CHECK_LAUNCH();
    return PT_OK;
}

// which route pt_gn_hinge_solve_f32 takes for these operands (1: the XCD-aligned fast route): the solve's own predicate
// (pt_sd_route_fast), evaluated on the host, nothing launched.  The Python mirror reads it with the pointers it passes to the solve.
extern "C" int pt_gn_hinge_route(const float* feat, long feat_stride_n, const float* w_in, const float* w_iters, int n, int C, int H, int W,
                                 int K) {
    if (n <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return PT_ERR_SHAPE;
    const int OH = H + (K + 1) % 2, OW = W + (K + 1) % 2;
    const PtFast f = pt_fast_plan(n, C, H, W, K, K, OH, OW);
    return pt_sd_route_fast(f, feat, feat_stride_n, w_in, w_iters, nullptr, 0, true) ? 1 : 0;
}
