/*
 * pt_hot.h -- C ABI of libpt_hot.so: the MI355X (gfx950) implementation of PyTracking's per-frame
 * online model-optimisation hot path.
 *
 * The reference (visionml/pytracking) has no FFI of its own on this path -- its operator API is a set of
 * Python callables.  Each entry point below names the reference callable it replaces
 * (paths relative to the reference root); the host-side mirror that binds them lives in
 * pytracking_amd/ (ctypes), and INTEGRATION.md shows the stub a maintainer would add to the reference.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer to contiguous fp32 unless stated;
 *   - the caller owns every buffer; the library never allocates or frees device memory and keeps no
 *     global state; scratch space is passed in (`ws`, sized by the matching *_ws_bytes());
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream), no device
 *     synchronisation, no host callbacks -> every call is hipGraph-capturable;
 *   - returns PT_OK (0) or a negative pt_status; nothing is launched when an argument check fails;
 *   - layouts are the reference's: feature maps NCHW (n, C, H, W), filters (C, KH, KW), boxes xywh.
 */
#ifndef PT_HOT_H
#define PT_HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pt_status {
    PT_OK = 0,
    PT_ERR_NULL = -1,        /* required pointer is NULL */
    PT_ERR_SHAPE = -2,       /* non-positive or inconsistent dimension */
    PT_ERR_UNSUPPORTED = -3, /* valid request the kernels do not cover (e.g. KH*KW > 16 in the fused solver) */
    PT_ERR_WORKSPACE = -4,   /* workspace too small / misaligned */
    PT_ERR_LAUNCH = -5       /* hipGetLastError() != hipSuccess after a launch */
} pt_status;

const char* pt_strerror(int status);
/* ABI version; bumped when a signature changes. */
int pt_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Filter layer -- ltr/models/layers/filter.py
 * ---------------------------------------------------------------------------------------------- */

/* apply_filter (filter.py:5-57), one sequence, one filter:
 *   scores[i,y,x] = sum_{c,u,v} feat[i,c,y+u-KH/2,x+v-KW/2] * filt[c,u,v]      (zero padded)
 * feat (n,C,H,W) with sample stride `feat_stride_n` floats (= C*H*W when dense; S*C*H*W for a 5-D
 * (n,S,C,H,W) tensor, the caller then loops over sequences); filt (C,KH,KW); scores (n,OH,OW) dense.
 * OH/OW may be the full correlation size H+2*(KH/2)-KH+1 (reference apply_filter) or anything smaller:
 * the top-left OHxOW corner is produced (pytracking/libs/operation.py:17-32 conv2d(mode='same')).
 * Requires KH*KW <= 16. */
/* Launch geometry of the XCD-aligned correlation pass for this shape, evaluated on the host, nothing launched:
 * out[0..9] = usable, tiles, k-step halves per tile, samples per workgroup, mixed pair layout, threads per workgroup, k-steps per wave,
 * channel ranges, dynamic LDS bytes, leftover-quad tile.  Returns 0, or PT_ERR_NULL. */
int pt_corr_pass_plan(int n, int C, int H, int W, int KH, int KW, int OH, int OW, int* out);
/* What the correlation launcher dispatches on beyond those ten fields, host only:
 * out[0..3] = usable, uniform-step 4x4 shift-and-add, quads behind the last full 64-position tile (0..15), and how they run
 * (0: none, 1: leftover quads on tile 0's wave, 2: a partial tile of its own).  Returns 0, or PT_ERR_NULL. */
int pt_corr_pass_tail(int n, int C, int H, int W, int KH, int KW, int OH, int OW, int* out);
/* Launch geometry of the XCD-aligned adjoint pass and the instantiation its dispatcher launches, host only:
 * out[0..10] = usable, map elements per lane E, compile-time groups per wave UM, groups per wave U, position slices, groups per slice,
 * 16-channel blocks, channel blocks per XCD (0: fewer blocks than XCDs), residual maps a workgroup holds at most, padded map row,
 * dynamic LDS bytes.  All 0 when the shape is not covered.  Returns 0, or PT_ERR_NULL. */
int pt_adj_pass_plan(int n, int C, int H, int W, int KH, int KW, int OH, int OW, int* out);
size_t pt_apply_filter_ws_bytes(int n, int C, int H, int W, int KH, int KW, int OH, int OW);
int pt_apply_filter_f32(const float* feat, long feat_stride_n, const float* filt, float* scores,
                        int n, int C, int H, int W, int KH, int KW, int OH, int OW,
                        void* ws, size_t ws_bytes, void* stream);

/* apply_feat_transpose (filter.py:91-182; _v2 and _v3 compute the same quantity):
 *   grad[c,u,v] = sum_{i,y,x} feat[i,c,y+u-KH/2,x+v-KW/2] * inp[i,y,x]
 * inp (n,OH,OW) dense; grad (C,KH,KW).  Requires KH*KW <= 16 (16-byte loads when (H*W) % 4 == 0). */
size_t pt_feat_transpose_ws_bytes(int n, int C, int H, int W, int KH, int KW, int OH, int OW);
int pt_feat_transpose_f32(const float* feat, long feat_stride_n, const float* inp, float* grad,
                          int n, int C, int H, int W, int KH, int KW, int OH, int OW,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Steepest-descent filter optimisers -- ltr/models/target_classifier/optimizer.py
 * ---------------------------------------------------------------------------------------------- */

enum { PT_SD_DIMP = 0, PT_SD_DIMP_L2 = 1, PT_SD_PRDIMP = 2 };
enum { PT_ACT_RELU = 0, PT_ACT_BENTPAR = 1 };       /* score_act (optimizer.py:74-82) */
enum { PT_MASK_SIGMOID = 0, PT_MASK_LINEAR = 1 };   /* mask_act  (optimizer.py:58-66) */

/* Host-side parameter block, read at call time (the trackers mutate the module attributes at run
 * time, pytracking/tracker/dimp/dimp.py:589-602, so nothing is baked in). */
typedef struct pt_sd_params {
    int   kind;            /* PT_SD_* */
    float step_length;     /* exp(log_step_length)                               optimizer.py:108 */
    float reg;             /* max(filter_reg^2, min_filter_reg^2)                optimizer.py:109 */
    float alpha_eps;       /*                                                    optimizer.py:156 */
    float feat_stride;     /*                                                    optimizer.py:113 */
    /* PT_SD_DIMP: learned radial look-up tables = the three 1x1 conv weights (optimizer.py:57-72).
     * DEVICE pointers to `num_bins` floats each. */
    int   num_bins;
    float bin_displacement;
    const float* label_lut;
    const float* mask_lut;
    const float* spatial_lut;
    int   mask_act;        /* PT_MASK_* */
    int   score_act;       /* PT_ACT_*  */
    float act_param;       /* BentIdentPar b */
    /* PT_SD_DIMP_L2 (optimizer.py:174-291) */
    float gauss_sigma;     /* also PT_SD_PRDIMP */
    float hinge_threshold;
    /* PT_SD_PRDIMP (optimizer.py:294-439) */
    float uni_weight;
    int   normalize_label;
    float label_shrink;
    int   has_softmax_reg;
    float softmax_reg;
    float label_threshold;
} pt_sd_params;

/* {DiMPSteepestDescentGN, DiMPL2SteepestDescentGN, PrDiMPSteepestDescentNewton}.forward for one
 * sequence (optimizer.py:85-170, 211-291, 355-439):
 *   w_in (C,K,K) is not modified; w_iters receives all num_iter+1 iterates ((num_iter+1),C,K,K),
 *   w_iters[0] = w_in; losses (num_iter+1 floats) may be NULL (= compute_losses False);
 *   bb (n,4) xywh in crop pixels; sample_weight (n) or NULL.
 * Requires K*K <= 16 (feature loads are 16-byte wide when (H*W) % 4 == 0, scalar otherwise). */
size_t pt_sd_ws_bytes(int n, int C, int H, int W, int K);
int pt_sd_solve_f32(const pt_sd_params* p, const float* w_in, const float* feat, long feat_stride_n,
                    const float* bb, const float* sample_weight,
                    int n, int C, int H, int W, int K, int num_iter,
                    float* w_iters, float* losses, void* ws, size_t ws_bytes, void* stream);

/* Route pt_sd_solve_f32 takes for exactly these operands -- the solve's own checks, predicate and dispatch helpers, evaluated on the
 * host, nothing launched: out[0] = 1 XCD-aligned fast route / 0 generic; on the fast route out[1] = residual provider of the adjoint pass
 * (1 DiMP relu, 2 DiMP bent identity, 3 DiMP-L2, 4 PrDiMP), out[2] = width of the fused gradient reduction (8 | 16 partials),
 * out[3] = 1 when the last update runs with the loss read-out.  Returns 0 or the status the solve would return for the shape. */
int pt_sd_solve_route(const pt_sd_params* p, const float* w_in, const float* feat, long feat_stride_n, const float* w_iters,
                      int n, int C, int H, int W, int K, int want_losses, int* out);

/* S independent sequences in one call (optimizer.py:101-104 `num_sequences`; KYS / multi-object wrappers call the optimiser with
 * S > 1).  Arrays of S pointers (host arrays of device pointers); sample_weight / losses may be NULL as arrays; ws: S workspaces of
 * ws_bytes_each >= pt_sd_ws_bytes each.  Sequence s runs on `stream` (s % (1 + n_aux) == 0) or on aux_streams[s % (1 + n_aux) - 1]:
 * the auxiliary streams wait for everything queued on `stream` before the call and `stream` waits for them before the call
 * returns, so the call is ordered on `stream` like pt_sd_solve_f32.  n_aux = 0: the sequences run back to back. */
int pt_sd_solve_batch_f32(const pt_sd_params* p, int S, const float* const* w_in, const float* const* feat, long feat_stride_n,
                          const float* const* bb, const float* const* sample_weight, int n, int C, int H, int W, int K,
                          int num_iter, float* const* w_iters, float* const* losses, void* const* ws, size_t ws_bytes_each,
                          void* stream, void* const* aux_streams, int n_aux);

/* GNSteepestDescent.forward (ltr/models/meta/steepestdescent.py:32-105) on LinearFilterHinge
 * (ltr/models/target_classifier/residual_modules.py:88-135), one sequence -- DiMP-simple's and the RTS classifier's online solver:
 *   m = min((label > hinge_threshold) + activation_leak, 1); residuals [sw*(act(F w, m) - m*label), filter_reg*w];
 *   act = LeakyReluPar (PT_ACT_RELU) or BentIdentPar(act_param) (PT_ACT_BENTPAR); sw = sqrt(sample_weight[i]), sqrt(1/n) when NULL;
 *   alpha = |g|^2 / max(|J g|^2 + steplength_reg |g|^2, 1e-8) with the filter_reg^2 |g|^2 term inside |J g|^2; step length 1.
 * label (n,OH,OW), OH = H + (K+1)%2; w_in (C,K,K) is not modified; w_iters receives all num_iter+1 iterates;
 * losses (num_iter+1 floats) may be NULL, else losses[t] = (sum r^2 + filter_reg^2 |w_t|^2) / (n*OH*OW + C*K*K).
 * Requires K*K <= 16 and num_iter <= 64. */
typedef struct {
    int   score_act;       /* PT_ACT_* */
    float act_param;       /* BentIdentPar b */
    float hinge_threshold;
    float activation_leak;
    float filter_reg;      /* the residual's filter_reg (its square is the regulariser) */
    float steplength_reg;  /* GNSteepestDescent.steplength_reg */
} pt_gn_hinge_params;
size_t pt_gn_hinge_ws_bytes(int n, int C, int H, int W, int K);
int pt_gn_hinge_solve_f32(const pt_gn_hinge_params* p, const float* w_in, const float* feat, long feat_stride_n,
                          const float* label, const float* sample_weight, int n, int C, int H, int W, int K, int num_iter,
                          float* w_iters, float* losses, void* ws, size_t ws_bytes, void* stream);
/* Route pt_gn_hinge_solve_f32 takes for exactly these operands -- the solve's own predicate, evaluated on the host, nothing launched:
 * 1 = the XCD-aligned fast route, 0 = the generic one (also every map of more than 1024 elements). */
int pt_gn_hinge_route(const float* feat, long feat_stride_n, const float* w_in, const float* w_iters, int n, int C, int H, int W, int K);

/* ------------------------------------------------------------------------------------------------
 * Multi-filter filter layer + LWL few-shot learner -- ltr/models/layers/filter.py (5-D `filter` / `input` branches),
 * ltr/models/meta/steepestdescent.py, ltr/models/lwl/loss_residual_modules.py
 *   F <= 16 filters per sequence, K in {1, 3} (zero padding K/2: output H x W), W <= 256, groups = 1, no dilation.
 * ---------------------------------------------------------------------------------------------- */

/* apply_filter (filter.py:29-34), one sequence, F filters:  filt (F,C,K,K); scores (n,F,H,W) dense
 *   scores[i,f,y,x] = sum_{c,u,v} filt[f,c,u,v] * feat[i,c,y+u-K/2,x+v-K/2] */
size_t pt_apply_filter_mf_ws_bytes(int n, int F, int C, int H, int W, int K);
int pt_apply_filter_mf_f32(const float* feat, long feat_stride_n, const float* filt, float* scores,
                           int n, int F, int C, int H, int W, int K, void* ws, size_t ws_bytes, void* stream);

/* apply_feat_transpose for a 5-D input (filter.py:158-176):  inp (n,F,H,W) dense; grad (F,C,K,K)
 *   grad[f,c,u,v] = sum_{i,y,x} feat[i,c,y+u-K/2,x+v-K/2] * inp[i,f,y,x] */
size_t pt_feat_transpose_mf_ws_bytes(int n, int F, int C, int H, int W, int K);
int pt_feat_transpose_mf_f32(const float* feat, long feat_stride_n, const float* inp, float* grad,
                             int n, int F, int C, int H, int W, int K, void* ws, size_t ws_bytes, void* stream);

/* GNSteepestDescent.forward (steepestdescent.py:32-105) on LWTLResidual (loss_residual_modules.py:16-41), one sequence:
 *   residuals [sw*(apply_filter(feat,w) - label), filter_reg*w]; w_in (F,C,K,K) is not modified; w_iters receives the
 *   num_iter+1 iterates; losses (num_iter+1 floats) may be NULL; label (n,F,H,W);
 *   sw_mode 0: sample_weight ignored (sqrt(1/n), :27-28), 1: (n) per image, 2: (n,F,H,W) per element (:29-33). */
size_t pt_lwl_ws_bytes(int n, int F, int C, int H, int W, int K);
int pt_lwl_gn_solve_f32(const float* w_in, const float* feat, long feat_stride_n, const float* label,
                        const float* sample_weight, int sw_mode, float filter_reg, float steplength_reg,
                        int n, int F, int C, int H, int W, int K, int num_iter,
                        float* w_iters, float* losses, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ATOM conjugate gradient -- pytracking/libs/optimization.py:72-163,227-289 (ConjugateGradient.run +
 * run_CG) specialised to pytracking/tracker/atom/optim.py:71-99 (ConvProblem) with the MLU response
 * activation (ltr/models/layers/activation.py:20-29).
 *   x (C,K,K) is updated IN PLACE (optimization.py:259-260); samples (n,C,H,W); y (n,H,W);
 *   sample_weights (n).  cg_state: 2*C*K*K+4 floats the caller keeps between calls
 *   (p, r_prev, rho, has_p) -- only consulted when direction_forget_factor != 0.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_atom_cg_ws_bytes(int n, int C, int H, int W, int K);
int pt_atom_cg_f32(float* x, const float* samples, long samples_stride_n, const float* y,
                   const float* sample_weights, float filter_reg, float act_min_val,
                   int n, int C, int H, int W, int K, int num_iter, int fletcher_reeves,
                   float direction_forget_factor, float* cg_state,
                   void* ws, size_t ws_bytes, void* stream);
/* Route pt_atom_cg_f32 takes for exactly these operands -- the update's own shape checks and route predicate, evaluated on the host,
 * nothing launched or allocated.  Fused route (C = 64, 4x4 filter, 4 or 5 position tiles, aligned operands):
 *   out = {1, position tiles, tail (0 none, 1 leftover quads on tile 0's wave, 2 a partial tile of its own), leftover quads, adjoint slices};
 * generic route: out = {0, 16-byte feature loads (0 | 1), k-step arm of the correlation kernel (16 | 8 | 4, 0 = run-time count),
 * channel slices, adjoint slices}.  Returns 0 or the status the update returns for the shape; `out` (5 ints) is zeroed then. */
int pt_atom_cg_route(const float* x, const float* samples, long samples_stride_n, const float* cg_state,
                     int n, int C, int H, int W, int K, int* out);

/* ATOM first-frame joint optimisation -- GaussNewtonCG.run (pytracking/libs/optimization.py:328-421) on
 * FactorizedConvProblem (pytracking/tracker/atom/optim.py:6-68), identity projection activation, MLU response activation:
 *   filter (Kc,K,K) and proj (Kc,M) [= the reference's (Kc,M,1,1)] are updated IN PLACE (optimization.py:403-404);
 *   samples (n,M,H,W) uncompressed features; y (n,H,W); sample_weights (n);
 *   cg_iters: HOST array of num_gn CG iteration counts, one Gauss-Newton iteration each (optimization.py:340-358);
 *   CG state is reset at every Gauss-Newton iteration (direction_forget_factor = 0, the tracker's setting). */
size_t pt_atom_gn_ws_bytes(int n, int M, int Kc, int H, int W, int K);
int pt_atom_gn_f32(float* filter, float* proj, const float* samples, long samples_stride_n, const float* y,
                   const float* sample_weights, float filter_reg, float projection_reg, float act_min_val,
                   int n, int M, int Kc, int H, int W, int K, const int* cg_iters, int num_gn, int fletcher_reeves,
                   void* ws, size_t ws_bytes, void* stream);
/* Routes of pt_atom_gn_f32 for exactly these samples -- the entry's own checks and dispatch helpers, evaluated on the host, nothing
 * launched or allocated (the other operands are the caller's 16-byte aligned arrays and the 256-byte aligned workspace).  out (10 ints):
 *   [0] conv1x1 arm (0 weights read in place, 1 banks of 16 rows in one launch, 2 one launch per group of <= 16 rows),
 *   [1] projection-adjoint arm (0 batched GEMM, 1 banked multi-filter adjoint, 2 one launch per group),
 *   [2] groups of 16 projection rows, [3] sample groups of the projection-adjoint partials, [4] 1 = the CG step's two correlations
 *   share one launch, [5] grid.z of the filter adjoint (1 + input-gradient layers), [6] 16-byte loads of the compressed maps,
 *   [7] k-step arm of the correlation kernel (16 | 8 | 4, 0 = run-time count), [8] channel slices, [9] adjoint slices.
 * Returns 0 or the status the entry returns for the shape; `out` is zeroed then. */
int pt_atom_gn_route(const float* samples, long samples_stride_n, int n, int M, int Kc, int H, int W, int K, int* out);

/* ------------------------------------------------------------------------------------------------
 * ToMP transformer model predictor -- replaces, for inference,
 *   FilterPredictor.predict_filter / predict_cls_bbreg_filters_parallel  (ltr/models/transformer/filter_predictor.py:50-150)
 *   Transformer.forward, post-norm encoder/decoder layers                (ltr/models/transformer/transformer.py:90-96,172-180,224-238)
 *   PositionEmbeddingSine('lin_sine', avoid_aliazing=True)               (ltr/models/transformer/position_encoding.py:6-58)
 *   DenseBoxRegressor.forward and the Linear of LinearFilterClassifier   (ltr/models/transformer/heads.py:93-98,119-141)
 *
 * Parameters travel as ONE contiguous fp32 device buffer ("pack"), tensors in the reference's own layouts, in this order
 * (names = the reference's state_dict keys below `filter_predictor.`):
 *   for each encoder layer i:  transformer.encoder.layers.i.{self_attn.in_proj_weight (3D,D), self_attn.in_proj_bias (3D),
 *       self_attn.out_proj.weight (D,D), self_attn.out_proj.bias (D), linear1.weight (F,D), linear1.bias (F),
 *       linear2.weight (D,F), linear2.bias (D), norm1.weight, norm1.bias, norm2.weight, norm2.bias (D each)}
 *   for each decoder layer i:  transformer.decoder.layers.i.{self_attn.[4 tensors as above], multihead_attn.[4 tensors],
 *       linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.*, norm2.*, norm3.* (weight, bias)}
 *   transformer.decoder.norm.{weight, bias}
 *   box_encoding.0.{weight (D/4,4), bias}, box_encoding.1.{weight, bias, running_mean, running_var} (D/4 each),
 *   box_encoding.3.{weight (D,D/4), bias}, box_encoding.4.{weight, bias, running_mean, running_var} (D each),
 *   box_encoding.6.{weight (D,D), bias}, query_embed_fg.weight (D), query_embed_test.weight (D)
 * pt_tomp_param_floats() returns the length of that buffer (0: configuration not covered).
 *
 * Shapes: train_feat (n_train, n_seq, D, H, W); test_feat (1, n_seq, D, H, W); train_label (n_train, n_seq, H, W);
 * train_ltrb (n_train, n_seq, 4, H, W); pos (H*W, D) from pt_tomp_posenc_f32 (input independent: compute once, keep).
 *   parallel = 0: predict_filter            -> filters (n_seq, D), enc_feat (n_seq, D, H, W)
 *   parallel = 1: predict_cls_bbreg_filters_parallel (n_seq must be 1, as the reference's mask row 1 assumes):
 *                 filters (2, D) = [cls, bbreg], enc_feat (2, D, H, W) = [cls, bbreg]; the memory frames
 *                 [num_gth_frames, n_train) are masked out as keys for the bbreg row (filter_predictor.py:134-136)
 * Covered: d_model in {128,256,384,512}, head dim in {16,32,64}, dim_ff % 64 == 0, <= 16 layers each, <= 8 batch rows.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pt_tomp_dims {
    int d_model, nhead, dim_ff, n_enc, n_dec;
    int H, W;          /* feature map of every frame */
    int max_res;       /* `feature_sz` of FilterPredictor (anti-aliasing factor of the positional encoding) */
} pt_tomp_dims;
size_t pt_tomp_param_floats(const pt_tomp_dims* dims);
/* Weight-only products of the decoder, folded once per weight update into a second caller-owned buffer of
 * pt_tomp_prepared_floats() floats (one query token per batch row makes self-attention, the query/key product and
 * value + out_proj plain matrix-vector products: W_o W_v, W_k,h^T W_q,h / sqrt(d_h), W_o[:,h] W_v,h and their biases; the
 * decoder starts from zeros, so the first layer's state after self-attention and its folded query are constants of the
 * weights and are stored here as well). */
size_t pt_tomp_prepared_floats(const pt_tomp_dims* dims);
int pt_tomp_prepare_f32(const pt_tomp_dims* dims, const float* params, float* prepared, void* stream);
int pt_tomp_posenc_f32(float* pos, int H, int W, int d_model, int max_res, void* stream);
size_t pt_tomp_predict_ws_bytes(const pt_tomp_dims* dims, int n_train, int n_seq, int parallel);
int pt_tomp_predict_f32(const pt_tomp_dims* dims, const float* params, const float* prepared, const float* pos,
                        const float* train_feat,
                        const float* test_feat, const float* train_label, const float* train_ltrb,
                        int n_train, int n_seq, int parallel, int num_gth_frames, float* filters, float* enc_feat,
                        void* ws, size_t ws_bytes, void* stream);
/* y (B,N) = [relu](x (B,K) weight(N,K)^T + bias): the Linear applied to the predicted filters (heads.py:95,123), B <= 8 */
int pt_tomp_linear_f32(const float* weight, const float* bias, const float* x, float* y, int B, int N, int K, int relu,
                       void* stream);
/* DenseBoxRegressor.forward (heads.py:119-141): feat (n, D, H, W), filter (D) -> ltrb (n, 4, H, W).
 * pack: linear.weight (D,D), linear.bias (D), then for tower conv i = 0..3: conv weight in (out, ky, kx, in) order
 * [= the reference's (out,in,3,3) tensor permuted (0,2,3,1)], conv bias (D), GroupNorm weight (D), GroupNorm bias (D);
 * then bbreg_layer weight (4, ky, kx, in) and bias (4). */
size_t pt_tomp_bbreg_param_floats(int d_model);
size_t pt_tomp_bbreg_ws_bytes(int n, int d_model, int H, int W);
int pt_tomp_bbreg_f32(const float* params, const float* feat, const float* filter, float* ltrb, int n, int d_model,
                      int H, int W, void* ws, size_t ws_bytes, void* stream);

/* The kernels the three ToMP entry points above would launch, in launch order, as route ids.  Host only: launches nothing, touches
 * no device, allocates nothing.  The queries walk the entry points' own host code and dispatchers, so what they report is what a call
 * with 256-byte aligned buffers (what the Python wrappers allocate) runs; parameter-pack, prepared-buffer and workspace offsets are the
 * real ones.  A launcher-selected kernel has one id per kernel or operand mode; a kernel that is launched unconditionally has one id.
 *   PT_TOMP_R_GEMM_*      launch_gemm: 32 x 32 tiles (plain grid / XCD swizzle / swizzle whose last group of 8 row tiles is partly
 *                         phantom), 64 x 64 tiles, k_gemm_ps 64 x 64 (PS2) and 128 x 64 (PS4, whole K or split-K), each with the
 *                         16-byte epilogue (_WIDE) or the scalar one, k_gemm_big, the 3x3 gather with and without the GroupNorm loader
 *   PT_TOMP_R_ATTN*       k_attn<16 | 32 | 64>
 *   PT_TOMP_R_LN*         k_ln_rows_t<4> plain / with two or four split-K addends + residual / two norms in one, k_ln_rows_t<2>,
 *                         k_ln_rows_t<1>, the generic k_ln_rows
 *   PT_TOMP_R_DEC0_*      no launch: decoder layer 0's first two GEMVs come as prepared constants (CONST) or are launched (LIVE)
 *   PT_TOMP_R_GEMV_*      k_gemv_dec<1 | 2 | 4 | 8>, k_gemv<4>, k_gemv<1>
 *   PT_TOMP_R_GN_APPLY    the tower's unfused GroupNorm (maps under 32 positions, more than 256 slices per image)
 * pt_tomp_predict_routes follows pt_tomp_predict_f32 (the routes do not depend on num_gth_frames), pt_tomp_bbreg_routes
 * pt_tomp_bbreg_f32, pt_tomp_linear_routes pt_tomp_linear_f32.  On PT_OK routes[0 .. *n_routes) are set and the rest of the `cap`
 * entries zeroed.  Otherwise every entry is zeroed and *n_routes = 0: PT_ERR_SHAPE / PT_ERR_UNSUPPORTED exactly where the entry point
 * (and pt_tomp_predict_ws_bytes / pt_tomp_bbreg_ws_bytes) refuses, PT_ERR_WORKSPACE when cap is too small (PT_TOMP_MAX_ROUTES always
 * suffices); PT_ERR_NULL for a null argument. */
enum pt_tomp_route {
    PT_TOMP_R_NONE = 0,
    PT_TOMP_R_TOKENS, PT_TOMP_R_BOX1,
    PT_TOMP_R_GEMM_T32, PT_TOMP_R_GEMM_T32_SWZ, PT_TOMP_R_GEMM_T32_SWZ_PAD, PT_TOMP_R_GEMM_T64,
    PT_TOMP_R_GEMM_PS2_WIDE, PT_TOMP_R_GEMM_PS2, PT_TOMP_R_GEMM_PS4_WIDE, PT_TOMP_R_GEMM_PS4,
    PT_TOMP_R_GEMM_PS4_SPLITK_WIDE, PT_TOMP_R_GEMM_PS4_SPLITK, PT_TOMP_R_GEMM_BIG, PT_TOMP_R_GEMM_CONV, PT_TOMP_R_GEMM_CONV_GN,
    PT_TOMP_R_ATTN16, PT_TOMP_R_ATTN32, PT_TOMP_R_ATTN64,
    PT_TOMP_R_LN256, PT_TOMP_R_LN256_SPLIT2, PT_TOMP_R_LN256_SPLIT4, PT_TOMP_R_LN256_DOUBLE, PT_TOMP_R_LN128, PT_TOMP_R_LN64,
    PT_TOMP_R_LN_GENERIC,
    PT_TOMP_R_DEC0_CONST, PT_TOMP_R_DEC0_LIVE,
    PT_TOMP_R_GEMV_DEC1, PT_TOMP_R_GEMV_DEC2, PT_TOMP_R_GEMV_DEC4, PT_TOMP_R_GEMV_DEC8, PT_TOMP_R_GEMV_V4, PT_TOMP_R_GEMV_V1,
    PT_TOMP_R_DEC_SCORES, PT_TOMP_R_DEC_CTX, PT_TOMP_R_TO_NCHW,
    PT_TOMP_R_REG_ATTEND, PT_TOMP_R_GN_REDUCE, PT_TOMP_R_GN_APPLY, PT_TOMP_R_REG_FINISH,
    PT_TOMP_R_COUNT
};
#define PT_TOMP_MAX_ROUTES 256
int pt_tomp_predict_routes(const pt_tomp_dims* dims, int n_train, int n_seq, int parallel, int* routes, int cap, int* n_routes);
int pt_tomp_bbreg_routes(int n, int d_model, int H, int W, int* routes, int cap, int* n_routes);
int pt_tomp_linear_routes(int B, int N, int K, int* routes, int cap, int* n_routes);

/* ------------------------------------------------------------------------------------------------
 * TaMOs multi-object filter predictor -- replaces, for inference,
 *   GOTFilterPredictor.predict_filter                       (ltr/models/transformer/filter_predictor.py:180-233)
 *   GOTFilterPredictor._predict_cls_bbreg_filters_parallel  (ltr/models/transformer/filter_predictor.py:245-315)
 *   Transformer.forward with T = num_tokens object queries  (ltr/models/transformer/transformer.py:90-96,172-180,224-238)
 * for label_enc = 'gaussian' and box_enc = 'ltrb_token' (ltr/train_settings/tamos/*.py), as the tracker calls it every frame
 * (pytracking/tracker/tamos/tamos.py:289-306).  The classifier's scores come from the multi-filter correlation that exists already.
 * heads.FPN and the multi-object DenseBoxRegressor on the FPN map: pt_fpn2_f32 / pt_tamos_bbreg_f32 below.  Out of scope: TaMOs.track's
 * host glue, training.  pt_tomp_* is unchanged.
 *
 * Pack: pt_tomp's transformer tensors in pt_tomp's order, then the 14 box_encoding tensors in pt_tomp's order, then
 * query_embed_fg.weight (T, D).  There is no test-frame token.  pt_tamos_param_floats() is the length (0: not covered).
 *
 * Shapes, with B = n_seq, or 2 when `parallel`: train_feat (n_train, n_seq, D, H, W); test_feat (1, n_seq, D, H, W);
 * train_label (n_train, n_seq, T, H, W); train_ltrb (n_train, n_seq, T, 4, H, W); pos (H*W, D) from pt_tomp_posenc_f32;
 * filters (B, T, D); enc_feat (B, D, H, W).
 *   parallel = 0: predict_filter.   parallel = 1 (n_seq must be 1): row 0 classification, row 1 box regression with the keys
 *   [num_gth_frames H W, L - H W) masked in encoder and decoder (filter_predictor.py:298-299).
 *
 * The call computes
 *   memory tokens  feat + sum_o label[o] E[o] + sum_o E[o] (.) MLP(ltrb[o])   (filter_predictor.py:204-220); E = query_embed_fg.weight,
 *                  MLP = 4 -> D/4 -> D -> D with eval-mode BatchNorm1d and ReLU (:6-17).  An absent object (zero label, zero box) still
 *                  contributes E[o] (.) MLP(0).  The object sum in front of the last Linear is one product with K = T D against
 *                  diag(E[o]) W3, a weight-only matrix that pt_tamos_prepare_f32 folds; test tokens are the features as they are (:222)
 *   encoder        pt_tomp's stack and launchers (transformer.py:172-180)
 *   decoder        T queries per batch row, post-norm (transformer.py:224-238): self-attention among the T queries, cross-attention of
 *                  the T nhead query rows over all L keys with pt_tomp's fold (W_k,h^T W_q,h / sqrt(d_h) and W_o[:,h] W_v,h, folded by
 *                  pt_tamos_prepare_f32) -- the keys stream in 64-key chunks whose (max, sum, context) are merged in chunk order, so
 *                  nothing of size L is held on chip and L has no limit of its own --, FFN, three LayerNorms, then decoder.norm (:140-141)
 * fp32 products and accumulation, no atomics (the same inputs give the same bits), no host synchronisation (graph-capturable).
 *
 * Covered: pt_tomp's dims (d_model in {128,256,384,512}, head width in {16,32,64}, dim_ff % 64 == 0, <= 16 layers each), B <= 8,
 * 1 <= T <= 16, any L whose buffers stay under 4 GiB (32-bit byte offsets).  Otherwise pt_tamos_param_floats / _ws_bytes return 0 and
 * the entry points PT_ERR_UNSUPPORTED / PT_ERR_SHAPE before any launch.
 *
 * pt_tamos_predict_routes: host only, like pt_tomp_predict_routes; the shared launchers report their PT_TOMP_R_* ids, the launches that
 * are new here -- k_tamos_tokens, k_tamos_box1, k_tamos_self_attn, k_tamos_xattn<D / 16>, k_tamos_xmerge -- ids of enum pt_tamos_route.
 * It refuses exactly where pt_tamos_predict_f32 does; PT_TAMOS_MAX_ROUTES entries always suffice.
 * ---------------------------------------------------------------------------------------------- */
enum pt_tamos_route {
    PT_TAMOS_R_TOKENS = 1000, PT_TAMOS_R_BOX1, PT_TAMOS_R_SELF_ATTN,
    PT_TAMOS_R_XATTN128, PT_TAMOS_R_XATTN256, PT_TAMOS_R_XATTN384, PT_TAMOS_R_XATTN512, PT_TAMOS_R_XMERGE,
    PT_TAMOS_R_END
};
#define PT_TAMOS_MAX_ROUTES 512
size_t pt_tamos_param_floats(const pt_tomp_dims* dims, int num_tokens);
size_t pt_tamos_prepared_floats(const pt_tomp_dims* dims, int num_tokens);
int pt_tamos_prepare_f32(const pt_tomp_dims* dims, int num_tokens, const float* params, float* prepared, void* stream);
size_t pt_tamos_predict_ws_bytes(const pt_tomp_dims* dims, int num_tokens, int n_train, int n_seq, int parallel);
int pt_tamos_predict_f32(const pt_tomp_dims* dims, int num_tokens, const float* params, const float* prepared, const float* pos,
                         const float* train_feat, const float* test_feat, const float* train_label, const float* train_ltrb,
                         int n_train, int n_seq, int parallel, int num_gth_frames, float* filters, float* enc_feat,
                         void* ws, size_t ws_bytes, void* stream);
int pt_tamos_predict_routes(const pt_tomp_dims* dims, int num_tokens, int n_train, int n_seq, int parallel, int* routes, int cap,
                            int* n_routes);

/* ------------------------------------------------------------------------------------------------
 * TaMOs heads -- replace, for inference, what pytracking/tracker/tamos/tamos.py:308-317 runs behind the filter predictor:
 *   FPN.forward with two levels                     (ltr/models/transformer/heads.py:144-162, torchvision FeaturePyramidNetwork)
 *   DenseBoxRegressor.forward with T filters / seq  (ltr/models/transformer/heads.py:119-141, the `attention.dim() == 5` branch)
 * Both stand on one kernel, k_conv3: a direct 3x3 token convolution (stride 1, padding 1, fp32 MFMA) in which one workgroup owns a
 * 128 x 64 output tile of one image and walks K = 9 Cin itself -- no per-tap partial buffer, no atomics, the same bits every call.
 *
 * pt_tamos_bbreg_f32: feat (n_img, D, H, W) NCHW; filters (n_img, T, D), the unprojected filters of each image's sequence;
 * ltrb (n_img, T, 4, H, W); params = the pack of pt_tomp_bbreg_f32 (pt_tomp_bbreg_param_floats), one pack serves both.  Computes
 *   filter_proj = linear(filters); attention[o] = feat . filter_proj[o]; tower(attention[o] (.) feat) over n_img T images;
 *   exp(bbreg_layer(.)).  The attended copies are never written: the first layer's loader multiplies by the per-pixel scalar.  Every
 *   tower layer leaves per-tile (sum, sum of squares) of its output (bias included); they are summed per image in slot order in double and
 *   the next layer's loader applies GroupNorm(1, D) + affine + ReLU, zero padding after the transform.
 * pt_fpn2_f32: feat_hi (n, C_hi, H2, W2), feat_lo (n, C_lo, H3, W3) -> feat2 (n, D, H2, W2) and, if want_feat3, feat3 (n, D, H3, W3)
 *   (feat3 may be NULL and is left untouched otherwise).  pack (pt_fpn2_param_floats): inner_blocks.0 weight (D, C_hi), bias (D);
 *   inner_blocks.1 weight (D, C_lo), bias (D); layer_blocks.0 weight (D, ky, kx, D), bias (D); layer_blocks.1 weight (D, ky, kx, D),
 *   bias (D).  feat3 = layer1(lat_lo); feat2 = layer0(lat_hi + nearest(lat_lo -> (H2, W2))) with the source index
 *   min(floor(dst * (float)in / out), in - 1) of F.interpolate(mode="nearest", size=...), added in the 3x3 loader.
 * Covered: D (and d_model) a multiple of 64 up to 512, C_hi / C_lo multiples of 64 up to 2048, 1 <= T <= 16, any H, W >= 1, every
 * buffer under 4 GiB (32-bit byte offsets), at most 65535 images.  Otherwise the *_ws_bytes queries return 0 and the entry points
 * PT_ERR_SHAPE / PT_ERR_UNSUPPORTED before any launch.  Asynchronous on `stream`, no host synchronisation, graph-capturable.
 * pt_tamos_bbreg_routes / pt_fpn2_routes: host only, like pt_tomp_bbreg_routes: the shared launchers report their
 * PT_TOMP_R_* ids, the new launches ids of enum pt_heads_route below (from 2000: no existing id moves) --
 * k_nchw_to_tokens, k_conv3<plain | per-row scalar | GroupNorm loader | top-down resize + add>, k_conv3_gn_finish, k_reg_out.
 * ---------------------------------------------------------------------------------------------- */
enum pt_heads_route {
    PT_HEADS_R_NCHW_TOKENS = 2000, PT_HEADS_R_CONV3_PLAIN, PT_HEADS_R_CONV3_ROWSCALE, PT_HEADS_R_CONV3_GN, PT_HEADS_R_CONV3_UPADD,
    PT_HEADS_R_CONV3_GN_FINISH, PT_HEADS_R_REG_OUT,
    PT_HEADS_R_END
};
size_t pt_tamos_bbreg_ws_bytes(int n_img, int T, int d_model, int H, int W);
int pt_tamos_bbreg_f32(const float* params, const float* feat, const float* filters, float* ltrb, int n_img, int T, int d_model,
                       int H, int W, void* ws, size_t ws_bytes, void* stream);
int pt_tamos_bbreg_routes(int n_img, int T, int d_model, int H, int W, int* routes, int cap, int* n_routes);
size_t pt_fpn2_param_floats(int C_hi, int C_lo, int d_out);
size_t pt_fpn2_ws_bytes(int n, int C_hi, int C_lo, int d_out, int H2, int W2, int H3, int W3);
int pt_fpn2_f32(const float* params, const float* feat_hi, const float* feat_lo, float* feat2, float* feat3, int n, int C_hi,
                int C_lo, int d_out, int H2, int W2, int H3, int W3, int want_feat3, void* ws, size_t ws_bytes, void* stream);
int pt_fpn2_routes(int n, int C_hi, int C_lo, int d_out, int H2, int W2, int H3, int W3, int want_feat3, int* routes, int cap,
                   int* n_routes);

/* ------------------------------------------------------------------------------------------------
 * Classification-feature head -- `residual_bottleneck(num_blocks=0, final_conv=True, l2norm=True)`
 * (ltr/models/target_classifier/features.py:49-73): Conv2d(Cin, Cout, 3, padding=1, bias=False) followed by
 * InstanceL2Norm(size_average=True, eps, scale) (ltr/models/layers/normalization.py:15-20), as DiMP-50 (1024 -> 512,
 * dimpnet.py:169-172) and ToMP (1024 -> 256, tompnet.py:99-102; run on three frames per tracked frame) build it.
 *   feat (n, Cin, H, W); weight_tap_major (Cout, ky, kx, Cin) = the reference's (Cout, Cin, 3, 3) tensor permuted
 *   (0,2,3,1); out (n, Cout, H, W) = conv * norm_scale * sqrt(Cout*H*W / (sum over the image of conv^2 + eps)).
 * Covered: Cin % 64 == 0, Cout % 4 == 0.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_clf_head_ws_bytes(int n, int Cin, int Cout, int H, int W);
int pt_clf_head_f32(const float* feat, const float* weight_tap_major, float* out, int n, int Cin, int Cout, int H, int W,
                    float norm_scale, float eps, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature head at stride 1 or 2 -- the heads in front of the LWL / RTS learners:
 *   `residual_basic_block(num_blocks=0, final_conv=True, l2norm=True)` (features.py:9-28), the target-model head of LWL and RTS
 *     (lwl_net.py:173-177, rts_net.py:294-298): Conv2d(1024, 512, 3, padding=1, bias=False) + InstanceL2Norm on a 30 x 52 map, stride 1;
 *   `residual_bottleneck(num_blocks=0, final_conv=True, l2norm=True, final_stride=2)` (features.py:49-73), the RTS classifier head
 *     (rts_net.py:339-344): the same convolution at stride 2, 1024 x 30 x 52 -> 512 x 15 x 26.
 *   feat (n, Cin, H, W); weight_tap_major (Cout, ky, kx, Cin) as for pt_clf_head_f32; out (n, Cout, Ho, Wo) with Ho = (H-1)/stride + 1,
 *   Wo = (W-1)/stride + 1, = y * norm_scale * sqrt(Cout*Ho*Wo / (sum over the image of y^2 + eps)), y the zero-padded 3x3 convolution
 *   at that stride (padding 1: output (oy, ox), tap (ky, kx) reads input (stride*oy + ky - 1, stride*ox + kx - 1)).
 * stride == 1 IS pt_clf_head_f32 (same kernels, same workspace size, same bits).  stride == 2: one partial product per tap on the exact
 * fp32 MFMA, the nine summed in fixed order.  Any other stride: PT_ERR_UNSUPPORTED, ws_bytes 0.
 * Covered: Cin % 64 == 0, Cout % 4 == 0.  Every check precedes the first launch; asynchronous on `stream`, the caller owns the
 * workspace; no atomics, fixed summation order: repeated calls give the same bits and the call can be captured in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_feat_head_ws_bytes(int n, int Cin, int Cout, int H, int W, int stride);
int pt_feat_head_f32(const float* feat, const float* weight_tap_major, float* out, int n, int Cin, int Cout, int H, int W, int stride,
                     float norm_scale, float eps, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Target localisation on the device -- the score-map arithmetic of DiMP/ToMP `localize_advanced`
 * (pytracking/tracker/dimp/dimp.py:238-303, pytracking/tracker/tomp/tomp.py) and `dcf.max2d`
 * (pytracking/libs/dcf.py:156-164), one launch, results left on the device for a single copy.
 *   pt_max2d_f32: a (n, H, W) -> max_val (n), argmax (n, 2) int64 [row, col]; ties: smallest column, then smallest row
 *     (the order torch.max over rows, then over columns produces).
 *   pt_localize_f32: scores (S, H, W) [S <= 8 scales], scores_hn (S, H, W) or NULL (= scores): the map the second
 *     peak is searched in (`perform_hn_without_windowing`, dimp.py:247-250); neigh_rows / neigh_cols: HOST arrays of S
 *     floats = target_neigh_sz of each scale in score cells (dimp.py:268).
 *     out8 (device) = [max1, row1, col1, scale_ind, max2, row2, col2, 0]: first peak over all scales (first scale on
 *     ties), second peak of scores_hn[scale_ind] with rows [round(row1 - nr/2), round(row1 + nr/2 + 1)) x the same in
 *     columns, clamped to the map, ZEROED (dimp.py:270-278; Python round() = half-to-even).
 * ---------------------------------------------------------------------------------------------- */
int pt_max2d_f32(const float* a, float* max_val, long long* argmax, int n, int H, int W, void* stream);
int pt_localize_f32(const float* scores, const float* scores_hn, const float* neigh_rows, const float* neigh_cols,
                    float* out8, int S, int H, int W, void* stream);

/* pt_localize_decide_f32: the whole of `localize_advanced` in one launch -- both peaks
 * as pt_localize_f32 finds them, then the outcome of dimp.py:258-303 decided on the device.  The caller supplies the
 * per-frame constants below (plain host arithmetic on the tracker's state; no device data is needed to form them):
 *   thresholds on the first peak are compared as doubles (`max_score1.item() < threshold`), the remaining tests are the
 *   reference's float32 tensor expressions (`python float * float32 tensor`, `float32 tensor > python float`);
 *   center = (score_sz - 1) / 2, ratio = img_support_sz / output_sz (dimp.py:241-244), per scale s: scale[s] =
 *   sample_scales[s], neigh = target_neigh_sz (dimp.py:268), prev = prev_target_vec (dimp.py:285), disp_threshold =
 *   dispalcement_scale * sqrt(H * W) / 2 (dimp.py:291).  Absent optional thresholds are passed as -infinity.
 * out16 (device memory OR device-visible pinned host memory; the kernel writes it directly) =
 *   [code, scale_ind, row, col, translation_row, translation_col, max1, row1, col1, max2, row2, col2, peak_chosen, 0, 0, seq]
 *   with code = PT_LOC_*, (row, col) the displacement (`max_disp`) of the chosen peak and translation =
 *   (disp - center) * ratio * scale[scale_ind] in float32 (dimp.py:256,282). */
enum { PT_LOC_NORMAL = 0, PT_LOC_HARD_NEGATIVE = 1, PT_LOC_UNCERTAIN = 2, PT_LOC_NOT_FOUND = 3 };
typedef struct {
    double target_not_found_threshold, uncertain_threshold, hard_sample_threshold;
    float distractor_threshold, hard_negative_threshold, target_not_found_f32, disp_threshold;
    float center_r, center_c, ratio_r, ratio_c;
    float scale[8], neigh_r[8], neigh_c[8], prev_r[8], prev_c[8];
} pt_localize_params;
int pt_localize_decide_f32(const float* scores, const float* scores_hn, const pt_localize_params* prm, float* out16,
                           int S, int H, int W, void* stream);

/* The tracker's host state `localize_advanced` reads (all HOST values): `params.*` thresholds as the Python floats they
 * are (absent optional ones: -infinity), the float32 contents of `kernel_size`, `img_support_sz`, `target_sz`, `pos`
 * ([row, col]) and per scale `sample_scales[s]`, `sample_pos[s] = (row, col)`.
 *   pt_localize_constants_f32: pt_localize_params from that state, in the reference's float32 operation order (host
 *     only: no launch, no device access).
 *   pt_localize_advanced_f32 = constants + pt_localize_decide_f32: one call per frame. */
typedef struct {
    double target_not_found_threshold, uncertain_threshold, hard_sample_threshold, distractor_threshold,
        hard_negative_threshold, target_neighborhood_scale, dispalcement_scale;
    float kernel_size[2], img_support_sz[2], target_sz[2], pos[2];
    float sample_scales[8], sample_pos[16];
} pt_localize_state;
int pt_localize_constants_f32(const pt_localize_state* st, int S, int H, int W, pt_localize_params* prm);
int pt_localize_advanced_f32(const float* scores, const float* scores_hn, const pt_localize_state* st, float* out16,
                             int S, int H, int W, void* stream);
/* pt_localize_advanced_sync_f32: the same, returning when the results are readable by the host.  out16_host MUST be
 * pinned host memory the device can write (hipHostMalloc, torch `pin_memory()`); anything else -> unsupported.  The
 * kernel stores a per-call sequence number into out16_host[15] last and the host polls that word (no runtime
 * synchronisation call on the frame's critical path); only work queued on `stream` BEFORE this launch is waited for. */
int pt_localize_advanced_sync_f32(const float* scores, const float* scores_hn, const pt_localize_state* st,
                                  float* out16_host, int S, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * IoU-guided box refinement -- DiMP.optimize_boxes_default / optimize_boxes_relative
 * (pytracking/tracker/dimp/dimp.py:725-788) on AtomIoUNet.predict_iou (ltr/models/bbreg/atom_iou_net.py:96-136):
 * gradient ascent on the predicted IoU w.r.t. the P proposal boxes, all iterations on the device.
 *   params pack (fp32, the reference's state_dict tensors below `bb_regressor.`, this order): fc3_rt.linear.weight
 *     (I3, C3*25), fc3_rt.linear.bias, fc3_rt.bn.{weight, bias, running_mean, running_var}, fc4_rt.linear.weight
 *     (I4, C4*9), fc4_rt.linear.bias, fc4_rt.bn.{...}, iou_predictor.weight (I3+I4), iou_predictor.bias (1).
 *   prepared: the two Linear weights transposed, written by pt_iou_prepare_f32 once per weight update.
 *   c3 (C3,H3,W3), c4 (C4,H4,W4): IoU features of ONE test image (get_iou_feat); mod3 (C3), mod4 (C4): modulation
 *   vectors (get_modulation); init_boxes / boxes_out (P,4) xywh in image coordinates; iou_out (P) = the prediction of the
 *   last forward pass, as the reference returns it.  step_length4: HOST [s,s,s,s] or [s0,s0,s1,s1] (dimp.py:737-738);
 *   relative = 1: optimise [cx/sw, cy/sh, log w, log h] with [sw, sh] = size of the first box (dimp.py:767-768).
 *   backtrack = 0: DiMP -- one step length for all proposals, multiplied by step_decay after every iteration;
 *   backtrack = 1: ATOM.optimize_boxes (pytracking/tracker/atom/atom.py:758-836) -- a proposal whose predicted IoU did
 *     not improve multiplies ITS step length by step_decay and takes its previous step back (no-op when step_decay >= 1).
 *   Pools are the reference's: 5x5 at 1/8 on c3, 3x3 at 1/16 on c4.  Covered: C3*25, C4*9, I3, I4 multiples of 32, P <= 256.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pt_iou_dims { int C3, C4, I3, I4, H3, W3, H4, W4; } pt_iou_dims;
size_t pt_iou_param_floats(const pt_iou_dims* dims);
size_t pt_iou_prepared_floats(const pt_iou_dims* dims);
int pt_iou_prepare_f32(const pt_iou_dims* dims, const float* params, float* prepared, void* stream);
size_t pt_iou_refine_ws_bytes(const pt_iou_dims* dims, int P);
int pt_iou_refine_f32(const pt_iou_dims* dims, const float* params, const float* prepared, const float* c3, const float* c4,
                      const float* mod3, const float* mod4, const float* init_boxes, float* boxes_out, float* iou_out,
                      int P, int num_iter, const float* step_length4, float step_decay, int relative, int backtrack,
                      void* ws, size_t ws_bytes, void* stream);

/* The same for the per-frame call of the trackers (proposals formed on the host, refined boxes needed on the host:
 * dimp.py:691-722, atom.py:724-756): init_boxes_host = P <= 16 boxes (xywh) in HOST memory, passed inside a kernel argument
 * block; out_host = PT_IOU_HOST_FLOATS floats of pinned host memory: boxes [0, 4P), IoU [64, 64+P), sequence word [95].
 * Returns when the results are readable (polls the sequence word; no hipStreamSynchronize).  PT_ERR_UNSUPPORTED for
 * P > 16 or out_host not device-writable host memory: use pt_iou_refine_f32. */
#define PT_IOU_HOST_FLOATS 96
int pt_iou_refine_sync_f32(const pt_iou_dims* dims, const float* params, const float* prepared, const float* c3, const float* c4,
                           const float* mod3, const float* mod4, const float* init_boxes_host, float* out_host, int P,
                           int num_iter, const float* step_length4, float step_decay, int relative, int backtrack, void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Precise RoI Pooling -- replaces ltr/external/PreciseRoIPooling (empty git submodule;
 * import sites ltr/models/target_classifier/initializer.py:4,18,45 and
 * ltr/models/bbreg/atom_iou_net.py:4,31-32,41-42,126-127,157,160).
 *   features (N,C,H,W); rois (R,5) = [batch_idx, x0, y0, x1, y1]; out / grad_out (R,C,PH,PW).
 *   bwd_feat ACCUMULATES into grad_features (caller zeroes it); bwd_coor writes grad_rois (R,5),
 *   column 0 = 0.
 * ---------------------------------------------------------------------------------------------- */
int pt_prroi_fwd_f32(const float* features, const float* rois, float* out,
                     int N, int C, int H, int W, int R, int PH, int PW, float spatial_scale, void* stream);
int pt_prroi_bwd_feat_f32(const float* grad_out, const float* rois, float* grad_features,
                          int N, int C, int H, int W, int R, int PH, int PW, float spatial_scale, void* stream);
int pt_prroi_bwd_coor_f32(const float* grad_out, const float* features, const float* rois, float* grad_rois,
                          int N, int C, int H, int W, int R, int PH, int PW, float spatial_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One synthetic tracking frame of the benchmark workload (BASELINE.json metric):
 *   classify(test_feat) -> on-device arg-max -> overwrite memory slot `slot` (features + box centred on
 *   the peak) -> steepest-descent solve over the n memory samples, all on `stream`, no host sync.
 * mem_feat (n,C,H,W), mem_bb (n,4), sample_weight (n), filter (C,K,K) in/out, scores_out (OH*OW),
 * peak_out (2 floats: row, col).
 * ---------------------------------------------------------------------------------------------- */
size_t pt_track_frame_ws_bytes(int n, int C, int H, int W, int K);
int pt_track_frame_f32(const pt_sd_params* p, float* filter, float* mem_feat, float* mem_bb,
                       const float* sample_weight, const float* test_feat, int slot,
                       int n, int C, int H, int W, int K, int num_iter,
                       float* scores_out, float* peak_out, void* ws, size_t ws_bytes, void* stream);

/* Frame CHAINS (round 6).  pt_track_frame_f32 leaves the last iterate in `filter` before its launches end: the solve's last
 * statement, w_T = w_{T-1} - step*alpha_T*g_T (optimizer.py:155-160), is one dependent launch whose ONLY consumer is the next
 * frame's first correlation (classification + s_0).  In a chain of frames on one stream and one workspace that launch can ride on
 * its consumer: with defer != 0 the call leaves (w_{T-1}, g_T, the operands of alpha_T) in the workspace and describes them in
 * *pending; the next pt_track_frame_chain_f32 call (same filter / workspace / n, C, H, W, K) finds pending->iters > 0, forms w_T in
 * the prologue of its first correlation -- the same expressions on the same operands: the same bits as pt_track_frame_f32 -- and
 * stores it to `filter`; pt_track_frame_flush_f32 applies a pending update on its own (end of the chain, or before anything else
 * reads `filter`).  While an update is pending `filter` holds w_0 of the last solve, NOT its result.
 *   *pending: caller-owned host struct, zero-initialised at the start of a chain; in-out.  A solve of fewer than 2 iterations is
 *   never deferred (pending->iters stays 0).  4x4 filters on the XCD-aligned path only: PT_ERR_UNSUPPORTED otherwise with nothing
 *   queued -- fall back to pt_track_frame_f32 (after a flush). */
typedef struct {
    int iters;            /* 0: nothing pending; else the iteration count T of the solve whose last update is pending */
    float step_length;    /* of that solve */
    float reg_eps;        /* its reg + alpha_eps */
} pt_frame_pending;
int pt_track_frame_chain_f32(const pt_sd_params* p, float* filter, float* mem_feat, float* mem_bb,
                             const float* sample_weight, const float* test_feat, int slot,
                             int n, int C, int H, int W, int K, int num_iter,
                             float* scores_out, float* peak_out, void* ws, size_t ws_bytes,
                             pt_frame_pending* pending, int defer, void* stream);
int pt_track_frame_flush_f32(pt_frame_pending* pending, float* filter, int n, int C, int H, int W, int K,
                             void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The tracking frame with the classification-feature head in front.
 * Replaces: ltr/models/target_classifier/features.py:66-72 (final 3x3 conv + InstanceL2Norm of the test frame) feeding
 * pytracking/tracker/dimp/dimp.py:190-194, 429-441, 605-648 (classify, memory insert, re-optimisation) in one call: the
 * head writes the normalised (C,H,W) feature straight into memory slot `slot`, which the first correlation of the solve
 * then reads like any other sample -- the test feature never exists as a separate tensor.
 *   backbone_feat (Cin,H,W); head_weight_tap_major (C,3,3,Cin) as for pt_clf_head_f32; everything else as pt_track_frame_f32.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_track_frame_head_ws_bytes(int n, int Cin, int C, int H, int W, int K);
int pt_track_frame_head_f32(const pt_sd_params* prm, float* filter, float* mem_feat, float* mem_bb,
                            const float* sample_weight, const float* backbone_feat, const float* head_weight_tap_major,
                            float norm_scale, float norm_eps, int slot, int n, int Cin, int C, int H, int W, int K,
                            int num_iter, float* scores_out, float* peak_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The WHOLE DiMP frame behind the backbone as one call (SURVEY.md section 8f items 1-3 joined to the frame above):
 *   head -> classify + memory insert + re-optimisation (pt_track_frame_head_f32) -> localize_advanced on the score map
 *   -> the tracker's glue between localisation and refinement ON THE DEVICE -> IoU-guided refinement of the proposals,
 * with ONE host wait at the end.  Replaces the call sequence of `DiMP.track` (pytracking/tracker/dimp/dimp.py:95-131):
 *   get_classification_features (:312-314), classify_target (:190-194), localize_target -> localize_advanced (:196-303),
 *   `new_pos = sample_pos[scale_ind] + translation_vec` (:118), update_state (:486-495), refine_target_box (:650-678:
 *   get_iounet_box :498-504, the jittered proposals :663-675), optimize_boxes_default / _relative (:725-788),
 * whose two host round trips (the localisation result, the refined boxes) and the Python between them are the frame's
 * critical path once the kernels are fast.  The proposals depend on the localisation result, so that dependency moves to
 * the device (`k_frame_glue`): the same float32 operations in the reference's order; the frame's random numbers
 * (`torch.rand(num_init_random_boxes, 4)`, :671) are drawn by the HOST generator as the reference does and passed in.
 * When the localisation says `not_found` the reference skips the refinement (:121): here it still runs and the caller
 * ignores boxes / IoU (the flag is in the result block).  S = 1 scale (the trackers' configuration).
 *
 * out_host: PT_FRAME_HOST_FLOATS floats of pinned host memory (device-writable):
 *   [0,16)   the 16 localisation results of pt_localize_advanced_f32
 *   [16,18)  self.pos after update_state (row, col);  [18,22) init_box (x, y, w, h) of get_iounet_box
 *   [32,32+4P) refined boxes, [96,96+P) predicted IoU, [127] sequence word the call polls.   P = 1 + num_random <= 16.
 * ---------------------------------------------------------------------------------------------- */
#define PT_FRAME_HOST_FLOATS 128
typedef struct pt_frame_glue {
    float image_sz[2];                 /* self.image_sz (rows, cols) */
    float img_sample_sz[2];            /* self.img_sample_sz */
    double target_inside_ratio;        /* params.target_inside_ratio (default 0.2) */
    double box_jitter_pos, box_jitter_sz;   /* params.box_jitter_pos / box_jitter_sz */
    int use_classifier;                /* params.use_classifier (default 1): update_state(new_pos) before the refinement */
    int num_random;                    /* params.num_init_random_boxes, 0 .. 15 */
    float rand_u[60];                  /* torch.rand(num_random, 4) of this frame, row-major */
} pt_frame_glue;
typedef struct pt_frame_full {
    /* head + solver: exactly the arguments of pt_track_frame_head_f32 */
    const pt_sd_params* sd;
    float *filter, *mem_feat, *mem_bb;
    const float *sample_weight, *backbone_feat, *head_weight_tap_major;
    float norm_scale, norm_eps;
    int slot, n, Cin, C, H, W, K, num_iter;
    float *scores_out, *peak_out;
    /* localisation + glue */
    const pt_localize_state* loc;
    const pt_frame_glue* glue;
    /* refinement: exactly the arguments of pt_iou_refine_f32 (boxes come from the glue) */
    const pt_iou_dims* iou_dims;
    const float *iou_params, *iou_prepared, *c3, *c4, *mod3, *mod4;
    int iou_iter, relative;
    float step_length4[4];
    float step_decay;
    /* optional second HIP stream.  The localisation + glue + refinement chain needs only the classification scores, which exist
     * after the frame's first correlation; with aux_stream != NULL that chain forks there (event) and runs on aux_stream CONCURRENTLY
     * with the steepest-descent iterations on `stream`, and `stream` joins it before the call's launches end (so everything queued on
     * `stream` afterwards is ordered behind both chains).  Valid because in this synthetic frame the new
     * sample's label box comes from the classification peak; `DiMP.track` labels the update with the REFINED state (dimp.py:139-145),
     * which makes its update depend on the refinement: leave aux_stream NULL for that order.  On return the result block is
     * host-visible; the filter / memory are complete in `stream` order, not necessarily yet: the call returns when the refinement
     * chain has written the sequence word, the steepest-descent tail on `stream` may still be running, so reading filter / mem_bb /
     * scores from the host or from another stream right after the return needs a wait on `stream` first.
     * Because the update is REORDERED relative to dimp.py:139-145, a call with aux_stream set AND num_iter > 0 is refused
     * (PT_ERR_UNSUPPORTED, nothing queued) unless aux_reordered_update_ok is non-zero. */
    void* aux_stream;
    int aux_reordered_update_ok;
    /* Graph replay (round 6).  A captured frame freezes every kernel ARGUMENT; with dyn != NULL (device memory, 16-byte aligned,
     * pt_track_frame_full_dyn_bytes() bytes) the per-frame VALUES -- the memory slot, the tracker state of the localisation and of the
     * glue (pos, target_sz, sample position / scale, thresholds), this frame's random numbers, the sequence number -- are read by the
     * kernels from that block instead, and the captured launches depend on pointers and shapes only.  Per frame the host writes the
     * block with pt_track_frame_full_dyn_fill_f32 into pinned memory, a copy node at the head of the graph moves it to `dyn`, the graph
     * is replayed and pt_host_wait_word_f32(out + 127, seq) waits for the result block.  Pointers (backbone_feat, c3, c4, mod3 / mod4,
     * scores_out, the result block, the workspace) are those of the capture: the caller's backbone writes into fixed buffers.  One
     * stream only (aux_stream must be NULL); num_iter / iou_iter / the proposal count are properties of the captured graph. */
    void* dyn;
} pt_frame_full;
size_t pt_track_frame_full_ws_bytes(const pt_frame_full* f);
int pt_track_frame_full_f32(const pt_frame_full* f, float* out_host, void* ws, size_t ws_bytes, void* stream);
/* the launches without the wait (graph capture, or a caller that waits on the stream itself) */
int pt_track_frame_full_launch_f32(const pt_frame_full* f, float* out, void* ws, size_t ws_bytes, void* stream);
/* graph replay: size of the per-frame block, and its host-side fill for the frame described by *f (slot, loc, glue; seq != 0) --
 * `out` / `ws` as captured; `dyn_host`: pinned host memory the graph's copy node reads.  Nothing is queued. */
size_t pt_track_frame_full_dyn_bytes(void);
int pt_track_frame_full_dyn_fill_f32(const pt_frame_full* f, float seq, float* out, void* ws, size_t ws_bytes, void* dyn_host);
/* wait until *word == seq (a result block's sequence word in pinned host memory; polled, falls back to hipStreamSynchronize after 2 s) */
int pt_host_wait_word_f32(const float* word, float seq, void* stream);

/* Measurement helper (bench.py): `reps` back-to-back launches of a kernel that only READS `floats` floats of `mem` (16-byte aligned)
 * with every CU -- the streaming floor of one feature pass over that footprint.  scratch2048: 2048 floats of device memory. */
int pt_stream_probe_f32(const float* mem, size_t floats, float* scratch2048, int reps, void* stream);

/* Result buffers of the *_sync_* / full-frame entry points are verified once (pinned, device-writable) and remembered;
 * call this before freeing such a buffer so that a later allocation at the same address is verified again. */
void pt_host_buffer_forget(const void* p);

/* ------------------------------------------------------------------------------------------------
 * Image-patch sampling in front of the backbone.
 * Replaces: pytracking/features/preprocessing.py:54-148 `sample_patch` (strided pre-downsampling, crop with replicate
 * padding, F.interpolate(mode='bilinear')) and :33-51 `sample_patch_multiscale` (S scales in one launch).
 *   im   (C, H, W) float image on the device;   out (S, C, OH, OW)
 *   geom one record per scale, the integers the reference computes on the host (preprocessing.py:83-128):
 *        df = pre-downsampling stride, (os0, os1) = its row / column offset, (tl0, tl1) = top-left corner of the crop in
 *        the down-sampled image (may be negative / beyond the border: replicate padding), crop_h x crop_w = crop size.
 * ---------------------------------------------------------------------------------------------- */
#define PT_PATCH_MAX_SCALES 8
typedef struct pt_patch_geom { int df, os0, os1, tl0, tl1, crop_h, crop_w; } pt_patch_geom;
int pt_sample_patch_f32(const float* im, int C, int H, int W, const pt_patch_geom* geom, int S, float* out, int OH, int OW,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * First-frame augmentation set (second half).
 * Replaces: pytracking/features/preprocessing.py:13-30 `sample_patch_transformed` -- the loop `T(im_patch)` over the
 * transforms of pytracking/features/augmentation.py (Identity :39, FlipHorizontal :44, FlipVertical :52, Translation :60,
 * Scale :73, Rotate :111, Blur :128) followed by `Transform.crop_to_output` (:20-37) -- as built by
 * pytracking/tracker/dimp/dimp.py:329-395 `generate_init_samples` (same in atom.py / tomp.py / kys.py).
 *   patch  (C, EH, EW) base patch on the device (the output of pt_sample_patch_f32 at the augmentation size)
 *   desc   T records on the HOST, one per transform (they travel in the kernel arguments):
 *          kind      PT_AUG_*                         (Translation is PT_AUG_IDENTITY with its shift in the pads)
 *          pad_top / pad_left = floor((OH - th) / 2) + shift[0], floor((OW - tw) / 2) + shift[1]   (augmentation.py:30-33)
 *          th, tw    size of the transformed image before the crop (EH, EW except for PT_AUG_SCALE: :84-87)
 *          fs0, fs1, tap_off0, tap_off1   PT_AUG_BLUR: half filter sizes ceil(2 sigma) and the offsets of the 2 fs + 1
 *                    normalised taps of each axis in `taps` (host, n_taps floats)                                     (:135-140)
 *          m[6]      PT_AUG_ROTATE: the 2x3 matrix that maps OUTPUT to INPUT pixels (the inverse of the matrix the
 *                    reference hands to cv.warpAffine, :121-126); parity of this kind is UNPINNED (no cv2 in the image)
 *   out    (T, C, OH, OW)
 * ---------------------------------------------------------------------------------------------- */
enum { PT_AUG_IDENTITY = 0, PT_AUG_FLIP_H = 1, PT_AUG_FLIP_V = 2, PT_AUG_BLUR = 3, PT_AUG_SCALE = 4, PT_AUG_ROTATE = 5 };
typedef struct pt_aug_desc {
    int kind, pad_top, pad_left, th, tw, fs0, fs1, tap_off0, tap_off1, reserved;
    double m[6];
} pt_aug_desc;
#define PT_AUG_MAX_TRANSFORMS 24   /* per launch; longer lists are split by the library */
#define PT_AUG_MAX_TAPS 256
int pt_augment_patches_f32(const float* patch, int C, int EH, int EW, const pt_aug_desc* desc, int T, const float* taps,
                           int n_taps, float* out, int OH, int OW, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement entry (bench.py roofline leg; not part of the reference's API).  Re-issues ONE feature pass of the
 * solve that pt_track_frame_f32 last ran on `ws` -- the launch of its last iteration, same kernel instantiation and
 * operands -- `reps` times back to back on `stream`, so that the caller can bracket the run with ONE HIP event pair
 * (elapsed / reps = kernel duration + one dependent-launch boundary).  Both passes only read the state they were
 * launched on, so the replay leaves the sequence's state untouched.  Needs num_iter >= 2 and the XCD-aligned path.
 *   which = 0: correlation pass with the fused gradient reduction;  which = 1: adjoint pass with the fused update.
 * ---------------------------------------------------------------------------------------------- */
int pt_track_frame_replay_pass_f32(const pt_sd_params* prm, const float* filter, const float* mem_feat,
                                   const float* mem_bb, const float* sample_weight, int n, int C, int H, int W, int K,
                                   int num_iter, void* ws, size_t ws_bytes, int which, int reps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Target-candidate matching (KeepTrack; pytracking/tracker/keep_track/keep_track.py:437-475), tcm.hip.
 *
 * pt_tcm_peaks_f32: local maxima of B score maps (ltr/data/processing_utils.py:669-705).
 *   scores (B, H, W), H, W <= 64; ks odd (max_pool2d window, stride 1, padding ks/2: padding never wins);
 *   a peak is scores == window max && scores > th.  Per map b: count[b] (int32) peaks, sorted by value, highest first,
 *   ties in ascending raster order (the reference's argsort leaves the order of ties unspecified); coords (B, H*W, 2) int64
 *   (y, x) and values (B, H*W): the first count[b] entries of map b are written.  Exact float comparisons: bit-identical to
 *   the reference for the same map.
 *
 * pt_tcm_desc_f32: DescriptorExtractor.get_descriptors (target_candidate_matching.py:28-36) at P points per image only:
 *   out[b, d, p] = bias[d] + sum_{c,u,v} weight[d, c, u, v] * x[b, c, y_p + u - 2, x_p + v - 2]
 *   x (B, C, H, W), weight (D, C, 4, 4) contiguous (16-byte aligned), bias (D), coords (B, P, 2) int64 (y, x) on the
 *   (H+1) x (W+1) output map (a point outside it reads zeros only), out (B, D, P).  C % 16 == 0, D % 64 == 0.  K = 16 C is
 *   split over C/16 workgroups per 64 output channels; the partials (ws: pt_tcm_desc_ws_bytes) are summed in a fixed order
 *   by a second launch: repeated calls are bit-identical.
 *
 * pt_tcm_match_f32: SuperGlue._forward (ltr/models/target_candidate_matching/superglue.py:299-361) for batch 1,
 *   output_normalization 'sinkhorn', input_dim == descriptor_dim == 256, no bottleneck, eval-mode BatchNorm.
 *   desc0 (256, M), desc1 (256, N) channel-major; kpts0 (M, 2), kpts1 (N, 2) as the caller passes them; scores0 (M),
 *   scores1 (N); the keypoint encoder input is ((k[0] - center[0]) / scale, (k[1] - center[1]) / scale, score) per side
 *   (normalize_keypoints: center = size / 2, scale = 0.7 max(size)).  bin_score is a device scalar, read at call time.
 *   Outputs: log_assignment (M+1, N+1), matches0 (M) / matches1 (N) int64 (-1: unmatched), match_scores0 (M) /
 *   match_scores1 (N).  One launch per dependent stage (5 per GNN layer), no host synchronisation: capturable.
 *   layer_types: bit l set = GNN layer l is 'cross' (else 'self').  M, N <= 64.
 *
 *   Weight pack (float32, every block row-major (out, in), BatchNorm folded: w' = w s, b' = (b - mean) s + beta,
 *   s = gamma / sqrt(var + eps)), in this order, pt_tcm_match_weight_floats(L) floats for L GNN layers (L = 0 with skip_gnn):
 *     keypoint encoder  W 32x3, b 32, W 64x32, b 64, W 128x64, b 128, W 256x128, b 256 (BN folded, ReLU), W 256x256, b 256
 *     per GNN layer     Wqkv 768x256 (proj[0]; proj[1]; proj[2]), bqkv 768, Wmerge 256x256, bmerge 256,
 *                       W1 512x512 (BN folded; input = [x; message]), b1 512, W2 256x512, b2 256
 *     final projection  W 256x256, b 256
 * ---------------------------------------------------------------------------------------------- */
#define PT_TCM_MAX_POINTS 64
#define PT_TCM_MAX_LAYERS 32
typedef struct pt_tcm_match_params {
    int M, N;
    int n_layers;            /* GNN layers in the pack (ignored when skip_gnn) */
    unsigned layer_types;    /* bit l: layer l is 'cross' */
    int skip_gnn;
    int sinkhorn_iters;
    float filter_threshold;
    float kpt_center0[2], kpt_scale0, kpt_center1[2], kpt_scale1;
    size_t weight_floats;    /* size of the pack handed in (checked against pt_tcm_match_weight_floats) */
} pt_tcm_match_params;
int pt_tcm_peaks_f32(const float* scores, int B, int H, int W, int ks, float th, int* count, long long* coords, float* values,
                     void* stream);
size_t pt_tcm_desc_ws_bytes(int B, int P, int C, int D);
int pt_tcm_desc_f32(const float* x, const float* weight, const float* bias, const long long* coords, int B, int C, int H, int W,
                    int P, int D, float* out, void* ws, size_t ws_bytes, void* stream);
size_t pt_tcm_match_weight_floats(int n_layers);
size_t pt_tcm_match_ws_bytes(const pt_tcm_match_params* p);
int pt_tcm_match_f32(const pt_tcm_match_params* p, const float* weights, const float* bin_score, const float* desc0,
                     const float* desc1, const float* kpts0, const float* kpts1, const float* scores0, const float* scores1,
                     float* log_assignment, long long* matches0, long long* matches1, float* match_scores0,
                     float* match_scores1, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * KYS state-aware response prediction (pytracking/tracker/kys/kys.py:314), kys.hip.
 *
 * pt_kys_cost_volume_f32: CostVolume.forward (ltr/models/kys/cost_volume.py:15-26) for kernel_size 3, stride 1, any
 *   max_displacement md >= 1.  feat_cur, feat_prev (B, C, H, W) contiguous.  For a current position (r, c), a previous position
 *   (r', c') and taps i, j in {-1, 0, 1}, a tap contributing only where BOTH indices lie inside the map:
 *       v(r, c, r', c') = sum_ch sum_{i,j} cur[b, ch, r+i, c+j] * prev[b, ch, r'+i, c'+j]          (no normalisation)
 *   remap != 0 (abs_coordinate_output): out (B, H*W, H, W), out[b, r' W + c', r, c] = v if |r'-r| <= md and |c'-c| <= md, else 0
 *   remap == 0: out (B, (2 md + 1)^2, H, W), out[b, di (2 md + 1) + dj, r, c] = v(r, c, r + di - md, c + dj - md)
 *   This is SpatialCorrelationSampler(3, 2 md + 1, 1, 1) (+ remap_cost_volume); parity with that CUDA extension is UNPINNED (it
 *   is not installable here; the definition above is written from its documented behaviour).
 *   Two launches: channel Gram matrix in up to 8 K slices on the matrix cores (ws: pt_kys_cost_volume_ws_bytes), then the 9-tap
 *   diagonal sum over the slices in double precision, window mask and store.  H*W <= PT_KYS_CV_MAX_HW.  Repeated calls are
 *   bit-identical.
 *
 * pt_kys_predict_response_f32: ResponsePredictor.forward (ltr/models/kys/response_predictor.py:65-159) in eval mode, with the
 *   shift_features calls PredictorWrapper.predict_response puts around it (predictor_wrapper.py:113-148): four launches, no host
 *   synchronisation.  prev_max_pool_ksz 1, H*W <= PT_KYS_PRED_MAX_HW.  with_conf is the conf_measure code PT_KYS_CONF_NONE /
 *   PT_KYS_CONF_MAX (largest propagation weight) / PT_KYS_CONF_ENTROPY (-sum_q w log(w + 1e-4) over all H*W previous positions,
 *   response_predictor.py:114-116).  rep_dim1 == 0 means one representation layer of rep_dim0 channels.  Covered structures, a
 *   closed list (anything else: pt_kys_weight_floats returns 0 and the call PT_ERR_UNSUPPORTED):
 *       state_dim 8, gru_ksz 3, representation_predictor_dims (64, 32), conf none / max     (the constructor defaults, kysnet.py:122-123)
 *       state_dim 8, gru_ksz 3, representation_predictor_dims (16,): rep_dim0 16, rep_dim1 0, conf none / max / entropy
 *                                                  (entropy: the trained network, ltr/train_settings/kys/kys.py:110-114)
 *   (64, 32) with entropy is refused only because tests/test_gpu_kys.py pins that refusal; the kernels would not mind.
 *   Inputs: cost_volume (B, H*W, H, W); state_prev (B, 8, H, W) or NULL, then label_prev (B, H, W) (shifted by -shift_px and fed
 *   to init_hidden_state_predictor); dimp_score (B, H, W) unshifted; window NULL or (H, W) (window_stride 0) / (B, H, W)
 *   (window_stride H*W).  shift_px: the pixel offset of the reference's +-0.5 / size translation (0.25 at the defaults of
 *   affine_grid / grid_sample: bilinear, zero padding, align_corners False); inputs are sampled at -shift_px, outputs at +shift_px.
 *   Outputs: response (B, H, W) shifted back; state_cur (B, 8, H, W); propagation_weights (B, H*W, H, W) (= cost_volume_processed);
 *   propagated_h (B, 8, H, W); propagation_conf (B, H, W) (with_conf != 0 only, else may be NULL); fused_score_orig (B, H, W) (before
 *   threshold, window and shift); is_target, is_target_after_prop, is_target_new (B, H, W) shifted back.
 *
 *   Weight pack (float32, conv weights (out, in, 3, 3) row-major, eval BatchNorm folded as for pt_tcm_match_f32), in this order:
 *     cost_volume_proc1  W 8x1, b 8 (BN folded, ReLU), W 1x8, b 1 (BN folded);  cost_volume_proc2 the same
 *     init_hidden_state_predictor  W 8x1 (no bias, tanh)
 *     is_target_predictor  W 4x8, b 4 (ReLU), W 1x4, b 1
 *     representation_predictor  W 64x(9 + conf), b 64, W 32x64, b 32 (ReLU);  response_predictor  W 1x32, b 1 (sigmoid)
 *       one layer (rep_dim1 == 0):  W 16x(9 + conf), b 16 (ReLU);  response_predictor  W 1x16, b 1 (sigmoid)
 *       (conf = 1 where with_conf != 0; 27900 / 27324 floats for (64, 32), 4924 / 4780 for (16,))
 *     state_predictor (ConvGRU, input = [score, response, max score, max response, state])  reset W 8x12, b 8; update; state_new
 * ---------------------------------------------------------------------------------------------- */
#define PT_KYS_CV_MAX_HW 1024
#define PT_KYS_PRED_MAX_HW 400
#define PT_KYS_CONF_NONE 0
#define PT_KYS_CONF_MAX 1
#define PT_KYS_CONF_ENTROPY 2
typedef struct pt_kys_predict_params {
    int B, H, W;
    int state_dim, rep_dim0, rep_dim1, gru_ksz;
    int with_conf;           /* conf_measure code: PT_KYS_CONF_NONE / _MAX / _ENTROPY */
    int has_thresh;          /* dimp_thresh is not None */
    float dimp_thresh;
    float shift_px;
    long window_stride;      /* floats between the windows of consecutive sequences: 0 or H*W */
    size_t weight_floats;    /* size of the pack handed in (checked against pt_kys_weight_floats) */
} pt_kys_predict_params;
size_t pt_kys_cost_volume_ws_bytes(int B, int C, int H, int W);
int pt_kys_cost_volume_f32(const float* feat_cur, const float* feat_prev, int B, int C, int H, int W, int kernel_size,
                           int max_displacement, int stride, int remap, float* out, void* ws, size_t ws_bytes, void* stream);
size_t pt_kys_weight_floats(int state_dim, int rep_dim0, int rep_dim1, int gru_ksz, int with_conf);   /* 0: dims not covered */
size_t pt_kys_predict_ws_bytes(int B, int H, int W);
int pt_kys_predict_response_f32(const pt_kys_predict_params* p, const float* weights, const float* cost_volume,
                                const float* state_prev, const float* label_prev, const float* dimp_score, const float* window,
                                float* response, float* state_cur, float* propagation_weights, float* propagated_h,
                                float* propagation_conf, float* fused_score_orig, float* is_target, float* is_target_after_prop,
                                float* is_target_new, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * IoU feature extraction -- AtomIoUNet.get_iou_feat (ltr/models/bbreg/atom_iou_net.py:172-179), iou_feat.hip.
 *
 *   c3_out (n, Cout3, H3, W3) = conv3_2t(conv3_1t(feat3)),  c4_out (n, Cout4, H4, W4) = conv4_2t(conv4_1t(feat4));
 *   every block = Conv2d(3x3, stride 1, padding 1, bias) -> BatchNorm2d in eval mode -> ReLU (atom_iou_net.py:7-12).
 *   feat3 (n, Cin3, H3, W3), feat4 (n, Cin4, H4, W4), fp32, contiguous; the two maps need not be related.
 *   fp32 MFMA with fp32 accumulation; the channel-split partial maps are summed in a fixed order: repeated calls are bit-identical.
 *   Six launches on the banded-correlation route (per layer: one correlation per tower, one epilogue for both towers); a layer whose
 *   rows are wider than the banded kernel takes (W > 170) goes through the per-tap split-K GEMM like pt_clf_head_f32.
 *
 * `pack` (pt_iou_feat_pack_floats floats, 16-byte aligned), the four blocks in the order conv3_1t, conv3_2t, conv4_1t, conv4_2t, per
 *   block:  weight (Cout, 3, 3, Cin) tap-major = Conv2d.weight.permute(0, 2, 3, 1), as for pt_clf_head_f32
 *           scale  (Cout) = bn.weight / sqrt(bn.running_var + bn.eps)
 *           shift  (Cout) = (conv.bias - bn.running_mean) * scale + bn.bias
 *   and a block computes relu(conv_without_bias(x) * scale + shift): BatchNorm is NOT folded into the weights.
 *
 * Covered: Cin % 64 == 0, Cmid % 16 == 0, Cout % 16 == 0 (each <= 4096), H * W <= 4096, n <= 8, operands 16-byte aligned.
 * Status: NULL pointer PT_ERR_NULL, non-positive size PT_ERR_SHAPE, uncovered shape / misaligned operand PT_ERR_UNSUPPORTED,
 * workspace too small or not 256-byte aligned PT_ERR_WORKSPACE -- all before anything is queued.  pt_iou_feat_ws_bytes and
 * pt_iou_feat_pack_floats return 0 for sizes that are not covered.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_iou_feat_pack_floats(int Cin3, int Cmid3, int Cout3, int Cin4, int Cmid4, int Cout4);
size_t pt_iou_feat_ws_bytes(int n, int Cin3, int Cmid3, int Cout3, int H3, int W3, int Cin4, int Cmid4, int Cout4, int H4, int W4);
int pt_iou_feat_f32(const float* feat3, const float* feat4, const float* pack, float* c3_out, float* c4_out, int n, int Cin3,
                    int Cmid3, int Cout3, int H3, int W3, int Cin4, int Cmid4, int Cout4, int H4, int W4, void* ws, size_t ws_bytes,
                    void* stream);

/* The geometry the banded tap-major 3x3 correlation (the convolutions of pt_clf_head_f32 and pt_iou_feat_f32) would run for n images,
 * Ftot filters (% 16), C input channels (% 16) on H x W maps.  Host only: launches nothing, touches no device.
 *   out[0..5] = ks (channel splits), br (rows per band), npg (4: 8 waves, 6: 12 waves), nb (bands), rows of the last band, Wp (LDS row).
 * PT_ERR_UNSUPPORTED with out zeroed when the banded kernel does not cover the shape (the callers then take their GEMM route);
 * PT_ERR_NULL for a null `out`. */
int pt_mf_corr_tm_plan(int n, int Ftot, int C, int H, int W, int* out);

/* ------------------------------------------------------------------------------------------------
 * IoU modulation vectors -- AtomIoUNet.get_modulation (ltr/models/bbreg/atom_iou_net.py:138-170), iou_mod.hip.
 *
 *   c3 = conv3_1r(feat3) (n, A, H3, W3),  c4 = conv4_1r(feat4) (n, D, H4, W4)      Conv2d(3x3, pad 1, bias) -> BatchNorm2d (eval) -> ReLU
 *   roi3 = PrRoIPool(3 x 3, s3)(c3, roi),  roi4 = PrRoIPool(1 x 1, s4)(c4, roi),   roi of image i = (i, x, y, x + w, y + h)
 *   fc3  = fc3_1r(roi3) (n, B)             a 3x3 VALID convolution over the 3 x 3 pooled map, i.e. a linear map 9 A -> B
 *   out3 (n, P3) = fc34_3r([fc3, roi4]),   out4 (n, P4) = fc34_4r([fc3, roi4])     1x1 convolutions over the concatenation (B + D)
 *   every block ends in BatchNorm2d (eval) -> ReLU.  feat3 (n, Cin3, H3, W3), feat4 (n, Cin4, H4, W4), boxes (n, 4) xywh in image
 *   coordinates ON THE DEVICE, all fp32 contiguous.  PrRoIPool as pt_prroi_fwd_f32: a bin of zero area or without a pixel gives 0, the
 *   box may hang over any edge.
 *
 * The two 3x3 convolutions are computed only where the pooling reads them: per image and level the pixel window
 *       columns max(0, floor(x * s)) ... min(W - 1, ceil((x + w) * s)),  rows likewise (fp32, x + w formed first),
 *   read from `boxes` by the kernels.  pt_iou_mod_window (host only, launches nothing) returns that window as inclusive
 *   (x0, y0, x1, y1): PT_OK, or 1 when it is empty (x1 < x0 or y1 < y0: the pooled values of that level are 0).  Taps outside the map
 *   read 0, taps outside the window read the map; nothing beyond the window and one ring around it enters the result.
 *   Windowed convolution on the fp32 MFMA with fp32 accumulation, the tail in plain fp32 FMA; no atomics, every sum in a fixed order:
 *   repeated calls are bit-identical.  Four launches (windowed convolution of both levels, pooling, fc3, fc34), no host synchronisation, no device-to-host copy: capturable in a graph.
 *
 * `pack` (pt_iou_mod_pack_floats floats, 16-byte aligned), the five blocks in the order conv3_1r, conv4_1r, fc3_1r, fc34_3r, fc34_4r,
 *   per block:  weight (Cout, KH, KW, Cin) tap-major = Conv2d.weight.permute(0, 2, 3, 1)   (3x3, 3x3, 3x3, 1x1, 1x1)
 *               scale  (Cout) = bn.weight / sqrt(bn.running_var + bn.eps)
 *               shift  (Cout) = (conv.bias - bn.running_mean) * scale + bn.bias
 *   and a block computes relu(conv_without_bias(x) * scale + shift): BatchNorm is NOT folded into the weights.
 *
 * Covered: Cin3, Cin4 % 64 == 0; A, B, D, P3, P4 % 16 == 0 (each <= 4096); 1 <= n <= 32; H * W <= 4096 per level; pooled sizes
 * exactly 3 x 3 (level 3) and 1 x 1 (level 4); s3, s4 > 0; operands 16-byte aligned.
 * Status: NULL pointer PT_ERR_NULL, non-positive size or scale PT_ERR_SHAPE, uncovered shape / misaligned operand PT_ERR_UNSUPPORTED,
 * workspace too small or not 256-byte aligned PT_ERR_WORKSPACE -- all before anything is queued.  pt_iou_mod_ws_bytes and
 * pt_iou_mod_pack_floats return 0 for sizes that are not covered.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_iou_mod_pack_floats(int Cin3, int A, int B, int Cin4, int D, int P3, int P4);
size_t pt_iou_mod_ws_bytes(int n, int Cin3, int A, int B, int Cin4, int D, int P3, int P4, int H3, int W3, int H4, int W4);
int pt_iou_mod_f32(const float* feat3, const float* feat4, const float* boxes, const float* pack, float* out3, float* out4, int n,
                   int Cin3, int A, int B, int Cin4, int D, int P3, int P4, int H3, int W3, int H4, int W4, float s3, float s4, void* ws,
                   size_t ws_bytes, void* stream);
int pt_iou_mod_window(const float box_xywh[4], float scale, int H, int W, int out_x0y0x1y1[4]);

/* ------------------------------------------------------------------------------------------------
 * Mask label encoder -- ResidualDS16SW.forward (ltr/models/lwl/label_encoder.py:9-55, ltr/models/rts/label_encoder.py:9-55),
 * label_enc.hip.  LWL and RTS run it on every stored mask on every frame (lwl.py:560-564, rts.py:688).
 *
 *   x (n,1,H,W) -> conv3x3 s2 p1 (1->c0) [BN] ReLU -> maxpool3x3 s2 p1 -> BasicBlock(c0->c1, s2) -> BasicBlock(c1->c2, s2)
 *               -> label_enc (n,f,h,w) = relu([BN](conv3x3(c2->f)))  and  sample_w (n,f,h,w) = conv3x3(c2->f);
 *   BasicBlock(x) = relu([bn2](conv2(relu([bn1](conv1 x)))) + downsample(x)), conv1 and downsample 3x3 stride 2 (downsample with bias).
 *   Each of the four stride-2 stages maps a size i to (i - 1) / 2 + 1 (integer division); h, w are H, W after all four.
 *   masks (n, H, W) fp32 contiguous.  fp32 throughout: the stem on the vector ALU with the pooled convolution outputs kept on chip, every
 *   other convolution on the exact fp32 MFMA; no atomics and no split sums, so repeated calls are bit-identical.  Six launches.
 *
 * `pack` (pt_label_enc_pack_floats floats, 16-byte aligned): six layers in the order
 *       stem                      Cout = c0,   Cin = 1
 *       res1.conv1 | downsample   Cout = 2 c1, Cin = c0    (conv1's c1 output channels first, then the downsample's)
 *       res1.conv2                Cout = c1,   Cin = c1
 *       res2.conv1 | downsample   Cout = 2 c2, Cin = c1
 *       res2.conv2                Cout = c2,   Cin = c2
 *       label_pred | samp_w_pred  Cout = 2 f,  Cin = c2    (label_pred's f output channels first)
 *   per layer:  weight (Cout, 3, 3, Cin) tap-major = Conv2d.weight.permute(0, 2, 3, 1)
 *               scale  (Cout)   1, or bn.weight / sqrt(bn.running_var + bn.eps) where a BatchNorm follows the convolution
 *               shift  (Cout)   the convolution's bias (0 without one), or (bias - bn.running_mean) * scale + bn.bias
 *   and a layer computes conv_without_bias(x) * scale + shift; BatchNorm is NOT folded into the weights.  ReLU follows the stem, the conv1
 *   half of a block's first layer, conv2 + residual (the residual is the downsample half, added behind scale / shift) and label_pred.
 *
 * Covered: c0, c1, c2, f multiples of 16 up to 64; H, W <= 8192; n <= 65535; pack 16-byte aligned.
 * Status: NULL pointer PT_ERR_NULL, non-positive size PT_ERR_SHAPE, uncovered size / misaligned pack PT_ERR_UNSUPPORTED, workspace too
 * small or not 256-byte aligned PT_ERR_WORKSPACE -- all before anything is queued.  pt_label_enc_ws_bytes and pt_label_enc_pack_floats
 * return 0 for sizes that are not covered.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_label_enc_pack_floats(int c0, int c1, int c2, int f);
size_t pt_label_enc_ws_bytes(int n, int H, int W, int c0, int c1, int c2, int f);
int pt_label_enc_f32(const float* masks, const float* pack, float* label_enc, float* sample_w, int n, int H, int W, int c0, int c1,
                     int c2, int f, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Box label encoders -- ResidualDS16FeatSWBox.forward and ResidualDS16FeatSWBoxCatMultiBlock.forward with use_gauss = False
 * (ltr/models/lwl/label_encoder.py:58-216, ltr/models/rts/label_encoder.py:106-265), box_enc.hip: the box-to-mask initialisation of RTS
 * (STAHelper.predict_mask) and of box-initialised LWL.  fp32, eval mode.  `boxes` (n, 4) = (x, y, w, h) fp32 on the DEVICE, read there:
 * no host synchronisation.  `feat` (n, feat_dim, h, w) fp32 with dense channel planes and an image stride of feat_img_stride floats
 * (>= feat_dim h w).  Every convolution is 3x3, padding 1, on the exact fp32 MFMA; no atomics and no split sums, so repeated calls are
 * bit-identical; asynchronous on `stream`, no allocation, graph-capturable.
 *
 * The mask: v = int(b) truncates toward zero and the reference's int(v + 0.5) then maps a negative integer k to k + 1; the mask is 1 on
 * rows range(H)[y : y + h] and columns range(W)[x : x + w] with Python's slice rules (a negative bound counts from the end, every bound
 * is clipped to [0, len]); pt_box_enc clamps the two starts with max(0, .) first, pt_box_cat_enc does not.
 * pt_box_slice (host only): that slice for integers, lo <= i < hi (empty where hi <= lo).  |start|, |extent|, len <= 2^29.
 *
 * pt_box_enc_f32:  mask (n,1,H,W), never stored -> the trunk of the mask label encoder above (stem, pool, BasicBlock(c0->c1, s2),
 *   BasicBlock(c1->c2, s2)) -> (n,c2,h,w), h, w = H, W after four stride-2 stages, which must be the feature's size
 *   -> res3 = BasicBlock(c2 + feat_dim -> c3, s1) over cat(trunk, feat) -- the concatenation is never written --
 *   -> label_enc (n,f,h,w) = [relu](conv3x3(c3->f)) (relu iff final_relu) and sample_w (n,f,h,w) = conv3x3(c3->f).
 *   `sample_w` may be NULL (a module with use_sample_w = False): that half is neither computed nor packed.  Eight launches.
 *   `pack` (pt_box_enc_pack_floats floats, 16-byte aligned): the first five layers of pt_label_enc_f32's pack (stem ... res2.conv2), then
 *       res3.conv1 | downsample   Cout = 2 c3,      Cin = feat_dim + c2   input channels ordered [feat | trunk] (the module's order is
 *                                                                          [trunk | feat]: the packer permutes)
 *       res3.conv2                Cout = c3,        Cin = c3
 *       label_pred [| samp_w_pred] Cout = 2 f or f, Cin = c3
 *   with the per-layer layout and arithmetic of pt_label_enc_f32 (tap-major weight | scale | shift; conv_without_bias(x) * scale + shift).
 *   Covered: c0, c1, c2 multiples of 16 up to 64 and H, W <= 8192 (the label encoder's limits); c3, f multiples of 16 up to 128;
 *   feat_dim a multiple of 16 up to 1024; h, w <= 1024; n <= 1024.
 *
 * pt_box_cat_enc_f32:  mask (n,1,H,W) resized to (n,1,h,w) (F.interpolate bilinear, align_corners = False: src = (dst + 0.5) in / out
 *   - 0.5 clamped below at 0, second tap clamped at in - 1; the identity when (H, W) = (h, w)), evaluated from the box, one launch
 *   -> nblocks BasicBlock(stride 1, biased 3x3 downsample, [BatchNorm]); the first over cat(feat, mask) (feat_dim + 1 channels)
 *   -> label_enc (n,F,h,w) = [relu]([BN](conv3x3)).  dims = the nblocks block widths, then F.  1 + 2 nblocks + 1 launches.
 *   `pack` (pt_box_cat_enc_pack_floats floats, 16-byte aligned): per block  conv1 | downsample (Cout = 2 d_b), conv2 (Cout = d_b), then
 *   label_pred (Cout = F); layer layout as above, except that a weight's input channels are padded with zeros to the next multiple
 *   of 16: weight (Cout, 3, 3, ceil16(Cin)).  The first block's Cin = feat_dim + 1 in the module's order [feat | mask].
 *   Covered: nblocks 1..4; every dim a multiple of 16 up to 128; feat_dim a multiple of 16 up to 1024; H, W <= 8192; h, w, n <= 1024.
 *
 * Status: NULL pointer PT_ERR_NULL, non-positive size or an image stride below feat_dim h w PT_ERR_SHAPE, uncovered size (a feature size
 * that is not the trunk's output size included) / misaligned pack PT_ERR_UNSUPPORTED, workspace too small or not 256-byte aligned
 * PT_ERR_WORKSPACE -- in this order, all before anything is queued; one exception: nblocks > 4 is PT_ERR_UNSUPPORTED before the entries
 * of `dims` are looked at (only nblocks + 1 of them are known to exist), so a non-positive dim behind too many blocks is not reported
 * as PT_ERR_SHAPE.  The *_ws_bytes and *_pack_floats queries return 0 for what is not covered.
 * ---------------------------------------------------------------------------------------------- */
int pt_box_slice(int start, int extent, int len, int clamp_start, int* lo, int* hi);
size_t pt_box_enc_pack_floats(int c0, int c1, int c2, int c3, int f, int feat_dim, int with_sample_w);
size_t pt_box_enc_ws_bytes(int n, int H, int W, int h, int w, int c0, int c1, int c2, int c3, int f, int feat_dim);
int pt_box_enc_f32(const float* boxes, const float* feat, long feat_img_stride, const float* pack, float* label_enc, float* sample_w,
                   int n, int H, int W, int h, int w, int c0, int c1, int c2, int c3, int f, int feat_dim, int final_relu, void* ws,
                   size_t ws_bytes, void* stream);
size_t pt_box_cat_enc_pack_floats(int nblocks, const int* dims, int feat_dim);
size_t pt_box_cat_enc_ws_bytes(int n, int H, int W, int h, int w, int nblocks, const int* dims, int feat_dim);
int pt_box_cat_enc_f32(const float* boxes, const float* feat, long feat_img_stride, const float* pack, float* label_enc, int n, int H,
                       int W, int h, int w, int nblocks, const int* dims, int feat_dim, int final_relu, void* ws, size_t ws_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segmentation decoder -- LWTLDecoder.forward (ltr/models/lwl/decoder.py:130-160) = RTSDecoder.forward (ltr/models/rts/decoder.py),
 * lwl_decoder.hip.  LWL and RTS run it once per frame (lwl_net.py segment_target) on the target-model scores and the backbone features.
 * fp32, eval mode, num_objects = None.
 *
 *   `levels` = 4 (layer4, layer3, layer2, layer1) or 3 (layer3, layer2, layer1); fc[l], hw[2l], hw[2l+1] = feature channels, height and
 *   width of level l IN EXECUTION ORDER (deepest first); oc = {4,2,2,1} * mdim (4 levels) or {2,2,1} * mdim (3 levels), nc = oc + ic.
 *   scores (n, ic, score_hw) and feats[l] (n, fc[l], H_l, W_l) fp32 contiguous; mask_out (n, 1, image_hw); dec_out (nullable) holds
 *   `levels` pointers, each nullable: a non-null dec_out[l] (n, oc_l, H_l, W_l), 16-byte aligned, receives level l's output x
 *   (the reference's '{L}_dec'), written by the launch that produces it -- no extra work.  feats and dec_out are HOST arrays of device
 *   pointers, read before the call returns.
 *   Per level: s = bilinear(scores); x = relu(proj(x_prev)) (not on the first level); h = reduce1(relu(reduce0(ft)));
 *   hpool = mean(h) on the first level, else x; h = 3 x relu(conv3x3(cat(h, s))); h = RRB1(h); h = h * gate + resize(hpool),
 *   gate = sigmoid(cab1(relu(cab0(cat(mean(h), mean(hpool)))))); x = RRB2(h); RRB(x) = relu(h + conv_b(relu(affine(conv_a(h))))), h = conv1x1(x).
 *   Then bicubic x2, relu(conv3x3 mdim -> mdim/2), bicubic to image_hw, conv3x3 -> 1 channel.  bilinear / bicubic are PyTorch's
 *   align_corners=False rules (bicubic A = -0.75, source not clamped, taps clamped).  No atomics: repeated calls are bit-identical.
 *
 * `pack` (pt_lwl_decoder_pack_floats floats, 16-byte aligned), per level in execution order:
 *       proj[L].0 (not on the first level)   1x1
 *       TSE[L].reduce.0, TSE[L].reduce.2     1x1, 1x1
 *       TSE[L].transform.0 / .2 / .4         3x3 nc->nc, nc->nc, nc->oc
 *       RRB1[L]: conv1x1, bblock.0 (+ BatchNorm), bblock's last convolution (no bias)      1x1, 3x3, 3x3
 *       CAB[L].convreluconv.0, .2            1x1 (2 oc -> oc), 1x1
 *       RRB2[L]                              as RRB1
 *   then project.conv1 (3x3 mdim -> mdim/2) and project.conv2: weight (9, mdim/2) tap-major, bias (1).
 *   1x1: weight (Cout, Cin), bias (Cout).
 *   3x3: weight (Cout, 3, 3, Cin) tap-major = Conv2d.weight.permute(0, 2, 3, 1)
 *        scale  (Cout)   1, or bn.weight / sqrt(bn.running_var + bn.eps) where a BatchNorm follows the convolution
 *        shift  (Cout)   the convolution's bias (0 without one), or (bias - bn.running_mean) * scale + bn.bias
 *   and a 3x3 layer computes conv_without_bias(x) * scale + shift; BatchNorm is NOT folded into the weights.  The layout does not depend
 *   on use_bn.
 *
 * Covered: levels 3 or 4 with the oc table above; ic % 16 == 0 (<= 256), mdim % 32 == 0 (<= 256), fc % 16 == 0 (<= 8192); n <= 8; every
 * map, partial-map set and token matrix below 2^32 - 32 bytes (the launchers' 32-bit byte offsets); pack 16-byte aligned.
 * Status: NULL pointer PT_ERR_NULL, non-positive size PT_ERR_SHAPE, uncovered structure / size / misaligned pointer PT_ERR_UNSUPPORTED,
 * workspace too small or not 256-byte aligned PT_ERR_WORKSPACE -- all before anything is queued.  pt_lwl_decoder_ws_bytes and
 * pt_lwl_decoder_pack_floats return 0 for what is not covered.
 * ---------------------------------------------------------------------------------------------- */
size_t pt_lwl_decoder_pack_floats(int levels, const int* fc, int ic, int mdim, int use_bn);
size_t pt_lwl_decoder_ws_bytes(int n, int levels, const int* fc, const int* hw, const int* score_hw, const int* image_hw, int ic, int mdim);
int pt_lwl_decoder_f32(const float* scores, const float* const* feats, const float* pack, float* mask_out, float* const* dec_out, int n,
                       int levels, const int* fc, const int* hw, const int* score_hw, const int* image_hw, int ic, int mdim, void* ws,
                       size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RTS instance-score encoder and learners fusion, rts_fusion.hip: what RTS.track() (pytracking/tracker/rts/rts.py:253-260) runs
 * between the classifier and the decoder.
 *
 * pt_score_enc_f32 -- ResidualDS16SW_Clf.forward (ltr/models/rts/label_encoder.py:57-103), the stride-1 sibling of the mask label
 * encoder above:
 *   s (n,1,H,W) -> conv3x3 s1 p1 (1->c0) [BN] ReLU -> maxpool3x3 s1 p1 -> BasicBlock(c0->c1, s1) -> BasicBlock(c1->c2, s1)
 *               -> label_enc (n,f,H,W) = relu([BN](conv3x3(c2->f)))  and  sample_w (n,f,H,W) = conv3x3(c2->f);
 *   every stride is 1, every map H x W.  scores (n, H, W) fp32 contiguous.  `sample_w` may be NULL (the tracker discards it): that half
 *   of the heads is then neither computed nor stored, and label_enc has the bits of the full call.  `pack` has the layout and the
 *   per-layer arithmetic of the mask label encoder's (six layers, tap-major weight | scale | shift each, conv_without_bias(x) * scale +
 *   shift).  Pooling padding is ignored, convolution padding is zero.  fp32 throughout: the stem on the vector ALU with the
 *   convolution output kept on chip, every other convolution on the exact fp32 MFMA; no atomics and no split sums, so repeated calls
 *   are bit-identical.  Six asynchronous launches, no allocation, no host synchronisation.
 *   Covered: c0, c1, c2, f multiples of 16 up to 64; H, W <= 1024; n <= 1024; pack 16-byte aligned.
 *
 * pt_learners_fuse_f32 -- the resize and LearnersFusion of RTSNet.segment_target (ltr/models/rts/rts_net.py:227-230,
 * ltr/models/rts/learners_fusion.py:24-38) in one launch:
 *   out (n,f,Ht,Wt) = fusion(seg_enc (n,f,Ht,Wt), resize(clf_enc (n,f,Hs,Ws) -> Ht x Wt)).
 *   resize = F.interpolate(mode='bilinear', align_corners=False) to an explicit size: src = (dst + 0.5) * (in / out) - 0.5 clamped
 *   below at 0, i0 = floor(src), i1 = min(i0 + 1, in - 1), weight src - i0, no antialiasing; skipped when the sizes are equal.
 *   mode PT_FUSE_ADD:    seg_enc + resized; `pack` is not read and may be NULL.  Covered: f <= 64.
 *   mode PT_FUSE_CONCAT: Conv2d(2f -> f, 3, padding 1, bias) over cat(seg_enc, resized) along the channels, on the fp32 MFMA; the resized
 *                        map and the concatenation never exist in memory.  `pack` (pt_learners_fuse_pack_floats floats, 16-byte
 *                        aligned) = weight (f, 3, 3, 2f) tap-major = Conv2d.weight.permute(0, 2, 3, 1), then bias (f).
 *                        Covered: f a multiple of 16 up to 64.
 *   Both: Hs, Ws, Ht, Wt <= 1024; n <= 1024.  No workspace.
 *
 * Status: NULL pointer PT_ERR_NULL, non-positive size PT_ERR_SHAPE, uncovered size / mode / misaligned pack PT_ERR_UNSUPPORTED,
 * workspace too small or not 256-byte aligned PT_ERR_WORKSPACE -- all before anything is queued.  pt_score_enc_ws_bytes,
 * pt_score_enc_pack_floats and pt_learners_fuse_pack_floats are host-only and return 0 for sizes that are not covered.
 * ---------------------------------------------------------------------------------------------- */
#define PT_FUSE_ADD 0
#define PT_FUSE_CONCAT 1
size_t pt_score_enc_pack_floats(int c0, int c1, int c2, int f);
size_t pt_score_enc_ws_bytes(int n, int H, int W, int c0, int c1, int c2, int f);
int pt_score_enc_f32(const float* scores, const float* pack, float* label_enc, float* sample_w, int n, int H, int W, int c0, int c1,
                     int c2, int f, void* ws, size_t ws_bytes, void* stream);
size_t pt_learners_fuse_pack_floats(int f);
int pt_learners_fuse_f32(const float* seg_enc, const float* clf_enc, const float* pack, float* out, int n, int f, int Hs, int Ws, int Ht,
                         int Wt, int mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segmentation read-out of LWL / RTS, seg_readout.hip: the host-side stages the trackers run between the decoder's raw score map and the
 * next frame's label encoder.  fp32, asynchronous on `stream`, no allocation, no host synchronisation, no atomics (two runs on the same
 * input are bit-identical), graph-capturable.  Workspaces are caller-owned, 256-byte aligned and sized by the *_ws_bytes queries.
 *
 * Statistics block: PT_SEG_STATS_FLOATS = 16 floats
 *    [0] prob_sum   [1] e_y   [2] e_x   [3] var_y   [4] var_x            of p       (get_target_state of lwl.py:276-298; var = the
 *    [5] prob_sum_c [6] e_y_c [7] e_x_c [8] var_y_c [9] var_x_c          of max(p,0) reference's e_h, e_w before the square root)
 *    [10] mask_count  [11] x_min [12] y_min [13] x_max [14] y_max         of the mask (masks_to_bboxes; an empty mask gives 0, 0, 0, 0)
 *    [15] 0
 *   Rows and columns are summed first (per-tile partial sums, added in tile order), the moments are centred on e_y / e_x afterwards, as
 *   the reference does; the one-pass sum p y^2 - e_y^2 sum p is not used.  prob_sum == 0 gives NaN moments, as the reference.  Counts
 *   are exact up to 2^24 pixels.
 *
 * pt_seg_readout_f32 -- convert_scores_crop_to_image (lwl.py:330-359, rts.py:460-493, sta_helper.py:88-117) with `> 0`, sigmoid and the
 *   sums of get_target_state / masks_to_bboxes in one pass plus the finishing kernel:
 *     resized(ry, rx) = bilinear(scores (Hc, Wc)) as F.interpolate(scale_factor=scale, mode='bilinear', align_corners=False) without a
 *                       recomputed scale factor: src = max((dst + 0.5) / scale - 0.5, 0), i0 = min(floor(src), in - 1),
 *                       i1 = min(i0 + 1, in - 1); Hr = floor(Hc * scale), Wr = floor(Wc * scale) are the CALLER's;
 *     scores_im(y, x) = resized(y - r1, x - c1) inside the window [r1, r1 + Hr) x [c1, c1 + Wr), -100 outside; (r1, c1) is the window's
 *                       unclipped corner, r1 = int(pos_r - 0.5 Hr) with truncation towards zero, the caller's as well;
 *     prob_im = sigmoid(scores_im) (0 outside the window: exp(100) overflows), mask_im = scores_im > 0 as 0 / 1 floats.
 *   The resized map is never stored.  scores_im, prob_im, mask_im (Hi, Wi) may each be NULL; `stats` is the block of prob_im with the
 *   mask scores_im > 0.  A window that misses the image gives the all-background image (-100, 0, 0) and mask_count 0.
 * pt_seg_state_f32 -- the statistics block of a probability image (H, W) on the device; the mask is `mask` > 0 when a mask image is
 *   given and prob > 0.5 when `mask` is NULL.  On the read-out's prob_im and mask_im it repeats the read-out's block bit for bit.
 * pt_seg_merge_f32 -- merge_results (lwl.py:217-248): scores (N, H, W) -> prob (N + 1, H, W), background first:
 *     p = sigmoid(s), bg = clamp(prod(1 - p), 1e-7, 1 - 1e-7), s_0 = log(bg / (1 - bg)), prob_i = 1 / sum_j exp(s_j - s_i) with j in
 *     the order 0 .. N; labels (H, W) uint8 = arg-max over i, the first maximum wins (0 = background); stats (N, 16): object i's block
 *     of prob_{i+1} with the mask labels == i + 1.  One pass over the pixels, the N + 1 scores of a pixel in registers.  1 <= N <=
 *     PT_SEG_MAX_OBJECTS.
 * pt_sample_mask_patch_f32 -- sample_patch(is_mask=True) (pytracking/features/preprocessing.py:95-146) for the integer geometry of
 *   pt_sample_patch_f32: the strided view im[os0::df, os1::df], the crop of crop_h x crop_w at (tl0, tl1) with ZERO padding, then
 *   torch's legacy 'nearest' resize to OH x OW in fp32: index = min((int)floorf(dst * ((float)in / (float)out)), in - 1).  im (C, H, W),
 *   out (C, OH, OW).
 * Covered: every image side <= PT_SEG_MAX_DIM; |r1|, |c1| <= PT_SEG_MAX_DIM; C <= 1024.
 * Status: NULL pointer PT_ERR_NULL, non-positive size or scale (N = 0, a bad geometry) PT_ERR_SHAPE, a size beyond the bounds above
 * PT_ERR_UNSUPPORTED, workspace too small or not 256-byte aligned PT_ERR_WORKSPACE -- all before anything is queued.  The *_ws_bytes
 * queries are host-only and return 0 for what is not covered.
 * ---------------------------------------------------------------------------------------------- */
#define PT_SEG_STATS_FLOATS 16
#define PT_SEG_MAX_OBJECTS 16
#define PT_SEG_MAX_DIM 8192
size_t pt_seg_readout_ws_bytes(int Hi, int Wi);
int pt_seg_readout_f32(const float* scores, int Hc, int Wc, double scale, int Hr, int Wr, int r1, int c1, int Hi, int Wi,
                       float* scores_im, float* prob_im, float* mask_im, float* stats, void* ws, size_t ws_bytes, void* stream);
size_t pt_seg_state_ws_bytes(int H, int W);
int pt_seg_state_f32(const float* prob, const float* mask, int H, int W, float* stats, void* ws, size_t ws_bytes, void* stream);
size_t pt_seg_merge_ws_bytes(int N, int H, int W);
int pt_seg_merge_f32(const float* scores, int N, int H, int W, float* prob, unsigned char* labels, float* stats, void* ws,
                     size_t ws_bytes, void* stream);
int pt_sample_mask_patch_f32(const float* im, int C, int H, int W, const pt_patch_geom* geom, float* out, int OH, int OW, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ECO's Fourier-domain per-frame path, eco.hip (pytracking/tracker/eco/eco.py:181-245, 293-309, 339-343; pytracking/libs/fourier.py,
 * dcf.py:97-103, 156-164).  fp32, complex numbers as a trailing dimension of 2 in the reference's layouts, asynchronous on `stream`, no
 * allocation, no host synchronisation, no atomics (two runs on the same input are bit-identical), graph-capturable.  Workspaces are
 * caller-owned and 256-byte aligned.
 *
 * Sample transform: x (S, Cin, H, W), proj (Cin, c) or NULL (then c == Cin), window (H, W), interp_y (Hf, 2), interp_x (Wh, 2) ->
 *   xf (S, c, Hf, Wh, 2), Hf = H + (H + 1) % 2, Wh = W / 2 + 1:
 *     y = (sum_ci x[., ci] proj[ci, k]) * window;  F[ky, kx] = sum_h sum_w y[h, w] exp(-2 pi i (ky h / H + kx w / W)), kx < Wh;
 *     row r of xf carries the frequency f = r - (Hf - 1) / 2, i.e. F[f mod H] -- for even H the Nyquist row appears at both ends, as
 *     rfftshift2 (fourier.py:8-10) leaves it;  xf = (F * interp_y[r]) * interp_x[kx];  with has_shift the two factors of shift_fs
 *     (fourier.py:78-92) follow: * exp(i shift_y f) * exp(i shift_x kx).
 *   window may be NULL (no window); interp_y and interp_x may be NULL together (no interpolation factors: the plain centred transform).
 *   A dense two-pass transform (rows, then columns); twiddle phases are reduced in integers, (k n) mod N, and the N cosine / sine values
 *   are evaluated in double precision.  In all these entry points the sums over channels, map rows / columns and series terms are
 *   accumulated in double-precision registers and rounded to fp32 once; everything in memory is fp32.
 * Shift: the two factors of shift_fs alone on xf (S, c, Hf, Wh, 2), odd Hf; out may not alias xf partially (out == xf is fine).
 * Filter response (eco.py:244-245): hf (1, c, Hf, Wh, 2), xf (S, c, Hf, Wh, 2) -> sf (S, 1, Hf, Wh, 2) = sum over k = 0 .. c - 1, in that
 *   order, of the complex products hf[k] * xf[s, k].
 * Localisation (eco.py:247-252, 272; fourier.py:34-61, 95-114): `sf`, `Hf`, `Wh`, `weight` are HOST arrays of nb <= PT_ECO_MAX_BLOCKS
 *   entries, the block with the largest series FIRST: device pointers to (S, 1, Hf[b], Wh[b], 2), odd Hf[b] <= Hf[0], Wh[b] <= Wh[0],
 *   and the translation weights (NULL: all 1, fusion 'sum').  A = weight[0] sf[0], and weight[b] sf[b] added at sum_fs's offsets (rows
 *   centred on the zero frequency, columns from 0).  The series is evaluated on the (Oh, Ow) grid, Oh >= Hf[0], Ow >= 2 Wh[0] - 1, even
 *   or odd, as the REAL PART OF THE HALF-SPECTRUM SERIES:
 *     scores[s, y, x] = Re sum_kx m_kx exp(2 pi i kx x / Ow) sum_r A[s, r, kx] exp(2 pi i (r - (Hf[0] - 1) / 2) y / Oh),  m_0 = 1, m_kx = 2:
 *   the kx = 0 column counts once, every kx > 0 column twice.  For Hermitian-consistent input this is what the inverse real transform of
 *   sample_fs returns after its zero padding (pad_top = (Oh - Hf) / 2 rounded down, the rest below; columns to Ow / 2 + 1) and its
 *   Oh Ow rescale; the imaginary part of the kx = 0 column is ignored here as it is there.  For a grid EQUAL to the series sample_fs
 *   passes no size to the inverse transform, which then returns 2 Wh - 2 columns: that case is defined here with Ow = 2 Wh - 1 and is
 *   not what the reference computes.  scores (S, 1, Oh, Ow); max_val (S) and argmax (S, 2) int64 [row, col] as the max2d entry above.
 * Memory insert (eco.py:223-230, 339-343): xf (1, c, Hf, Wh, 2), shifted when has_shift, stored transposed into slot `ind` of
 *   samples (Hf, Wh, n, c, 2); nothing outside the slot is written.
 * Covered: H, W <= PT_ECO_MAX_FEAT; Oh, Ow <= PT_ECO_MAX_GRID; Wh[0] <= 64.
 * Status: NULL pointer PT_ERR_NULL, a non-positive or inconsistent size PT_ERR_SHAPE, a size beyond the bounds above PT_ERR_UNSUPPORTED,
 * workspace too small or misaligned PT_ERR_WORKSPACE -- all before anything is queued.  The ws_bytes query is host-only and returns 0 for
 * what is not covered.
 * ---------------------------------------------------------------------------------------------- */
#define PT_ECO_MAX_FEAT 64
#define PT_ECO_MAX_GRID 1024
#define PT_ECO_MAX_BLOCKS 4
#define PT_ECO_MAX_SAMPLES 1024
/* Filter update, FilterOptim.run (pytracking/tracker/eco/optim.py:142-208) on run_CG (pytracking/libs/optimization.py:72-163): one call,
 * all feature blocks.  Per block: samples (Hf, Wh, n, c, 2), weights (n) ON THE DEVICE, yf (Hf, Wh), reg_filter (Rh, Rw), sample_energy
 * (c, Hf, Wh) in/out, new_xf (c, Hf, Wh, 2) or NULL, x (c, Hf, Wh, 2) updated IN PLACE, and the carried CG state the caller owns: p and
 * r_prev (c, Hf, Wh, 2) and state[2] = {rho, 1 if p is valid else 0} (zero-initialise state[1] before the first call).  Steps: the sample-energy
 * moving average (1 - lr) e + lr |new_xf|^2 when new_xf is given; b = yf conj(sum_n w_n S_n); diag_M = (1 - reg_param) (data_param e +
 * (1 - data_param) mean_c e) + reg_param reg_energy; r = b - A(x); num_iter iterations with M1 = 1 / diag_M, Polak-Ribiere or
 * Fletcher-Reeves beta clamped at 0, alpha = rho / ip(p, q) (standard_alpha) or ip(p, r) / ip(p, q), the residual update skipped on the
 * last iteration.  direction_forget_factor 0 resets the state, otherwise rho /= factor when p is valid.  ip is inner_prod_fs.  CG scalars
 * are per block; if any block's rho is exactly 0 at the top of an iteration the run ends for every block with x as it stands (a flag in
 * the workspace turns the remaining launches into no-ops; rho of that iteration is kept, as in the reference).  num_iter == 0 returns at
 * once.  A(v) = S^H diag(w) S v per bin plus the regulariser: v extended to the left by conj(flip(v[.., 1 : pad2 + 1, :])), convolved with
 * reg_filter at padding (pad1, pad2), min(pad2, Wh - 1) columns dropped, convolved again without padding; pad1 = min(Rh - 1, Hf - 1),
 * pad2 = min(Rw - 1, 2 Wh - 2).  A filter whose clipped padding does not give (Hf, Wh) back (the reference's conv2d raises there) is
 * PT_ERR_UNSUPPORTED.  Covered: c <= 64, n <= PT_ECO_MAX_SAMPLES, Rh, Rw <= 15, <= PT_ECO_MAX_BLOCKS blocks. */
typedef struct pt_eco_fu_block {
    const float *samples, *weights, *yf, *reg_filter;
    float* sample_energy;
    const float* new_xf;
    float *x, *p, *r_prev, *state;
    int Hf, Wh, c, n, Rh, Rw;
    float learning_rate, reg_energy;
} pt_eco_fu_block;
size_t pt_eco_filter_update_ws_bytes(const pt_eco_fu_block* blk, int nb);
int pt_eco_filter_update_f32(const pt_eco_fu_block* blk, int nb, int num_iter, int fletcher_reeves, int standard_alpha,
                             float direction_forget_factor, float precond_data_param, float precond_reg_param, void* ws, size_t ws_bytes,
                             void* stream);
/* First-frame joint optimisation of filter and projection matrix (eco.py:152-158): GaussNewtonCG.run (pytracking/libs/optimization.py:
 * 293-421) on FactorizedConvProblem (pytracking/tracker/eco/optim.py:8-118), one call, all feature blocks, num_gn_iter Gauss-Newton
 * iterations of num_cg_iter CG iterations each.  Per block: samples (Hf, Wh, n, Cin, 2) UNCOMPRESSED, weights_sqrt (nw = 1 or n) ON THE
 * DEVICE, yf (Hf, Wh), reg_filter (Rh, Rw), diag_M (c, Hf, Wh) and proj_precond (the problem constructor's preconditioner: inputs, not
 * recomputed), hf (c, Hf, Wh, 2) and proj (Cin, c) updated IN PLACE.  Residuals: sw_s (x[k,s]^T P h[k] - yf[k]); one correlation of
 * [conj(flip(h[.., 1 : pad2 + 1, :])), h] with reg_filter at padding (pad1, pad2) = (min(Rh - 1, Hf - 1), min(Rw - 1, Wh - 1)), the left
 * extension counted in the residual but not in the Jacobian (the reference detaches it); sqrt(projection_reg) P.  Each Gauss-Newton
 * iteration solves J^T J d = -J^T f0 by run_CG from d = 0: Fletcher-Reeves beta clamped at 0, alpha = rho / ip(p, q), M1 = 1 / diag_M on the
 * filter and 1 / proj_precond on the projection, p and rho reset, the residual update skipped on the last iteration; ip is ONE scalar per
 * block, inner_prod_fs of the filter parts plus the dot product of the projection parts, so alpha and beta are per block.  If any block's
 * rho is exactly 0 at the top of a CG iteration, that Gauss-Newton iteration's CG run ends for every block, the step accumulated so far
 * (none in the first iteration, where the reference raises) is added and the next Gauss-Newton iteration goes on; a flag in the workspace
 * turns the remaining launches of the run into no-ops.  Zero Gauss-Newton or CG iterations return PT_OK and touch nothing.
 * Covered: Cin <= 512, c <= 64, n <= 64, Rh, Rw <= 15, <= PT_ECO_MAX_BLOCKS blocks, num_cg_iter <= 62, num_gn_iter <= 32. */
typedef struct pt_eco_init_block {
    const float *samples, *weights_sqrt, *yf, *reg_filter, *diag_M;
    float *hf, *proj;            /* in/out */
    int Hf, Wh, Cin, c, n, nw /* 1 or n */, Rh, Rw;
    float proj_precond;
} pt_eco_init_block;
size_t pt_eco_joint_init_ws_bytes(const pt_eco_init_block* blk, int nb);
int pt_eco_joint_init_f32(const pt_eco_init_block* blk, int nb, int num_gn_iter, int num_cg_iter, float projection_reg, void* ws,
                          size_t ws_bytes, void* stream);
int pt_eco_sample_f32(const float* x, const float* proj, const float* window, const float* interp_y, const float* interp_x, int has_shift,
                      float shift_y, float shift_x, float* xf, int S, int Cin, int c, int H, int W, void* stream);
int pt_eco_shift_f32(const float* xf, float shift_y, float shift_x, float* out, int S, int c, int Hf, int Wh, void* stream);
int pt_eco_apply_filter_f32(const float* hf, const float* xf, float* sf, int S, int c, int Hf, int Wh, void* stream);
size_t pt_eco_localize_ws_bytes(int S, int Wh, int Oh, int Ow);
int pt_eco_localize_f32(const float* const* sf, const int* Hf, const int* Wh, const float* weight, int nb, int S, int Oh, int Ow, float* scores,
                        float* max_val, long long* argmax, void* ws, size_t ws_bytes, void* stream);
int pt_eco_insert_f32(const float* xf, int has_shift, float shift_y, float shift_x, float* samples, int c, int Hf, int Wh, int n, int ind,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PT_HOT_H */
