/*
 * pt_bbn.h -- C ABI of libpt_bbn.so: the forward pass of the trackers' ResNet backbones on AMD Instinct MI355X (gfx950), i.e.
 * `ResNet.forward(x, output_layers)` of ltr/models/backbone/resnet.py (ResNet-18 / -50 / -101, `resnet_baby`) and of
 * ltr/models/backbone/resnet_mrcnn.py (the LWL / RTS ResNet-50) in eval mode: the 7x7 stem, the 3/2/1 max-pool and the residual blocks up to
 * the deepest requested layer, every BatchNorm folded into a per-channel (scale, shift) behind its convolution.
 *
 * One convolution family.  Every convolution is an implicit GEMM over tokens on v_mfma_f32_16x16x4_f32 (exact fp32): M = n * Ho * Wo output
 * pixels of ALL images of the call in one token range, N = Cout, K = k * k * Cin (tap-major, input channel innermost), kernel 1x1 or 3x3 at
 * stride 1 or 2 (k_conv), and the 7x7 stride-2 stem read straight from the NCHW input (the same kernel with its stem loader).  The epilogue
 * computes fma(acc, scale[co], shift[co]), adds the residual where the block has one, applies ReLU where the network does, writes the next
 * layer's operand (tokens x channels) and, for a requested output layer, the NCHW map.  The max-pool is a launch of its own (k_pool); its
 * input is post-ReLU, so its padding is 0 instead of -inf: the same maximum.
 *
 * Launch filling.  pt_bbn_plan picks per convolution the largest row tile of {128, 64, 32} x 64 columns that still gives
 * PT_BBN_FILL_WGS workgroups, else the 32-row tile; with the 32-row tile it doubles a K-split (2, 4, 8) while the doubled launch does not
 * exceed PT_BBN_FILL_WGS workgroups and every split keeps at least PT_BBN_MIN_KSTEPS K-steps of 32.  A split convolution writes its partial sums
 * to the workspace and k_reduce adds them in the order z = 0, 1, ... and applies the epilogue.
 *
 * Between layers the activations are tokens x channels (NHWC) in the workspace; the boundary is NCHW in, NCHW out.
 *
 * Limits (PT_BBN_ERR_UNSUPPORTED, nothing queued): `inplanes` a multiple of 8 in 8..PT_BBN_MAX_INPLANES; 1..PT_BBN_MAX_BLOCKS blocks per
 * layer; strides 1 or 2; dilation 1 only (a desc cannot state another); basic blocks carry the stride on conv1; n, H, W such that the
 * input, every activation, every weight matrix, every split's partial sums and every output stay below PT_BBN_MAX_VIEW_BYTES (the kernels
 * address each of them with 32-bit byte offsets); at least one pixel per map (n, H, W >= 1: PT_BBN_ERR_SHAPE otherwise).
 *
 * A fifth library next to libpt_hot.so, libpt_mot.so, libpt_loc.so and libpt_mem.so, with the same conventions:
 *   - all tensors are contiguous float32 device memory; `stream` is a hipStream_t (void*), NULL = default;
 *   - every function returns PT_BBN_OK (0) (pt_bbn_plan: the number of launches) or a negative pt_bbn_status; nothing is queued when an
 *     argument check fails;
 *   - caller-owned buffers, no allocation, no atomics, no host synchronisation, every sum in a fixed order: repeated calls give the same
 *     bits and the call can be captured in a graph.
 */
#ifndef PT_BBN_H
#define PT_BBN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pt_bbn_status {
    PT_BBN_OK = 0,
    PT_BBN_ERR_NULL = -1,        /* required pointer is NULL */
    PT_BBN_ERR_SHAPE = -2,       /* non-positive dimension, empty or unknown output mask */
    PT_BBN_ERR_UNSUPPORTED = -3, /* valid request outside the limits above */
    PT_BBN_ERR_WORKSPACE = -4,   /* workspace too small or misaligned */
    PT_BBN_ERR_LAUNCH = -5       /* hipGetLastError() != hipSuccess after a launch */
} pt_bbn_status;

const char* pt_bbn_strerror(int status);
int pt_bbn_abi_version(void);

#define PT_BBN_MAX_INPLANES 256
#define PT_BBN_MAX_BLOCKS 48          /* per layer */
#define PT_BBN_MAX_LAUNCHES 768       /* rows pt_bbn_plan may return */
#define PT_BBN_MAX_VIEW_BYTES 0x7FFFFF00
#define PT_BBN_FILL_WGS 256           /* the workgroup count a launch is planned to reach: one per CU */
#define PT_BBN_MIN_KSTEPS 4           /* K-steps of 32 every K-split keeps */
#define PT_BBN_STEM_K 160             /* the stem's K = 3 * 7 * 7 = 147 padded with zero weights to whole K-steps */

enum { PT_BBN_BASIC = 0, PT_BBN_BOTTLENECK = 1 };

/* bits of out_mask, entries of outs[] */
enum { PT_BBN_OUT_CONV1 = 0, PT_BBN_OUT_LAYER1 = 1, PT_BBN_OUT_LAYER2 = 2, PT_BBN_OUT_LAYER3 = 3, PT_BBN_OUT_LAYER4 = 4, PT_BBN_OUT_COUNT = 5 };

/* the kernels */
enum { PT_BBN_K_CONV = 0, PT_BBN_K_STEM = 1, PT_BBN_K_POOL = 2, PT_BBN_K_REDUCE = 3 };

/* the routes: (kernel, row tile, K-split) */
enum {
    PT_BBN_R_STEM = 0,           /* k_conv<64, stem loader> */
    PT_BBN_R_POOL = 1,
    PT_BBN_R_T128 = 2,           /* k_conv<128>, no split */
    PT_BBN_R_T64 = 3,
    PT_BBN_R_T32 = 4,
    PT_BBN_R_T32_S2 = 5,         /* k_conv<32>, grid.z = 2, partial sums */
    PT_BBN_R_T32_S4 = 6,
    PT_BBN_R_T32_S8 = 7,
    PT_BBN_R_REDUCE = 8,         /* k_reduce behind a split convolution */
    PT_BBN_R_COUNT = 9
};

/* The network.  resnet.py: stride_conv = 2 for bottlenecks (the 3x3), conv1_after_pool = 0; resnet_mrcnn.py: stride_conv = 1 (the first
 * 1x1), conv1_after_pool = 1.  The first block of a layer has a downsample (1x1 convolution of the layer's stride + BatchNorm) exactly when
 * its stride is not 1 or its channel count changes, as both files build it for dilation 1. */
typedef struct {
    int block;                   /* PT_BBN_BASIC / PT_BBN_BOTTLENECK */
    int inplanes;
    int blocks[4];               /* blocks of layer1..layer4 */
    int stride[4];               /* stride of the first block of layer1..layer4 */
    int stride_conv;             /* which convolution of that block carries it: 1 = conv1, 2 = conv2 */
    int conv1_after_pool;        /* the `conv1` output is the map behind the max-pool */
} pt_bbn_desc;

/* One launch of a call, as pt_bbn_plan reports it. */
typedef struct {
    int kernel;                  /* PT_BBN_K_* */
    int route;                   /* PT_BBN_R_* */
    int layer, block, conv;      /* layer 0 = stem / pool; conv 1..3, 0 = the downsample */
    int bm, split, ksteps;       /* row tile, K-split, K-steps per split (0 for pool / reduce) */
    int grid_x, grid_y, grid_z;
    int M, N, K;
    int Hin, Win, Hout, Wout, ksize, stride;
    int residual, relu, out;     /* out: the PT_BBN_OUT_* entry this launch writes as NCHW, -1 none */
} pt_bbn_launch;

/* Floats of the weight pack: per convolution, in the order stem, then per layer and block conv1, conv2, (conv3,) (downsample): the weights
 * (Cout, K) tap-major with the input channel innermost (the stem: (Cout, PT_BBN_STEM_K), K index c * 49 + ky * 7 + kx, zero behind 147),
 * then scale (Cout), then shift (Cout).  0 for a desc outside the limits. */
size_t pt_bbn_pack_floats(const pt_bbn_desc* desc);

/* Bytes of workspace of a call; 0 for a call pt_bbn_forward_f32 refuses. */
size_t pt_bbn_ws_bytes(const pt_bbn_desc* desc, int n, int H, int W, int out_mask);

/* Host only: the launches of the call in order -> their number, or a negative status.  rows: PT_BBN_MAX_LAUNCHES entries, or NULL. */
int pt_bbn_plan(const pt_bbn_desc* desc, int n, int H, int W, int out_mask, pt_bbn_launch* rows);

/* x (n, 3, H, W) -> outs[i] (n, C_i, H_i, W_i) for every bit i of out_mask (the other entries are not read); nothing behind the deepest
 * requested layer is computed.  pack: pt_bbn_pack_floats floats, 16-byte aligned; ws: 256-byte aligned, pt_bbn_ws_bytes bytes.  No output
 * may overlap x, the pack, the workspace or another output. */
int pt_bbn_forward_f32(const pt_bbn_desc* desc, const float* pack, const float* x, int n, int H, int W, int out_mask, float* const outs[5],
                       void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PT_BBN_H */
