// Token / padding helpers of the per-tap split-K GEMM route of a 3x3 convolution on (n, C, H, W) maps (launch_gemm(..., conv = true) of
// mfma_gemm.h wants a K-contiguous operand with Cin % 64 == 0): shared by iou_feat.hip and lwl_decoder.hip.
// Header-only (anonymous namespace): each translation unit gets its own instantiations.
#pragma once
#include "common.h"

namespace {

// GEMM route: (n, C, HW) -> tokens X[(img * HW + p) * Cpad + c], channels C .. Cpad - 1 zero.  grid (ceil(HW/32), Cpad/32, n)
__global__ __launch_bounds__(256) void k_iou_tokens(const float* __restrict__ in, float* __restrict__ X, int C, int Cpad, int HW) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, img = blockIdx.z;
    const float* src = in + (long)img * C * HW;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        tile[ty + 8 * i][tx] = (c < C && p < HW) ? src[(long)c * HW + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        if (p < HW && c < Cpad) X[((long)img * HW + p) * Cpad + c] = tile[tx][ty + 8 * i];
    }
}

// GEMM route, Cin % 64 != 0: tap-major weights (rows = Cout * 9, Cin) -> (rows, Cpad), zero padded
__global__ __launch_bounds__(256) void k_iou_padw(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cpad, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / Cpad;
    const int c = (int)(i - row * Cpad);
    wp[i] = c < Cin ? w[row * Cin + c] : 0.f;
}

}  // namespace
