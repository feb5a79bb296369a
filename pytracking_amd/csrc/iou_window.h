// The pixel window of a target box on one backbone level: the pixels Precise RoI Pooling (prroi_dev.h: make_bin) can read for the RoI
// (x, y, x + w, y + h) at spatial scale s on an H x W map,
//     columns  max(0, floor(x0 * s)) ... min(W - 1, ceil(x1 * s)),   rows likewise,
// the union of what make_bin clamps to over all bins of any pooled size.  Shared by the windowed convolution and the pooling kernel of
// iou_mod.hip and by the host-only export pt_iou_mod_window: ONE definition, in the fp32 arithmetic of make_bin (x1 = x + w first, as
// AtomIoUNet.get_modulation forms the RoI, then the scale).  The box only ever enters comparisons and clamped integers.
#pragma once

struct PtIouWin { int x0, y0, x1, y1; };          // inclusive; empty where x1 < x0 or y1 < y0

// floor / ceil of a scaled coordinate as an int; beyond +-2^29 it is clipped there (any map is smaller) and a NaN becomes -2^29
__host__ __device__ inline int pt_iou_win_int(float v) {
    const float lim = 536870912.f;
    v = v >= -lim ? v : -lim;                     // NaN fails the comparison
    v = v <= lim ? v : lim;
    return (int)v;
}

__host__ __device__ inline PtIouWin pt_iou_window(const float* bb, float s, int H, int W) {
    const float X0 = bb[0] * s, Y0 = bb[1] * s, X1 = (bb[0] + bb[2]) * s, Y1 = (bb[1] + bb[3]) * s;
    PtIouWin w;
    const int fx = pt_iou_win_int(floorf(X0)), fy = pt_iou_win_int(floorf(Y0));
    const int cx = pt_iou_win_int(ceilf(X1)), cy = pt_iou_win_int(ceilf(Y1));
    w.x0 = fx > 0 ? fx : 0;
    w.y0 = fy > 0 ? fy : 0;
    w.x1 = cx < W - 1 ? cx : W - 1;
    w.y1 = cy < H - 1 ? cy : H - 1;
    return w;
}

__host__ __device__ inline bool pt_iou_win_empty(const PtIouWin& w) { return w.x1 < w.x0 || w.y1 < w.y0; }
