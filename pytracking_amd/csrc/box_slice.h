// The box-to-mask rule of the LWL / RTS box label encoders (ltr/models/lwl/label_encoder.py:83-92 and :163-172, the same code under
// ltr/models/rts): mask[y1 : y1 + h, x1 : x1 + w] = 1 with Python's slice semantics, shared by the stem that rasterises the box into its
// LDS tile (label_enc.hip), the resized-mask kernel (box_enc.hip) and the host-only export pt_box_slice.  The box only ever enters
// comparisons, never an address.
#pragma once

// int(int(v) + 0.5) of the reference: truncation toward zero, then -- for a negative integer k -- int(k + 0.5) = k + 1.  Values beyond
// +-2^29 are clipped there (any map is shorter, so the slice is the same) and a NaN becomes -2^29; the reference raises on either.
__host__ __device__ inline int pt_box_int(float v) {
    const float lim = 536870912.f;
    v = v >= -lim ? v : -lim;                    // NaN fails the comparison
    v = v <= lim ? v : lim;
    const int k = (int)v;
    return k < 0 ? k + 1 : k;
}

// range(len)[a : b] with a = start (max(0, start) with `clamp_start`) and b = start + extent -> [lo, hi), hi <= lo where it is empty.
// A negative bound counts from the end (len + v) and every bound is clipped to [0, len].  |start|, |extent| <= 2^29.
__host__ __device__ inline void pt_box_slice_rule(int start, int extent, int len, bool clamp_start, int* lo, int* hi) {
    int a = clamp_start && start < 0 ? 0 : start, b = start + extent;
    a = a < 0 ? a + len : a;
    b = b < 0 ? b + len : b;
    a = a < 0 ? 0 : (a > len ? len : a);
    b = b < 0 ? 0 : (b > len ? len : b);
    *lo = a;
    *hi = b;
}

// The rows [y0, y1) and columns [x0, x1) a box (x, y, w, h) sets in an H x W mask.
struct PtBoxRect { int x0, x1, y0, y1; };
__host__ __device__ inline PtBoxRect pt_box_rect(const float* bb, int H, int W, bool clamp_start) {
    PtBoxRect r;
    pt_box_slice_rule(pt_box_int(bb[0]), pt_box_int(bb[2]), W, clamp_start, &r.x0, &r.x1);
    pt_box_slice_rule(pt_box_int(bb[1]), pt_box_int(bb[3]), H, clamp_start, &r.y0, &r.y1);
    return r;
}
