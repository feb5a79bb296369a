// libpt_loc: ATOM's per-frame score localisation on the device (include/pt_loc.h).
//   ATOM.localize_target      pytracking/tracker/atom/atom.py:304-339
//   ATOM.localize_advanced    atom.py:341-406
//   fourier.cfft2 / shift_fs / sample_fs   pytracking/libs/fourier.py:20-24, 35-61, 78-92
// The reference transforms the (S, 1, N_h, N_w) scores with a real FFT, shifts the phases, zero-pads the spectrum to the output grid,
// transforms back, multiplies by the window, rolls the map with four torch.cat and takes two max2d with about ten .item() / .cpu() round
// trips.  All of it up to the arg-max is linear and separable in the real input:
//     out = A_y . (weight * s) . A_x^T,   A[y, m] = (1 + 2 sum_{k=1..N/2} cos(pi k r / (N G))) / N,  r = (N G - p G + 2 y N - 2 m G) mod 2 N G
// (N: series side, G: grid side, p: kernel side % 2; the k = N/2 term of an even N keeps the weight 2: `rfftshift2` puts the Nyquist row at
// both ends and the zero-padded `irfft` counts the Nyquist column with its conjugate).  k_loc_interp evaluates that by definition: r is reduced
// in integers, cos(pi r / (N G)) comes from cospi in double, the k-th harmonic from the Chebyshev recurrence, every sum runs in double in a
// fixed order and is rounded to float32 once.  The window multiply that follows is the reference's float32 product.
//
// Launch 1 (k_loc_interp), grid (ceil(G_h / 8), S): a workgroup owns 8 rows of the OUTPUT map of one scale -- already rolled by
// (G + 1) // 2 when the advanced branch is on -- and leaves the band's peak (max2d's tie order, localize_dev.h) in the workspace.
// Launch 2 (k_loc_decide), one workgroup: the first peak over bands, then scales (torch.max's first index), the masked second peak of the
// chosen scale, every branch of atom.py:366-406 or the plain branch of :321-331, and the record whose sequence word the host polls.
//
// Arithmetic types follow what the reference's expressions evaluate to under torch, as in csrc/localize.hip and csrc_mot/mot_readout.hip:
// `tensor.item() < python float` compares doubles, `python float * float32 tensor` and `float32 tensor > python float` are float32
// operations with the scalar rounded to float32 first, Python's round() on doubles is rint.  Every product, quotient and sum of the
// decision is rounded on its own (__fmul_rn / __fadd_rn ...): no FMA contraction.
#include <chrono>
#include <math.h>
#include "../csrc/pt_internal.h"
#include "../csrc/localize_dev.h"
#include "../../include/pt_loc.h"

static_assert(PT_AL_NORMAL == PT_LOC_NORMAL && PT_AL_HARD_NEGATIVE == PT_LOC_HARD_NEGATIVE && PT_AL_UNCERTAIN == PT_LOC_UNCERTAIN &&
              PT_AL_NOT_FOUND == PT_LOC_NOT_FOUND, "the flags of the libraries are one set");

#define PT_AL_CHECK_LAUNCH()                                          \
    do {                                                              \
        if (hipGetLastError() != hipSuccess) return PT_AL_ERR_LAUNCH; \
    } while (0)

namespace {

constexpr int ROWS = PT_AL_BAND_ROWS, NMAX = PT_AL_MAX_SERIES;
constexpr int DECIDE_THREADS = 1024;

struct BandPeak { float v; int r, c, pad; };          // 16 bytes per (scale, band)

struct LocArgs {
    const float *scores, *window;
    float *map_out, *map_hn, *rec;
    BandPeak* part;
    int S, Nh, Nw, Gh, Gw, nbands;
    float seq;
    pt_loc_atom_params p;
};

// A[y, m] of the header: sample y of the shifted, zero-padded series of one-hot m.  All integers stay below 2^21: N G <= 18432.
__device__ __forceinline__ double interp_weight(int N, int G, int p, int y, int m) {
    const int NG = N * G, two = 2 * NG;
    int num = (NG - p * G + 2 * y * N - 2 * m * G) % two;
    if (num < 0) num += two;
    const double c1 = cospi((double)num / (double)NG);
    double prev = 1.0, cur = c1, sum = 0.0;           // cos(k theta), k = 0, 1: Chebyshev recurrence for the higher harmonics
    for (int k = 1; k <= N / 2; ++k) {
        sum += cur;
        const double next = 2.0 * c1 * cur - prev;
        prev = cur;
        cur = next;
    }
    return (1.0 + 2.0 * sum) / (double)N;
}

__global__ __launch_bounds__(256) void k_loc_interp(LocArgs a) {
    __shared__ double s_in[NMAX * NMAX];
    __shared__ double Ay[ROWS][NMAX];
    __shared__ double T[ROWS][NMAX];
    __shared__ Peak sh[4];
    const int band = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int Nh = a.Nh, Nw = a.Nw, Gh = a.Gh, Gw = a.Gw;
    const bool adv = a.p.advanced != 0;
    const int roll_h = adv ? (Gh + 1) / 2 : 0, roll_w = adv ? (Gw + 1) / 2 : 0;

    const float* src = a.scores + (long)s * Nh * Nw;
    for (int i = tid; i < Nh * Nw; i += 256) s_in[i] = (double)__fmul_rn(a.p.weight, src[i]);          // atom.py:307
    {
        const int yb = tid / NMAX, m = tid % NMAX, row = band * ROWS + yb;
        if (m < Nh && row < Gh) Ay[yb][m] = interp_weight(Nh, Gh, a.p.parity[0], (row + roll_h) % Gh, m);
    }
    __syncthreads();
    {
        const int yb = tid / NMAX, n = tid % NMAX, row = band * ROWS + yb;
        if (n < Nw && row < Gh) {
            double t = 0.0;
            for (int m = 0; m < Nh; ++m) t += Ay[yb][m] * s_in[m * Nw + n];
            T[yb][n] = t;
        }
    }
    __syncthreads();

    const bool win_first = a.p.windowed && (adv || !a.p.hn);
    const bool two_maps = adv && a.p.hn;
    Peak best{-INFINITY, Gh, Gw};
    const long plane = (long)s * Gh * Gw;
    for (int col = tid; col < Gw; col += 256) {
        const int x = (col + roll_w) % Gw;
        double ax[NMAX];
#pragma unroll
        for (int n = 0; n < NMAX; ++n) ax[n] = n < Nw ? interp_weight(Nw, Gw, a.p.parity[1], x, n) : 0.0;
        for (int yb = 0; yb < ROWS; ++yb) {
            const int row = band * ROWS + yb;
            if (row >= Gh) break;
            double v = 0.0;
#pragma unroll
            for (int n = 0; n < NMAX; ++n)
                if (n < Nw) v += T[yb][n] * ax[n];
            const float f = (float)v;                                       // the one rounding
            float first = f;
            if (win_first) first = __fmul_rn(f, a.window[(long)((row + roll_h) % Gh) * Gw + x]);       // atom.py:316 / :352, un-rolled window
            a.map_out[plane + (long)row * Gw + col] = first;
            if (two_maps) a.map_hn[plane + (long)row * Gw + col] = f;
            const Peak p{first, row, col};
            if (better(p, best)) best = p;
        }
    }
    best = block_peak(best, sh);
    if (tid == 0) a.part[s * a.nbands + band] = BandPeak{best.v, best.r, best.c, 0};
}

__device__ __forceinline__ float disp_norm(float dr, float dc) {           // torch.sqrt(torch.sum(target_disp ** 2))
    return __fsqrt_rn(__fadd_rn(__fmul_rn(dr, dr), __fmul_rn(dc, dc)));
}

__global__ __launch_bounds__(DECIDE_THREADS) void k_loc_decide(LocArgs a) {
    __shared__ Peak sh[DECIDE_THREADS / 64];
    const pt_loc_atom_params& q = a.p;
    const int Gh = a.Gh, Gw = a.Gw, tid = threadIdx.x;
    // first peak: dcf.max2d per scale over the bands, then torch.max over the scales (first index on a tie)
    Peak p1{-INFINITY, Gh, Gw};
    int s1 = 0;
    for (int s = 0; s < a.S; ++s) {
        Peak p{-INFINITY, Gh, Gw};
        if (tid < a.nbands) {
            const BandPeak b = a.part[s * a.nbands + tid];
            p = Peak{b.v, b.r, b.c};
        }
        p = block_peak(p, sh);
        if (s == 0 || p.v > p1.v) { p1 = p; s1 = s; }
    }
    const bool adv = q.advanced != 0;
    int code = PT_AL_NORMAL, pick = 1, which = 0;
    Peak p2{0.f, 0, 0};
    bool second = false;
    if (adv) {
        if ((double)p1.v < q.target_not_found_threshold) code = PT_AL_NOT_FOUND;                         // atom.py:366
        else second = true;
    }
    if (second) {                                                         // the same in every thread: p1 is
        which = q.hn ? 1 : 0;
        const float* map = (q.hn ? a.map_hn : a.map_out) + (long)s1 * Gh * Gw;
        const double nr = (double)q.neigh[0], nc = (double)q.neigh[1];
        const int top = max((int)rint((double)p1.r - nr / 2), 0);
        const int bottom = min((int)rint((double)p1.r + nr / 2 + 1), Gh);
        const int left = max((int)rint((double)p1.c - nc / 2), 0);
        const int right = min((int)rint((double)p1.c + nc / 2 + 1), Gw);
        p2 = block_peak(scan_map(map, Gh, Gw, top, bottom, left, right), sh);
    }
    if (tid != 0) return;

    float tv[2];
    if (!adv) {
        // disp = (max_disp + output_sz / 2) % output_sz - output_sz / 2, then * (img_support_sz / output_sz) * target_scale * scale_factors
        const float d[2] = {(float)p1.r, (float)p1.c}, g[2] = {(float)Gh, (float)Gw};
        for (int k = 0; k < 2; ++k) {
            const float disp = __fsub_rn(fmodf(__fadd_rn(d[k], q.half[k]), g[k]), q.half[k]);
            tv[k] = __fmul_rn(__fmul_rn(__fmul_rn(disp, q.ratio[k]), q.target_scale), q.scale_factors[s1]);
        }
    } else {
        const float d1r = __fsub_rn((float)p1.r, q.center[0]), d1c = __fsub_rn((float)p1.c, q.center[1]);
        const float d2r = __fsub_rn((float)p2.r, q.center[0]), d2c = __fsub_rn((float)p2.c, q.center[1]);
        if (second) {
            if (p2.v > __fmul_rn(q.distractor_threshold, p1.v)) {                                       // atom.py:388-401
                const float n1 = disp_norm(d1r, d1c), n2 = disp_norm(d2r, d2c);
                const bool far1 = n1 > q.disp_threshold, near1 = n1 < q.disp_threshold;
                const bool far2 = n2 > q.disp_threshold, near2 = n2 < q.disp_threshold;
                if (far2 && near1) code = PT_AL_HARD_NEGATIVE;
                else if (near2 && far1) { code = PT_AL_HARD_NEGATIVE; pick = 2; }
                else code = PT_AL_UNCERTAIN;
            } else if (p2.v > __fmul_rn(q.hard_negative_threshold, p1.v) && p2.v > q.target_not_found_f32) {   // atom.py:403
                code = PT_AL_HARD_NEGATIVE;
            }
        }
        const float dr = pick == 1 ? d1r : d2r, dc = pick == 1 ? d1c : d2c;
        tv[0] = __fmul_rn(__fmul_rn(dr, q.ratio[0]), q.target_scale);
        tv[1] = __fmul_rn(__fmul_rn(dc, q.ratio[1]), q.target_scale);
    }
    float* o = a.rec;
    o[PT_AL_R_FLAG] = (float)code; o[PT_AL_R_SCALE] = (float)s1;
    o[PT_AL_R_ROW1] = (float)p1.r; o[PT_AL_R_COL1] = (float)p1.c; o[PT_AL_R_MAX1] = p1.v;
    o[PT_AL_R_ROW2] = (float)p2.r; o[PT_AL_R_COL2] = (float)p2.c; o[PT_AL_R_MAX2] = p2.v;
    o[PT_AL_R_TV] = tv[0]; o[PT_AL_R_TV + 1] = tv[1];
    o[PT_AL_R_PICK] = (float)pick; o[PT_AL_R_WHICH] = (float)which;
    for (int k = PT_AL_R_WHICH + 1; k < PT_AL_R_SEQ; ++k) o[k] = 0.f;
    __threadfence_system();                                              // the record is visible before its sequence word
    __hip_atomic_store(o + PT_AL_R_SEQ, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

bool covered_shape(int S, int Nh, int Nw, int Gh, int Gw) {
    if (S < 1 || S > PT_AL_MAX_SCALES) return false;
    const int N[2] = {Nh, Nw}, G[2] = {Gh, Gw};
    for (int d = 0; d < 2; ++d)
        if (N[d] < PT_AL_MIN_SERIES || N[d] > PT_AL_MAX_SERIES || G[d] > PT_AL_MAX_GRID || G[d] <= 2 * (N[d] / 2) + 1) return false;
    return true;
}

int bands_of(int Gh) { return (Gh + ROWS - 1) / ROWS; }

}  // namespace

extern "C" const char* pt_loc_strerror(int status) {
    switch (status) {
        case PT_AL_OK: return "ok";
        case PT_AL_ERR_NULL: return "required pointer is NULL";
        case PT_AL_ERR_SHAPE: return "non-positive or inconsistent dimension";
        case PT_AL_ERR_UNSUPPORTED: return "unsupported: configuration not covered by the gfx950 localisation";
        case PT_AL_ERR_WORKSPACE: return "workspace too small or misaligned";
        case PT_AL_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown status";
    }
}

extern "C" int pt_loc_abi_version(void) { return 1; }

// Every product / quotient below is a float32 operation in the reference (float32 CPU tensors; Python scalars are rounded to float32 by
// torch's binary ops), so plain `float` arithmetic with contraction off reproduces the values bit for bit.
#pragma clang fp contract(off)
extern "C" int pt_loc_atom_constants_f32(const pt_loc_atom_state* st, pt_loc_atom_params* q) {
    if (!st || !q) return PT_AL_ERR_NULL;
    for (int d = 0; d < 2; ++d)
        if (!(st->output_sz[d] >= 1.f) || !(st->img_support_sz[d] > 0.f) || st->kernel_size[d] < 1) return PT_AL_ERR_SHAPE;
    if (!(st->target_scale > 0)) return PT_AL_ERR_SHAPE;
    *q = pt_loc_atom_params{};
    q->target_not_found_threshold = st->target_not_found_threshold;
    q->distractor_threshold = (float)st->distractor_threshold;
    q->hard_negative_threshold = (float)st->hard_negative_threshold;
    q->target_not_found_f32 = (float)st->target_not_found_threshold;
    q->disp_threshold = (float)(st->dispalcement_scale * sqrt((double)st->output_sz[0] * (double)st->output_sz[1]) / 2);   // atom.py:391
    const float ts = (float)st->target_scale, tns = (float)st->target_neighborhood_scale;
    for (int d = 0; d < 2; ++d) {
        q->ratio[d] = st->img_support_sz[d] / st->output_sz[d];           // atom.py:330, :364
        q->half[d] = st->output_sz[d] / 2.0f;                             // atom.py:327
        q->center[d] = floorf(st->output_sz[d] / 2.0f);                   // output_sz // 2, atom.py:363
        q->neigh[d] = (tns * st->target_sz[d]) / ts;                      // atom.py:373
        q->parity[d] = st->kernel_size[d] % 2;                            // atom.py:310
    }
    q->target_scale = ts;
    q->weight = (float)st->translation_weight;
    for (int k = 0; k < PT_AL_MAX_SCALES; ++k) q->scale_factors[k] = st->scale_factors[k];
    q->advanced = st->advanced_localization != 0;
    q->windowed = st->windowed != 0;
    q->hn = q->windowed && st->hn_without_windowing != 0;
    return PT_AL_OK;
}

extern "C" size_t pt_loc_atom_ws_bytes(int S, int Nh, int Nw, int Gh, int Gw) {
    if (!covered_shape(S, Nh, Nw, Gh, Gw)) return 0;
    return ((size_t)S * bands_of(Gh) * sizeof(BandPeak) + 255) & ~(size_t)255;
}

extern "C" int pt_loc_atom_f32(const float* scores, int S, int Nh, int Nw, int Gh, int Gw, const float* window, const pt_loc_atom_params* prm,
                               float* map_out, float* map_hn_out, float* rec, float seq, void* ws, size_t ws_bytes, void* stream) {
    if (!scores || !prm || !map_out || !rec || !ws) return PT_AL_ERR_NULL;
    if (Nh <= 0 || Nw <= 0 || Gh <= 0 || Gw <= 0) return PT_AL_ERR_SHAPE;
    if (!covered_shape(S, Nh, Nw, Gh, Gw)) return PT_AL_ERR_UNSUPPORTED;
    if (prm->windowed && !window) return PT_AL_ERR_NULL;
    if (prm->advanced && prm->hn && !map_hn_out) return PT_AL_ERR_NULL;
    if (prm->hn && !prm->windowed) return PT_AL_ERR_SHAPE;
    if ((prm->parity[0] | prm->parity[1]) & ~1) return PT_AL_ERR_SHAPE;
    if (ws_bytes < pt_loc_atom_ws_bytes(S, Nh, Nw, Gh, Gw) || ((uintptr_t)ws & 255)) return PT_AL_ERR_WORKSPACE;
    LocArgs a{};
    a.scores = scores; a.window = window; a.map_out = map_out; a.map_hn = map_hn_out; a.rec = rec;
    a.part = (BandPeak*)ws;
    a.S = S; a.Nh = Nh; a.Nw = Nw; a.Gh = Gh; a.Gw = Gw; a.nbands = bands_of(Gh);
    a.seq = seq;
    a.p = *prm;
    hipLaunchKernelGGL(k_loc_interp, dim3(a.nbands, S), dim3(256), 0, (hipStream_t)stream, a);
    PT_AL_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_loc_decide, dim3(1), dim3(DECIDE_THREADS), 0, (hipStream_t)stream, a);
    PT_AL_CHECK_LAUNCH();
    return PT_AL_OK;
}

extern "C" int pt_loc_atom_wait_f32(const float* rec_host, float seq, void* stream) {
    if (!rec_host) return PT_AL_ERR_NULL;
    const volatile float* word = rec_host + PT_AL_R_SEQ;
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n((const volatile int*)word, __ATOMIC_ACQUIRE) != __builtin_bit_cast(int, seq)) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return PT_AL_ERR_LAUNCH;
            break;
        }
    }
    return PT_AL_OK;
}
