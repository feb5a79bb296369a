/*
 * pt_loc.h -- C ABI of libpt_loc.so: the per-frame score localisation of the ATOM tracker on AMD Instinct MI355X (gfx950), i.e.
 * `ATOM.localize_target` and `ATOM.localize_advanced` (pytracking/tracker/atom/atom.py:304-406): the Fourier interpolation of the raw
 * classification scores onto the output grid, the optional output window, both peaks and the outcome, in two launches and one host wait.
 *
 * The chain cfft2 / (N_h N_w) -> shift_fs -> sample_fs(output_sz) is linear and separable in the real input:
 *     out = A_y . (weight * s) . A_x^T,   A[y, m] = (1 + 2 sum_{k=1..N/2} cos(pi k r / (N G))) / N,
 *     r = (N G - p G + 2 y N - 2 m G) mod 2 N G,   N: series side, G: grid side, p: kernel side % 2
 * so no complex intermediate and no padded spectrum exists.  The k = N/2 term of an even N carries the weight 2 of every other term: the
 * reference's `rfftshift2` puts the Nyquist row at both ends of the series and its zero-padded `irfft` counts the Nyquist column with its
 * conjugate.  Phases are reduced in integers, sums are kept in double registers and rounded to float32 once.
 *
 * A third library next to libpt_hot.so (include/pt_hot.h) and libpt_mot.so (include/pt_mot.h), with the same conventions:
 *   - all tensors are contiguous float32 device memory unless stated otherwise; `stream` is a hipStream_t (void*), NULL = default;
 *   - every function returns PT_AL_OK (0) or a negative pt_loc_status; nothing is queued when an argument check fails;
 *   - no atomics, no host synchronisation inside the library (pt_loc_atom_wait_f32 is the one documented exception), every sum in a
 *     fixed order: repeated calls give the same bits and both launches can be captured in a graph.
 */
#ifndef PT_LOC_H
#define PT_LOC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pt_loc_status {
    PT_AL_OK = 0,
    PT_AL_ERR_NULL = -1,        /* required pointer is NULL */
    PT_AL_ERR_SHAPE = -2,       /* non-positive or inconsistent dimension */
    PT_AL_ERR_UNSUPPORTED = -3, /* valid request the kernels do not cover */
    PT_AL_ERR_WORKSPACE = -4,   /* workspace too small or misaligned */
    PT_AL_ERR_LAUNCH = -5       /* hipGetLastError() != hipSuccess after a launch */
} pt_loc_status;

const char* pt_loc_strerror(int status);
int pt_loc_abi_version(void);

#define PT_AL_MAX_SCALES 8      /* S */
#define PT_AL_MIN_SERIES 4      /* N_h, N_w */
#define PT_AL_MAX_SERIES 32
#define PT_AL_MAX_GRID 576      /* G_h, G_w; each strictly larger than 2 * (N / 2) + 1 */
#define PT_AL_BAND_ROWS 8       /* grid rows per workgroup of the interpolation launch (the one band split there is) */
#define PT_AL_REC_FLOATS 16     /* the result record */

/* outcome of `localize_advanced`: the values of PT_LOC_* in pt_hot.h (the plain arg-max branch reports PT_AL_NORMAL) */
enum { PT_AL_NORMAL = 0, PT_AL_HARD_NEGATIVE = 1, PT_AL_UNCERTAIN = 2, PT_AL_NOT_FOUND = 3 };

/* positions inside the result record */
enum {
    PT_AL_R_FLAG = 0,           /* PT_AL_NORMAL ... PT_AL_NOT_FOUND */
    PT_AL_R_SCALE = 1,          /* scale_ind */
    PT_AL_R_ROW1 = 2,           /* first peak: cell (`max_disp1`) and value */
    PT_AL_R_COL1 = 3,
    PT_AL_R_MAX1 = 4,
    PT_AL_R_ROW2 = 5,           /* second peak on the masked map (0, 0, 0 when the plain branch or `not_found` skipped the search) */
    PT_AL_R_COL2 = 6,
    PT_AL_R_MAX2 = 7,
    PT_AL_R_TV = 8,             /* 2 floats: translation_vec [row, col] */
    PT_AL_R_PICK = 10,          /* 1: translation_vec comes from the first peak, 2: from the second (atom.py:396) */
    PT_AL_R_WHICH = 11,         /* the map the reference method returns: 0 `map_out`, 1 `map_hn_out` (atom.py:369-370) */
    PT_AL_R_SEQ = 15            /* the call's sequence word, stored last */
};

/* What one call reads from the tracker, each value in the type the reference holds it in: `params.*` and the translation weight are
 * Python floats (doubles), the sizes float32 CPU tensors, `target_scale` a Python float or a float32 tensor (either way it enters the
 * reference's float32 products rounded to float32). */
typedef struct {
    double target_not_found_threshold, distractor_threshold, hard_negative_threshold, target_neighborhood_scale, dispalcement_scale,
        translation_weight, target_scale;
    float img_support_sz[2], output_sz[2], target_sz[2];
    float scale_factors[PT_AL_MAX_SCALES];   /* params.scale_factors (read by the plain branch only, atom.py:331) */
    int kernel_size[2];
    int advanced_localization;   /* params.advanced_localization */
    int windowed;                /* self.output_window is not None */
    int hn_without_windowing;    /* params.perform_hn_without_windowing */
    int reserved;
} pt_loc_atom_state;

/* the parameter block of the kernels */
typedef struct {
    double target_not_found_threshold;
    float distractor_threshold, hard_negative_threshold, target_not_found_f32, disp_threshold;
    float ratio[2];              /* img_support_sz / output_sz */
    float center[2];             /* output_sz // 2 */
    float half[2];               /* output_sz / 2 */
    float neigh[2];              /* target_neigh_sz */
    float target_scale, weight;
    float scale_factors[PT_AL_MAX_SCALES];
    int parity[2];               /* kernel_size % 2 */
    int advanced, windowed, hn;  /* hn: windowed and perform_hn_without_windowing */
    int reserved;
} pt_loc_atom_params;

/* Host only: the parameter block from the tracker state, in the reference's float32 operation order (atom.py:327-331, 363-364, 373, 391).
 * PT_AL_ERR_SHAPE for a non-positive size or scale. */
int pt_loc_atom_constants_f32(const pt_loc_atom_state* state, pt_loc_atom_params* out);

/* Bytes of workspace pt_loc_atom_f32 needs for this shape (one partial peak per band and scale); 0 for a shape it refuses. */
size_t pt_loc_atom_ws_bytes(int S, int Nh, int Nw, int Gh, int Gw);

/* Queues the two launches.
 *   scores (S, 1, Nh, Nw): the raw classification scores;  window (Gh, Gw): `self.output_window`, required when prm->windowed.
 *   map_out (S, 1, Gh, Gw): the map the first peak is found on -- rolled by (G + 1) // 2 (atom.py:355-356) when prm->advanced, as sampled
 *   otherwise; windowed when prm->windowed and (not prm->hn or prm->advanced).
 *   map_hn_out (S, 1, Gh, Gw): required when prm->advanced and prm->hn: the rolled un-windowed map the second peak is found on.
 *   rec: PT_AL_REC_FLOATS floats, device memory or pinned host memory the device can write, the PT_AL_R_SEQ word stored last (system scope
 *   release) with the value `seq`.
 *   ws: 256-byte aligned device memory of pt_loc_atom_ws_bytes.
 * Launch 1, grid (ceil(Gh / PT_AL_BAND_ROWS), S): each workgroup interpolates PT_AL_BAND_ROWS grid rows of one scale and leaves the band's
 * peak; launch 2, one workgroup: the first peak over bands and scales, the masked second peak of the chosen scale, the outcome.
 * Refused with PT_AL_ERR_UNSUPPORTED before anything is queued: S outside 1..PT_AL_MAX_SCALES, a series side outside
 * PT_AL_MIN_SERIES..PT_AL_MAX_SERIES, a grid side above PT_AL_MAX_GRID or not strictly larger than 2 * (N / 2) + 1 (the reference raises for
 * a smaller grid and takes another route, with another column count, for an equal one). */
int pt_loc_atom_f32(const float* scores, int S, int Nh, int Nw, int Gh, int Gw, const float* window, const pt_loc_atom_params* prm,
                    float* map_out, float* map_hn_out, float* rec, float seq, void* ws, size_t ws_bytes, void* stream);

/* Host only: returns when the PT_AL_R_SEQ word of the record holds `seq` (rec_host: pinned host memory the call was given as `rec`).  After
 * 2 s without it, it falls back to hipStreamSynchronize(stream) once. */
int pt_loc_atom_wait_f32(const float* rec_host, float seq, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PT_LOC_H */
