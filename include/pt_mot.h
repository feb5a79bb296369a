/*
 * pt_mot.h -- C ABI of libpt_mot.so: the per-frame multi-object read-out of the TaMOs tracker on AMD Instinct MI355X
 * (gfx950), i.e. what `TaMOs.track` does per object with the classifier's score maps and the box regressor's ltrb maps
 * (pytracking/tracker/tamos/tamos.py:106-153, 248-280, 319-320, 324-429, 582-599), and the training targets of its memory.
 *
 * A second library next to libpt_hot.so (include/pt_hot.h), with the same conventions:
 *   - all tensors are contiguous float32 device memory unless stated otherwise; `stream` is a hipStream_t (void*), NULL = default;
 *   - every function returns PT_MOT_OK (0) or a negative pt_mot_status; nothing is queued when an argument check fails;
 *   - no atomics, no host synchronisation inside the library (pt_mot_wait_f32 is the one documented exception), every sum in a
 *     fixed order: repeated calls give the same bits and every launch can be captured in a graph.
 */
#ifndef PT_MOT_H
#define PT_MOT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pt_mot_status {
    PT_MOT_OK = 0,
    PT_MOT_ERR_NULL = -1,        /* required pointer is NULL */
    PT_MOT_ERR_SHAPE = -2,       /* non-positive or inconsistent dimension, bad object index */
    PT_MOT_ERR_UNSUPPORTED = -3, /* valid request the kernels do not cover */
    PT_MOT_ERR_WORKSPACE = -4,   /* (reserved: no entry point of this library takes a workspace) */
    PT_MOT_ERR_LAUNCH = -5       /* hipGetLastError() != hipSuccess after a launch */
} pt_mot_status;

const char* pt_mot_strerror(int status);
int pt_mot_abi_version(void);

#define PT_MOT_MAX_OBJECTS 16    /* objects per frame (the deployed tracker follows 10) */
#define PT_MOT_MAX_CELLS 8192    /* H * W of the map the decision is taken on: it is staged in 32 KiB of LDS */
#define PT_MOT_MAX_CENTRES 64    /* Gaussian labels per pt_mot_targets_f32 call */
#define PT_MOT_REC_FLOATS 32     /* one result record per object */

/* outcome of `localize_advanced`: the values of PT_LOC_* in pt_hot.h */
enum { PT_MOT_NORMAL = 0, PT_MOT_HARD_NEGATIVE = 1, PT_MOT_UNCERTAIN = 2, PT_MOT_NOT_FOUND = 3 };

/* positions inside a result record */
enum {
    PT_MOT_R_FLAG = 0,           /* PT_MOT_NORMAL ... PT_MOT_NOT_FOUND */
    PT_MOT_R_PICK = 1,           /* 1: the first peak is `score_loc`, 2: the second (tamos.py:419) */
    PT_MOT_R_ROW = 2,            /* chosen cell */
    PT_MOT_R_COL = 3,
    PT_MOT_R_MAX1 = 4,           /* first peak: value, row, col */
    PT_MOT_R_ROW1 = 5,
    PT_MOT_R_COL1 = 6,
    PT_MOT_R_MAX2 = 7,           /* second peak on the masked map: value, row, col (0, 0, 0 when an early exit skipped the search) */
    PT_MOT_R_ROW2 = 8,
    PT_MOT_R_COL2 = 9,
    PT_MOT_R_PRESENCE = 10,      /* maximum of the un-masked map: `object_presence_score` */
    PT_MOT_R_RAW_BOX = 11,       /* 4 floats x, y, w, h of direct_bbox_regression */
    PT_MOT_R_BOX = 15,           /* 4 floats x, y, w, h after clip_bbox_to_image_area */
    PT_MOT_R_LTRB = 19,          /* the four ltrb values read at the chosen cell */
    PT_MOT_R_OBJECT = 23,        /* the object's index */
    PT_MOT_R_SECOND = 24,        /* 1 when the second peak was searched for (no threshold exit) */
    PT_MOT_R_SEQ = 31            /* the call's sequence word, stored last */
};

/* What one frame's read-out reads from the tracker, each value in the type the reference holds it in: `params.*` thresholds and
 * `self.scale_factor` are Python floats (doubles), the sizes float32 CPU tensors, the image size and the stride ints.  Optional
 * thresholds the parameter file does not define are -inf (their test never fires).  The last five fields state the configuration;
 * what the kernels do not cover is refused (see pt_mot_readout_f32). */
typedef struct {
    double target_not_found_threshold, uncertain_threshold, hard_sample_threshold, distractor_threshold,
        hard_negative_threshold, target_neighborhood_scale, dispalcement_scale, scale_factor;
    float img_support_sz[2], img_sample_sz[2], train_img_sample_sz[2], kernel_size[2];
    float sample_coords[4];      /* row 0 of `sample_coords`: y0, x0, y1, x1 */
    int image_h, image_w;        /* image.shape[:2] */
    int stride;                  /* of the box regression (track() passes 8) */
    int min_width, min_height;   /* of clip_bbox_to_image_area (10, 10) */
    int normalize_scores;        /* params.normalize_scores: sigmoid of the map */
    int score_preprocess;        /* 0 'none'; anything else is refused */
    int score_filter_ksz;        /* <= 1, or refused */
    int window_output;           /* 0, or refused */
    int advanced_localization;   /* 1, or refused */
} pt_mot_frame;

/* host state of one object: self.pos[oid], self.pos_prev[oid], self.target_sz[oid] (float32, [row, col]) */
typedef struct {
    float pos[2], pos_prev[2], target_sz[2];
} pt_mot_object;

/* per-object constants of localize_advanced in score cells (tamos.py:372,394,408,414) */
typedef struct {
    float center[2];             /* score_center */
    float neigh[2];              /* target_neigh_sz */
    float prev[2];               /* prev_target_vec */
    float disp_threshold;
    float reserved;
} pt_mot_consts;

/* Host only: the constants above from the host state, in the reference's float32 operation order (H, W: size of the map the decision is
 * taken on).  PT_MOT_ERR_UNSUPPORTED for an even kernel_size. */
int pt_mot_constants_f32(const pt_mot_frame* frame, const pt_mot_object* object, int H, int W, pt_mot_consts* out);

/* The whole per-object decision of one frame, one launch, one workgroup per active object.
 *   scores (T, Hs, Ws): the classifier's raw output;  ltrb (T, 4, H, W): the box regressor's output.
 *   The map the decision is taken on has the size (H, W): `scores` itself when (Hs, Ws) == (H, W); its bicubic upsample (A = -0.75,
 *   align_corners = False, taps clamped: tamos.py:319-320) when both sizes differ; one size equal and one different is PT_MOT_ERR_SHAPE
 *   (the reference fails there too).  With frame->normalize_scores the sigmoid follows.  The map is staged in LDS once and, when
 *   map_out is not NULL, written to map_out[object] of the (T, H, W) tensor map_out.
 *   active: HOST array of n_active distinct object indices in [0, T); objects: HOST array of n_active states, in the same order.
 *   rec: T records of PT_MOT_REC_FLOATS floats, device memory or pinned host memory the device can write; the records of the active
 *   objects are written, each one's PT_MOT_R_SEQ word last (system scope release) with the value `seq`.  seq = 0: no word is kept apart,
 *   the slot is written 0 like the reserved ones.
 * Refused with PT_MOT_ERR_UNSUPPORTED before anything is queued: T or n_active outside 1..PT_MOT_MAX_OBJECTS, H * W > PT_MOT_MAX_CELLS,
 * score_preprocess != 0, score_filter_ksz > 1, window_output, advanced_localization off, an even kernel_size. */
int pt_mot_readout_f32(const float* scores, int Hs, int Ws, const float* ltrb, int H, int W, int T, const int* active, int n_active,
                       const pt_mot_object* objects, const pt_mot_frame* frame, float* map_out, float* rec, float seq, void* stream);

/* Host only: returns when the PT_MOT_R_SEQ word of every active object's record holds `seq` (rec_host: pinned host memory the read-out
 * was given as `rec`).  Polls the n_active words; after 2 s without them it falls back to hipStreamSynchronize(stream) once. */
int pt_mot_wait_f32(const float* rec_host, const int* active, int n_active, float seq, void* stream);

/* The Gaussian label of get_label_function / dcf.label_function_spatial (tamos.py:582-592, dcf.py:48-59): the `.item()` doubles of
 * feature_sz, sigma and end_pad ([row, col]).  The label has (sz[0] + end_pad[0], sz[1] + end_pad[1]) cells. */
typedef struct {
    double sz[2], sigma[2], end_pad[2];
} pt_mot_label;

/* The training targets of the memory, one launch.  Either part may be absent (nb = 0 / n_centres = 0), not both.
 *   encode_bbox (tamos.py:114-153): boxes (nb, 4) xywh on the DEVICE -> ltrb_out (nb, 4, out_h / stride, out_w / stride), zeros for a
 *   box with w <= 0 or h <= 0; (out_h, out_w) = params.image_sample_size, both multiples of `stride` (else PT_MOT_ERR_UNSUPPORTED).
 *   label: centres HOST array (n_centres, 2) float32 [row, col] (`center` of tamos.py:589) -> label_out (n_centres, LH, LW);
 *   n_centres <= PT_MOT_MAX_CENTRES. */
int pt_mot_targets_f32(const float* boxes, int nb, int out_h, int out_w, int stride, float* ltrb_out, const pt_mot_label* label,
                       const float* centres, int n_centres, float* label_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PT_MOT_H */
