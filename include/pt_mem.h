/*
 * pt_mem.h -- C ABI of libpt_mem.so: the per-frame sample-memory update of the trackers on AMD Instinct MI355X (gfx950), i.e. the step every
 * tracker class ends an update frame with, `update_memory` -> `update_sample_weights` (pytracking/tracker/dimp/dimp.py:430-484 and its eight
 * copies): decay the sample weights, choose the slot to overwrite, renormalise, apply the `init_samples_minimum_weight` floor, and store the
 * new sample, its label / box / mask into that slot -- in two launches and at most one host wait.
 *
 * The rule is written nine times in the reference, in four variants (PT_MEM_RULE_*):
 *   A  dimp.py:445, kys.py:548, tomp.py:563, dimp_simple.py:475, tamos.py:541   r_ind = num_stored while the memory fills, else the first
 *                                                                               arg-min of sw[s_ind:]
 *   B  atom.py:603                                                              always the arg-min (while the memory fills: the first zero)
 *   C  lwl.py:474, rts.py:608                                                   A, and with `lower_init_weight` and no previous index
 *                                                                               sw[r_ind] = 1 without the decay
 *   D  keep_track.py:667                                                        A with the arg-min over certainty * weight; r_ind == prev_ind
 *                                                                               leaves the weights alone
 * Common: `num_stored == 0 or lr == 1` resets to (1, 0, ...); without a previous index `sw /= 1 - lr; sw[r_ind] = lr`, with one
 * `sw[r_ind] = sw[prev_ind] / (1 - lr)`; then `sw /= sw.sum()`; then, when sw[:num_init].sum() < floor,
 * `sw /= floor + sw[num_init:].sum(); sw[:num_init] = floor / num_init` (after which the weights no longer sum to 1: the reference's behaviour).
 *
 * Arithmetic: every sum in double in a fixed order; every weight a reference statement stores is the double result rounded to float32 once.
 * The floor test compares the double sum of the float32 normalised weights with the floor.  The arg-min takes torch.min's tie order (lowest
 * index among equal keys); the rule-D key is the float32 product certainty[i] * weights[i].
 *
 * A fourth library next to libpt_hot.so (include/pt_hot.h), libpt_mot.so (include/pt_mot.h) and libpt_loc.so (include/pt_loc.h), with the same
 * conventions:
 *   - all tensors are contiguous float32 device memory unless stated otherwise; `stream` is a hipStream_t (void*), NULL = default;
 *   - every function returns PT_MEM_OK (0) or a negative pt_mem_status; nothing is queued when an argument check fails;
 *   - no atomics, no host synchronisation inside the library (pt_mem_wait_f32 is the one documented exception), every sum in a fixed order:
 *     repeated calls give the same bits and both launches can be captured in a graph.
 */
#ifndef PT_MEM_H
#define PT_MEM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pt_mem_status {
    PT_MEM_OK = 0,
    PT_MEM_ERR_NULL = -1,        /* required pointer is NULL */
    PT_MEM_ERR_SHAPE = -2,       /* non-positive or inconsistent dimension or index */
    PT_MEM_ERR_UNSUPPORTED = -3, /* valid request the kernels do not cover */
    PT_MEM_ERR_WORKSPACE = -4,   /* workspace too small or misaligned */
    PT_MEM_ERR_LAUNCH = -5       /* hipGetLastError() != hipSuccess after a launch */
} pt_mem_status;

const char* pt_mem_strerror(int status);
int pt_mem_abi_version(void);

#define PT_MEM_MAX_BLOCKS 4      /* B: entries of the tracker's `sample_weights` TensorList per call */
#define PT_MEM_MAX_WEIGHTS 1024  /* n: weights per block */
#define PT_MEM_MAX_ROWS 8        /* R: rows stored per call */
#define PT_MEM_REC_FLOATS 16     /* the result record */

enum { PT_MEM_RULE_A = 0, PT_MEM_RULE_B = 1, PT_MEM_RULE_C = 2, PT_MEM_RULE_D = 3 };

/* what is stored into the slot */
enum {
    PT_MEM_COPY = 0,             /* dst slot = src */
    PT_MEM_THRESH = 1,           /* dst slot = src[i] >= arg ? 1 : 0 (ATOM's hinge_mask row, atom.py:597-599) */
    PT_MEM_SCALAR = 2            /* elems == 1, dst slot = arg: a host float (src is not read) */
};

/* positions inside the result record: PT_MEM_MAX_BLOCKS floats each, entry b belongs to block b */
enum {
    PT_MEM_R_INDEX = 0,          /* replace index */
    PT_MEM_R_FLOOR = 4,          /* 1 when the floor was applied, else 0 */
    PT_MEM_R_SUM = 8,            /* the normalising sum (`sw.sum()` in front of the floor test) */
    PT_MEM_R_SEQ = 12            /* the call's sequence word, one per workgroup, each stored last: the record is complete when all
                                    PT_MEM_MAX_BLOCKS words hold it (the workgroup of block 0 stores the words of the blocks a call lacks) */
};

/* One entry of the tracker's `sample_weights` TensorList and the host state the reference reads next to it. */
typedef struct {
    float* weights;              /* (n), updated in place */
    const float* certainty;      /* (n): `target_label_certainties`, rule D only; NULL otherwise */
    int n, num_init, num_stored;
    int prev_ind;                /* previous replace index, -1 for None */
    int rule;                    /* PT_MEM_RULE_* */
    int lower_init_weight;       /* params.lower_init_weight (read by rule C) */
    double lr;                   /* the learning rate as the Python float the reference holds */
    double floor;                /* init_samples_minimum_weight; 0 = none */
} pt_mem_block;

/* One tensor stored into the chosen slot of its block: dst + index[block] * elems. */
typedef struct {
    const float* src;            /* (elems); may be an offset slice of a larger tensor */
    float* dst;                  /* (blocks[block].n, elems): the whole memory */
    size_t elems;
    int block;
    int op;                      /* PT_MEM_COPY / PT_MEM_THRESH / PT_MEM_SCALAR */
    float arg;
    int reserved;
} pt_mem_row;

/* Host only: the replace index where the reference's index is a host value: the reset case (num_stored == 0 or lr == 1) -> 0; rules A / C / D
 * with num_stored < n -> num_stored.  -1 where the index comes from the device (and for a NULL block). */
int pt_mem_host_index(const pt_mem_block* block);

/* Bytes of workspace pt_mem_update_f32 needs for B blocks (the indices the second launch reads); 0 for a B it refuses. */
size_t pt_mem_ws_bytes(int B);

/* Queues the two launches.
 *   blocks: B entries, rows: R entries (host arrays, read before the call returns; R may be 0 and rows NULL then).
 *   rec: PT_MEM_REC_FLOATS floats, device memory or pinned host memory the device can write; the PT_MEM_R_SEQ words are stored last (system
 *   scope release) with the value `seq`.
 *   ws: 256-byte aligned device memory of pt_mem_ws_bytes(B).
 * Launch 1 (k_mem_weights), grid (B): one workgroup per block: the arg-min, the update, the sum, the floor; writes the weights, the index into
 * the workspace and the record.  Launch 2 (k_mem_insert), grid over 16-byte chunks of all rows: stores every row at its block's index.
 * Refused with PT_MEM_ERR_UNSUPPORTED before anything is queued: B outside 1..PT_MEM_MAX_BLOCKS, R outside 0..PT_MEM_MAX_ROWS, n outside
 * 1..PT_MEM_MAX_WEIGHTS, num_init > n, a floor with num_init == 0, a floor with num_init == n where the arg-min has to run (the reference
 * raises on the empty torch.min there), a row whose block is out of range, a row whose src range overlaps its dst memory, an unknown rule or op,
 * PT_MEM_SCALAR with elems != 1, rule D without certainty.  PT_MEM_ERR_SHAPE: negative num_init / num_stored, prev_ind outside -1..n-1,
 * elems == 0, lr outside 0..1, a floor that is negative or not finite.
 * Not checked, the caller guarantees it: the dst memories of two rows do not overlap each other, and no dst or src overlaps a weights
 * vector, the workspace or the record.  A dst may be the block's certainty vector (KeepTrack stores the new certainty there): launch 1 has
 * read it before launch 2 writes. */
int pt_mem_update_f32(const pt_mem_block* blocks, int B, const pt_mem_row* rows, int R, float* rec, float seq, void* ws, size_t ws_bytes,
                      void* stream);

/* Host only: returns when all PT_MEM_R_SEQ words of the record hold `seq` (rec_host: pinned host memory the call was given as `rec`).  After
 * 2 s without them, it falls back to hipStreamSynchronize(stream) once. */
int pt_mem_wait_f32(const float* rec_host, float seq, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PT_MEM_H */
