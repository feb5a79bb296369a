// libpt_mem: the trackers' per-frame sample-memory update on the device (include/pt_mem.h).
//   DiMP.update_memory / update_sample_weights      pytracking/tracker/dimp/dimp.py:430-484   (rule A; kys.py:534, tomp.py:546,
//                                                   dimp_simple.py:457, tamos.py:514 are copies)
//   ATOM.update_memory / update_sample_weights      atom.py:590-639                           (rule B)
//   LWL.update_memory / update_sample_weights       lwl.py:459-516, rts.py:594                (rule C)
//   KeepTrack.update_sample_weights_based_on_certainty   keep_track.py:667-708                (rule D)
// The reference runs about ten tiny launches on an n-element vector and synchronises the host twice per update: `torch.min(...)` followed by
// `.item()`, and the truth test of the device tensor `sw[:num_init].sum() < init_samp_weight`.
//
// Launch 1 (k_mem_weights), grid (B), 256 threads: one workgroup per entry of `sample_weights`.  A thread holds the weights tid, tid + 256,
// tid + 512, tid + 768 and their arg-min keys in registers, read before anything is written.  The first arg-min (torch.min's tie order: lowest
// index among equal keys, the first NaN if there is one), the update, the sum and the floor decision follow; the weights, the index (workspace)
// and the record are written at the end.  Sums: double, per thread in index order, then the wave's shuffle tree, then the four waves in
// order -- a fixed order, so the bits repeat.  Every weight a reference statement stores is the double result rounded to float32 once.
// Launch 2 (k_mem_insert), 256 threads per workgroup, one 16-byte chunk per thread and grid-stride step: every row goes to
// dst + index[block] * elems, with 16-byte loads and stores when src and the slot are 16-byte aligned, element by element otherwise.
#include <chrono>
#include <math.h>
#include "../csrc/pt_internal.h"
#include "../../include/pt_mem.h"

#define PT_MEM_CHECK_LAUNCH()                                          \
    do {                                                               \
        if (hipGetLastError() != hipSuccess) return PT_MEM_ERR_LAUNCH; \
    } while (0)

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64, PER = PT_MEM_MAX_WEIGHTS / THREADS;
constexpr int ROW_WGS = 256;                       // workgroups per row at the most: 8 rows fill 2048 workgroups, the rest is grid-stride

struct MemArgs {
    pt_mem_block b[PT_MEM_MAX_BLOCKS];
    pt_mem_row r[PT_MEM_MAX_ROWS];
    int row_n[PT_MEM_MAX_ROWS];                    // slots of the row's memory
    int row_wg0[PT_MEM_MAX_ROWS + 1];              // first workgroup of every row in launch 2
    int B, R;
    float* rec;
    int* idx;                                      // workspace: the replace index per block
    float seq;
};

struct Key { float k; int i; };

// torch.min over a 1-d tensor: NaN wins, then the smaller value, then the lower index
__device__ __forceinline__ bool before(const Key a, const Key b) {
    const bool an = a.k != a.k, bn = b.k != b.k;
    if (an != bn) return an;
    if (!an && a.k != b.k) return a.k < b.k;
    return a.i < b.i;
}

__device__ __forceinline__ Key block_argmin(Key v, Key* sh) {
    for (int off = 32; off > 0; off >>= 1) {
        const Key o{__shfl_down(v.k, off), __shfl_down(v.i, off)};
        if (before(o, v)) v = o;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    Key m = sh[0];
    for (int w = 1; w < WAVES; ++w)
        if (before(sh[w], m)) m = sh[w];
    return m;
}

__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < WAVES; ++w) s += sh[w];
    return s;
}

__global__ __launch_bounds__(THREADS) void k_mem_weights(MemArgs a) {
    __shared__ Key sh_key[WAVES];
    __shared__ double sh_sum[WAVES];
    const int blk = blockIdx.x, tid = threadIdx.x;
    const pt_mem_block& q = a.b[blk];
    const int n = q.n, num_init = q.num_init, prev = q.prev_ind, rule = q.rule;
    const bool floored = q.floor > 0.0;
    const int s_ind = floored ? num_init : 0;

    float w[PER], key[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * THREADS;
        w[j] = i < n ? q.weights[i] : 0.f;
        key[j] = (rule == PT_MEM_RULE_D && i < n) ? __fmul_rn(q.certainty[i], w[j]) : w[j];
    }
    const float w_prev = prev >= 0 ? q.weights[prev] : 0.f;

    int r = 0;
    if (q.num_stored == 0 || q.lr == 1.0) {                                  // sw[:] = 0; sw[0] = 1
#pragma unroll
        for (int j = 0; j < PER; ++j) w[j] = (tid + j * THREADS == 0) ? 1.f : 0.f;
    } else {
        if (rule != PT_MEM_RULE_B && q.num_stored < n) {
            r = q.num_stored;
        } else {                                                             // _, r_ind = torch.min(key[s_ind:], 0)
            Key best{INFINITY, 0x7fffffff};
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const Key c{key[j], tid + j * THREADS};
                if (c.i >= s_ind && c.i < n && (best.i == 0x7fffffff || before(c, best))) best = c;
            }
            r = block_argmin(best, sh_key).i;
        }
        const double keep = 1.0 - q.lr;
        if (prev < 0) {
            const bool lower = rule == PT_MEM_RULE_C && q.lower_init_weight != 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int i = tid + j * THREADS;
                if (!lower) w[j] = (float)((double)w[j] / keep);             // sw /= 1 - lr
                if (i == r) w[j] = lower ? 1.f : (float)q.lr;                // sw[r_ind] = lr
            }
        } else if (!(rule == PT_MEM_RULE_D && r == prev)) {
            const float v = (float)((double)w_prev / keep);                  // sw[r_ind] = sw[prev_ind] / (1 - lr)
#pragma unroll
            for (int j = 0; j < PER; ++j)
                if (tid + j * THREADS == r) w[j] = v;
        }
    }

    double part = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) part += (tid + j * THREADS < n) ? (double)w[j] : 0.0;
    const double total = block_sum(part, sh_sum);
#pragma unroll
    for (int j = 0; j < PER; ++j) w[j] = (float)((double)w[j] / total);      // sw /= sw.sum()

    int applied = 0;
    if (floored) {
        double head = 0.0, tail = 0.0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * THREADS;
            if (i < num_init) head += (double)w[j];
            else if (i < n) tail += (double)w[j];
        }
        head = block_sum(head, sh_sum);
        tail = block_sum(tail, sh_sum);
        if (head < q.floor) {                                                // sw[:num_init].sum() < init_samp_weight
            applied = 1;
            const double div = q.floor + tail;
            const float init = (float)(q.floor / (double)num_init);
#pragma unroll
            for (int j = 0; j < PER; ++j) w[j] = (tid + j * THREADS < num_init) ? init : (float)((double)w[j] / div);
        }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * THREADS;
        if (i < n) q.weights[i] = w[j];
    }
    if (tid != 0) return;
    a.idx[blk] = r;
    float* o = a.rec;
    o[PT_MEM_R_INDEX + blk] = (float)r;
    o[PT_MEM_R_FLOOR + blk] = (float)applied;
    o[PT_MEM_R_SUM + blk] = (float)total;
    if (blk == 0)
        for (int k = a.B; k < PT_MEM_MAX_BLOCKS; ++k) o[PT_MEM_R_INDEX + k] = o[PT_MEM_R_FLOOR + k] = o[PT_MEM_R_SUM + k] = 0.f;
    __threadfence_system();                                                  // the record is visible before its sequence words
    __hip_atomic_store(o + PT_MEM_R_SEQ + blk, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (blk == 0)
        for (int k = a.B; k < PT_MEM_MAX_BLOCKS; ++k) __hip_atomic_store(o + PT_MEM_R_SEQ + k, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ float row_value(int op, float arg, float v) {
    return op == PT_MEM_THRESH ? (v >= arg ? 1.f : 0.f) : v;
}

__global__ __launch_bounds__(THREADS) void k_mem_insert(MemArgs a) {
    const int wg = blockIdx.x;
    int r = 0;
    while (r + 1 < a.R && wg >= a.row_wg0[r + 1]) ++r;
    const pt_mem_row& row = a.r[r];
    const int idx = a.idx[row.block];
    if (idx < 0 || idx >= a.row_n[r]) return;                                // cannot happen: launch 1 chooses inside the memory
    const size_t elems = row.elems, chunks = (elems + 3) / 4;
    float* out = row.dst + (size_t)idx * elems;
    if (row.op == PT_MEM_SCALAR) {
        if (threadIdx.x == 0) out[0] = row.arg;
        return;
    }
    const float* src = row.src;
    const int op = row.op;
    const float arg = row.arg;
    const bool vec = ((((uintptr_t)src) | ((uintptr_t)out)) & 15) == 0;
    const size_t step = (size_t)(a.row_wg0[r + 1] - a.row_wg0[r]) * THREADS;
    for (size_t c = (size_t)(wg - a.row_wg0[r]) * THREADS + threadIdx.x; c < chunks; c += step) {
        const size_t e = c * 4;
        if (vec && e + 4 <= elems) {
            float4 v = *reinterpret_cast<const float4*>(src + e);
            v.x = row_value(op, arg, v.x); v.y = row_value(op, arg, v.y); v.z = row_value(op, arg, v.z); v.w = row_value(op, arg, v.w);
            *reinterpret_cast<float4*>(out + e) = v;
        } else {
            for (size_t k = e; k < e + 4 && k < elems; ++k) out[k] = row_value(op, arg, src[k]);
        }
    }
}

bool device_index(const pt_mem_block& q) {         // the arg-min has to run
    if (q.num_stored == 0 || q.lr == 1.0) return false;
    return q.rule == PT_MEM_RULE_B || q.num_stored >= q.n;
}

int check_block(const pt_mem_block& q) {
    if (!q.weights) return PT_MEM_ERR_NULL;
    if (q.n < 1 || q.n > PT_MEM_MAX_WEIGHTS) return PT_MEM_ERR_UNSUPPORTED;
    if (q.rule < PT_MEM_RULE_A || q.rule > PT_MEM_RULE_D) return PT_MEM_ERR_UNSUPPORTED;
    if (q.num_init < 0 || q.num_stored < 0 || q.prev_ind < -1 || q.prev_ind >= q.n) return PT_MEM_ERR_SHAPE;
    if (!(q.lr >= 0.0 && q.lr <= 1.0) || !(q.floor >= 0.0) || !std::isfinite(q.floor)) return PT_MEM_ERR_SHAPE;
    if (q.num_init > q.n) return PT_MEM_ERR_UNSUPPORTED;
    if (q.rule == PT_MEM_RULE_D && !q.certainty) return PT_MEM_ERR_UNSUPPORTED;
    if (q.floor > 0.0) {
        if (q.num_init == 0) return PT_MEM_ERR_UNSUPPORTED;                 // floor / num_init
        if (q.num_init == q.n && device_index(q)) return PT_MEM_ERR_UNSUPPORTED;   // torch.min of an empty tensor
    }
    return PT_MEM_OK;
}

}  // namespace

extern "C" const char* pt_mem_strerror(int status) {
    switch (status) {
        case PT_MEM_OK: return "ok";
        case PT_MEM_ERR_NULL: return "required pointer is NULL";
        case PT_MEM_ERR_SHAPE: return "non-positive or inconsistent dimension or index";
        case PT_MEM_ERR_UNSUPPORTED: return "unsupported: configuration not covered by the gfx950 memory update";
        case PT_MEM_ERR_WORKSPACE: return "workspace too small or misaligned";
        case PT_MEM_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown status";
    }
}

extern "C" int pt_mem_abi_version(void) { return 1; }

extern "C" int pt_mem_host_index(const pt_mem_block* q) {
    if (!q) return -1;
    if (q->num_stored == 0 || q->lr == 1.0) return 0;
    if (q->rule != PT_MEM_RULE_B && q->num_stored >= 0 && q->num_stored < q->n) return q->num_stored;
    return -1;
}

extern "C" size_t pt_mem_ws_bytes(int B) { return (B < 1 || B > PT_MEM_MAX_BLOCKS) ? 0 : 256; }

extern "C" int pt_mem_update_f32(const pt_mem_block* blocks, int B, const pt_mem_row* rows, int R, float* rec, float seq, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (!blocks || !rec || !ws || (R > 0 && !rows)) return PT_MEM_ERR_NULL;
    if (B < 1 || B > PT_MEM_MAX_BLOCKS || R < 0 || R > PT_MEM_MAX_ROWS) return PT_MEM_ERR_UNSUPPORTED;
    MemArgs a{};
    for (int b = 0; b < B; ++b) {
        const int rc = check_block(blocks[b]);
        if (rc != PT_MEM_OK) return rc;
        a.b[b] = blocks[b];
    }
    int wgs = 0;
    for (int r = 0; r < R; ++r) {
        const pt_mem_row& row = rows[r];
        if (row.block < 0 || row.block >= B) return PT_MEM_ERR_UNSUPPORTED;
        if (row.op < PT_MEM_COPY || row.op > PT_MEM_SCALAR) return PT_MEM_ERR_UNSUPPORTED;
        if (!row.dst || (row.op != PT_MEM_SCALAR && !row.src)) return PT_MEM_ERR_NULL;
        if (row.elems == 0) return PT_MEM_ERR_SHAPE;
        if (row.op == PT_MEM_SCALAR && row.elems != 1) return PT_MEM_ERR_UNSUPPORTED;
        const int n = blocks[row.block].n;
        if (row.op != PT_MEM_SCALAR) {
            const uintptr_t s0 = (uintptr_t)row.src, s1 = s0 + row.elems * sizeof(float);
            const uintptr_t d0 = (uintptr_t)row.dst, d1 = d0 + (size_t)n * row.elems * sizeof(float);
            if (s0 < d1 && d0 < s1) return PT_MEM_ERR_UNSUPPORTED;
        }
        a.r[r] = row;
        a.row_n[r] = n;
        a.row_wg0[r] = wgs;
        const size_t want = ((row.elems + 3) / 4 + THREADS - 1) / THREADS;
        wgs += (int)(want < (size_t)ROW_WGS ? want : (size_t)ROW_WGS);
    }
    for (int r = R; r <= PT_MEM_MAX_ROWS; ++r) a.row_wg0[r] = wgs;
    if (ws_bytes < pt_mem_ws_bytes(B) || ((uintptr_t)ws & 255)) return PT_MEM_ERR_WORKSPACE;
    a.B = B; a.R = R; a.rec = rec; a.idx = (int*)ws; a.seq = seq;
    hipLaunchKernelGGL(k_mem_weights, dim3(B), dim3(THREADS), 0, (hipStream_t)stream, a);
    PT_MEM_CHECK_LAUNCH();
    if (R > 0) {
        hipLaunchKernelGGL(k_mem_insert, dim3(wgs), dim3(THREADS), 0, (hipStream_t)stream, a);
        PT_MEM_CHECK_LAUNCH();
    }
    return PT_MEM_OK;
}

extern "C" int pt_mem_wait_f32(const float* rec_host, float seq, void* stream) {
    if (!rec_host) return PT_MEM_ERR_NULL;
    const volatile float* word = rec_host + PT_MEM_R_SEQ;
    const int want = __builtin_bit_cast(int, seq);
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < PT_MEM_MAX_BLOCKS; ++k) {
        while (__atomic_load_n((const volatile int*)(word + k), __ATOMIC_ACQUIRE) != want) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return PT_MEM_ERR_LAUNCH;
                return PT_MEM_OK;
            }
        }
    }
    return PT_MEM_OK;
}
