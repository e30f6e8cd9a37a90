// Shared host-side plumbing of libvmpc_hip: context, workspace arena, error handling,
// per-stage HIP-event profiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/vmpc.h"

extern thread_local char vmpc_err_buf[512];

#define VMPC_HIP_CHECK(expr)                                                                  \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            snprintf(vmpc_err_buf, sizeof vmpc_err_buf, "%s:%d: %s -> %s", __FILE__, __LINE__, \
                     #expr, hipGetErrorString(_e));                                           \
            return VMPC_E_HIP;                                                                \
        }                                                                                     \
    } while (0)

#define VMPC_CHECK(expr)              \
    do {                              \
        int _r = (expr);              \
        if (_r != VMPC_OK) return _r; \
    } while (0)

// device-side status word layout (ctx->d_status, 4 x u32)
#define VMPC_ST_NONCANON 0  // count of non-canonical scalars seen by recode kernels
#define VMPC_ST_SHORT_OVERFLOW 1  // the fused short-commitment path (msm_short.hip) met a bin or bucket beyond its fixed
                                  // capacities: the call's result is void, vmpc_ctx_sync returns VMPC_E_AGAIN
#define VMPC_ST_WORDS 4
#define VMPC_SHORT_CURSOR_WORDS 256  // ctx->short_cursors: [2][128] words (msm_short.hip checks it against its bin count)

struct vmpc_stage {
    const char *name;
    double ms = 0;
    uint64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct vmpc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // growable scratch arena (never shrinks; reused by every call on this context)
    void *ws = nullptr;
    size_t ws_bytes = 0;
    size_t ws_used = 0;
    uint64_t ws_generation = 0;    // allocations of the arena so far (vmpc_ctx_debug_arena_info)
    uint32_t *d_status = nullptr;
    int window_override = 0;
    int bucket_wgs_per_cu = 0;     // > 0: persistent bucket kernel with this many 256-thread workgroups per CU
    int reduce_max_chunks = 32768; // most chunk-lanes per bucket set in the bucket reduction (msm_sort.hip)
    int reduce_chunks_override = 0; // > 0: chunk-lanes per bucket set, fixed (power of two)
    int short_path = 1;            // commitments over a 16-row table of <= 2^17 columns: the fused path (msm_short.hip)
    int short_backoff = 0;         // eligible calls still to take the general path after an overflow (vmpc_ctx_sync sets it)
    size_t lds_optin = 0;          // the device's largest dynamic LDS per workgroup (sharedMemPerBlockOptin)
    int fold_jump_digit_bits = 8;  // signed digits of the fold jump's shared schedule (fold_jump.hip; VMPC_FOLD_JUMP_DIGITS=4: the old form)
    bool sort_wide_ready = false;  // the wide window's fine-sort kernels have their dynamic-LDS limit set (msm_sort.hip)
    bool short_ready = false;      // its kernels' dynamic-LDS limits are set on this context's device
    uint32_t *short_cursors = nullptr;   // [2][128] bin fill counts, zero between calls (the path's last kernel re-arms them)
    int reduce_tree = 1;           // short chunks: weights from the quad tree (msm_reduce_tree.hip), not per-lane ladders
    bool reduce_tree_ready = false; // its kernels' dynamic-LDS limits are set on this context's device
    int seg_shift_min = -3;        // shortest bucket segments the plan may choose: 64 >> 3 entries (msm_sort.hip)
    int sort_fine_bits = -1;       // fine bits of the two-level bucket sort; -1 = automatic (msm_sort.hip)
    int plan_fill_shift = 0;       // the next plan's digit rows are only 1 / 2^shift populated (the A_i, B_i pair of a
                                   // prover round: each scalar vector is zero on half of its positions): the segment
                                   // length follows the expected number of entries, not the number of positions
    int cu_count = 256;
    // what the last sort left in the arena (msm_sort_digits records it, vmpc_ws_reserve clears it): vmpc_msm_sort_view
    vmpc_sort_view sort_view = {};
    bool sort_view_valid = false;
    hipEvent_t xevent = nullptr;   // cross-context ordering (vmpc_ctx_wait_for)
    // Phase pipelining (vmpc_ctx_set_bucket_stream): the bucket stage of every commitment of this context runs on a
    // stream SHARED by the contexts of a pipeline - bucket kernels then run back to back, one at a time, and the sort
    // of the next pass / the reduction and recombination of the previous one run beside them on the contexts' own
    // streams (msm_accumulate).  Not owned.
    hipStream_t bucket_stream = nullptr;
    hipEvent_t ev_sorted = nullptr, ev_bucketed = nullptr;
    hipStream_t stage_stream = nullptr;   // stream the next stage bracket's events are recorded on (nullptr: `stream`)
    // pinned staging for small host -> device parameter blocks (vmpc_stage_h2d)
    void *pin = nullptr;
    size_t pin_bytes = 0;
    hipEvent_t pin_event = nullptr;
    bool stream_waits = false;     // work is queued behind a hipStreamWaitValue32 only this thread can release: nothing
                                   // may synchronise the stream now (vmpc_ws_reserve / vmpc_pinned_reserve refuse to grow)
    // the last kernel of a queued-ahead prover round publishes its completion itself (vmpc_publish_done): set by
    // prover.hip before it queues the round's commitment, consumed (and cleared) by the launch of that kernel
    uint32_t *done_flag_dev = nullptr;
    uint32_t done_seq = 0;
    uint32_t p4_seq = 0;           // sequence numbers of the prover's pinned mailbox words (prover.hip), never reused
    void *pin_out = nullptr;       // 4 KiB of pinned, device-mapped host memory behind `pin` (same allocation): small
    void *pin_out_dev = nullptr;   // results a kernel writes for the host every round (prover.hip); its device address
    // arena of the prover's round context, kept between proofs (prover.hip)
    void *p4_pool = nullptr;
    size_t p4_pool_bytes = 0;
    bool p4_pool_busy = false;
    void *p4_kblock = nullptr;         // the columns of k in a folded vector's table (a single-lane chain of 240
    int p4_kblock_rows = 0;            // doublings, 0.7 ms): k belongs to the CRS, so they are made once
    uint8_t p4_kblock_key[64] = {0};
    // polynomial products over GF(n) of BN-256 (csrc/bn256_koe.hip, csrc/bn256_ntt.hip)
    int poly_product = 0;              // VMPC_POLY_PRODUCT_*: which products koe_poly_mul hands to the NTT (0: none)
    void *ntt_twiddles = nullptr;      // the NTT's twiddle tables, built on first use, independent of the length
    size_t ntt_arena_cap = 0;          // > 0: the NTT's arena cap in bytes (vmpc_ctx_set_ntt_arena_cap; 0: NTT_ARENA_MAX)
    int cs_extension = 0;              // VMPC_CS_EXTENSION_*: which extensions of Protocol 8 cs_extend hands to it (0: none)
    // profiling
    bool profile = false;
    std::vector<vmpc_stage> stages;
    std::vector<hipEvent_t> event_pool;
};

// Reserve `bytes` from the context arena (256-byte aligned).  The arena is reset at the
// start of each public call; if it is too small the call grows it (stream-synchronising).
int vmpc_ws_reserve(vmpc_ctx *ctx, size_t total_bytes);
inline void *vmpc_ws_take(vmpc_ctx *ctx, size_t bytes) {
    size_t off = (ctx->ws_used + 255) & ~(size_t)255;
    ctx->ws_used = off + bytes;
    return (char *)ctx->ws + off;
}
// enqueue a copy of a small host block (schedules, parameter tables) to `dst`; `src` may be freed on return
int vmpc_stage_h2d(vmpc_ctx *ctx, void *dst, const void *src, size_t bytes);
// make sure ctx->pin holds `bytes` (>= 64 KiB) and ctx->pin_out / pin_out_dev exist.  ONE allocation for both:
// on this stack a second hipHostMalloc was seen to drop the GPU mapping of an earlier 4-KiB one (memory access
// fault on the first kernel write after it).
int vmpc_pinned_reserve(vmpc_ctx *ctx, size_t bytes);
inline size_t vmpc_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the product of vmpc_bn256_fr_poly_mul_batch_dev by the NTT over the integers (csrc/bn256_ntt.hip); arguments checked
// by the caller: n_wit >= 1 products of a non-empty window
int vmpc_ntt_poly_mul(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na, const void *b, size_t b_stride,
                      size_t nb, size_t k_lo, size_t k_cnt, void *out, size_t out_stride, size_t n_wit);

// The same machinery for a caller that reserves itself (cs_extend of csrc/circuit_sat.hip: ONE reservation per call).
// vmpc_ntt_plan_at plans n_wit products by transforms of 2^log_l points under an arena cap: `bytes` is what the two
// residue buffers need, b_rows rows of row_bytes for b and `group` rows for a (at most 65535: a grid dimension).
// vmpc_ntt_fr_rows_mul is the product over GF(l) in those buffers, no reservation: `rows` rows of a against ONE b, the
// window [k_lo, k_lo + k_cnt) of the CYCLIC product of 2^log_l points (the caller's L: nothing may alias into the
// window), under the caller's stage names.
struct vmpc_ntt_plan {
    int log_l;
    size_t L, row_bytes;       // residues of one row
    size_t group, b_rows;      // a rows per group; b rows held (1: the shared b)
    size_t bytes;              // arena
};
struct vmpc_ntt_stages {
    const char *split, *fwd, *inv, *crt;
};
vmpc_ntt_plan vmpc_ntt_plan_at(int log_l, bool shared_b, size_t n_wit, size_t cap);
int vmpc_ntt_fr_rows_mul(vmpc_ctx *ctx, const vmpc_ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb, uint32_t *ra,
                         const void *a, size_t a_stride, size_t na, size_t rows, const void *b, size_t nb, size_t k_lo,
                         size_t k_cnt, void *out, size_t out_stride);
// the same window reduced mod n, the BN-256 order (cs_extend<frbn>)
int vmpc_ntt_frbn_rows_mul(vmpc_ctx *ctx, const vmpc_ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb, uint32_t *ra,
                           const void *a, size_t a_stride, size_t na, size_t rows, const void *b, size_t nb, size_t k_lo,
                           size_t k_cnt, void *out, size_t out_stride);

// what csrc/bn256_qap_mtree.hip needs of it besides: the arena cap in force, the arena of vmpc_ntt_poly_mul under a cap,
// and one level of a subproduct tree (all its nodes and rows in one launch sequence) with its arena
size_t vmpc_ntt_arena_cap(const vmpc_ctx *ctx);
size_t vmpc_ntt_poly_mul_bytes(size_t na, size_t nb, bool shared_b, size_t n_wit, size_t cap);
size_t vmpc_ntt_tree_level_bytes(size_t m, size_t nodes, size_t rows);
int vmpc_ntt_tree_level(vmpc_ctx *ctx, const void *T, size_t m, int log_nodes, const void *nin, void *nout,
                        size_t rows_y, size_t rows_z);

// profiling helpers: bracket a kernel launch with events when ctx->profile is on
int vmpc_stage_begin(vmpc_ctx *ctx, const char *name);
void vmpc_stage_end(vmpc_ctx *ctx, int handle);

struct vmpc_stage_scope {
    vmpc_ctx *ctx;
    int h;
    vmpc_stage_scope(vmpc_ctx *c, const char *name) : ctx(c), h(vmpc_stage_begin(c, name)) {}
    ~vmpc_stage_scope() { vmpc_stage_end(ctx, h); }
};

// Tuning knobs whose A/B has been lost (DESIGN.md section 10 keeps the numbers) are read only when
// VMPC_EXPERIMENTAL=1 is set as well: a stray variable in a caller's environment cannot switch a slower path on.
const char *vmpc_getenv_experimental(const char *name);

#define VMPC_IGNORE(expr) ((void)(expr))
#define VMPC_KERNEL_CHECK() VMPC_HIP_CHECK(hipGetLastError())

// Completion word for the host: every workgroup of a grid calls this (one thread, after its own result stores);
// the last one to arrive stores `seq` to `flag` (pinned host memory the host polls) and re-arms the counter.
#ifdef __HIPCC__
__device__ __forceinline__ void vmpc_publish_done(uint32_t *counter, uint32_t *flag, uint32_t seq) {
    __threadfence_system();
    if (atomicAdd(counter, 1u) == gridDim.x - 1) {
        *counter = 0;
        __threadfence_system();
        *(volatile uint32_t *)flag = seq;
    }
}
#endif
