// Sums of products of sparse entries with a dense vector over a field of csrc/fr256.h: the transposed sparse product
//     out[dst(c)] = sum over the entries e of column c of vals[e] weights[rows[e]]
// (a row sum is the same thing with rows and columns exchanged), deterministic, no atomics.
//
// fr_sparse_dot is the lane body: a range of entries against the vector through an index map, unreduced products in
// f256_acc, ONE reduction.  fr_colsum runs a plan over entries in column order (sparse.colsum_plan makes it on the
// host): ITEMS (start, end, dst) of at most 64 entries, one lane each - dst < n_out: the column fits one item and the
// lane writes out[dst]; dst = FR_COLSUM_PARTIAL | p: the lane writes partial sum p of a LONG column - and long columns
// (dst, first partial, count), one workgroup each, which adds the column's partials in a fixed tree.  Entries past
// nnz, entries whose row is not below n_rows and destinations out of range add / write nothing.
#pragma once
#include "common.h"
#include "fr256.h"

#define FR_COLSUM_WG 256
#define FR_COLSUM_PARTIAL 0x80000000u
#define FR_SPARSE_SKIP 0xFFFFFFFFu

// sum over e in [e0, e1) of vals[e] vec[map(idx[e])], entries whose map is FR_SPARSE_SKIP left out.  E: the caller's
// index type.  The map returns the position by value: written through a reference it cost k_fr_colsum six VGPRs.
template <class F, class E, class Map>
__device__ __forceinline__ F fr_sparse_dot(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ vals, E e0,
                                           E e1, const uint32_t *__restrict__ vec, const Map map) {
    f256_acc acc = f256_acc_zero();
    for (E e = e0; e < e1; e++) {
        const uint32_t p = map(idx[e]);
        if (p == FR_SPARSE_SKIP) continue;
        const F a = f256_ld<F>(vals, (long long)e), b = f256_ld<F>(vec, p);
        f256_acc_mac(acc, a.v, b.v);
    }
    return f256_acc_reduce<F>(acc);
}

// the identity on [0, n), nothing outside
struct fr_colsum_below {
    uint32_t n;
    __device__ uint32_t operator()(uint32_t r) const { return r < n ? r : FR_SPARSE_SKIP; }
};

template <class F>
__global__ void __launch_bounds__(FR_COLSUM_WG)
k_fr_colsum(const uint32_t *__restrict__ weights, uint32_t n_rows, const uint32_t *__restrict__ rows,
            const uint32_t *__restrict__ vals, uint64_t nnz, const uint32_t *__restrict__ items, uint64_t n_items,
            uint32_t *__restrict__ part, uint32_t n_partial, uint32_t *__restrict__ out, uint32_t n_out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_items) return;
    const uint32_t e0 = items[3 * k], e1 = items[3 * k + 1], dst = items[3 * k + 2];
    const F v = fr_sparse_dot<F>(rows, vals, (uint64_t)e0, e1 < nnz ? (uint64_t)e1 : nnz, weights,
                                 fr_colsum_below{n_rows});
    if (dst & FR_COLSUM_PARTIAL) {
        if ((dst & ~FR_COLSUM_PARTIAL) < n_partial) f256_st(part, dst & ~FR_COLSUM_PARTIAL, v);
    } else if (dst < n_out) {
        f256_st(out, dst, v);
    }
}

// one workgroup per long column (dst, first, count): out[dst] = sum of part[first .. first + count), fixed order
template <class F>
__global__ void __launch_bounds__(FR_COLSUM_WG)
k_fr_colfinish(const uint32_t *__restrict__ longs, const uint32_t *__restrict__ part, uint32_t n_partial,
               uint32_t *__restrict__ out, uint32_t n_out) {
    __shared__ F red[FR_COLSUM_WG];
    const int t = threadIdx.x;
    const uint32_t dst = longs[3 * blockIdx.x], first = longs[3 * blockIdx.x + 1], count = longs[3 * blockIdx.x + 2];
    F s = f256_zero<F>();
    for (uint64_t i = t; i < count; i += FR_COLSUM_WG)
        if ((uint64_t)first + i < n_partial) s = f256_add(s, f256_ld<F>(part, (long long)(first + i)));
    red[t] = s;
    __syncthreads();
    for (int h = FR_COLSUM_WG / 2; h > 0; h >>= 1) {
        if (t < h) red[t] = f256_add(red[t], red[t + h]);
        __syncthreads();
    }
    if (t == 0 && dst < n_out) f256_st(out, dst, red[0]);
}

// VMPC_E_RANGE, then VMPC_E_INVAL, before any pointer is touched; max_rows: the caller's cap on the dense vector
static inline int fr_colsum_check(const vmpc_ctx *ctx, const void *weights, size_t n_rows, size_t max_rows,
                                  const uint32_t *rows, const void *vals, size_t nnz, const uint32_t *items,
                                  size_t n_items, const uint32_t *long_cols, size_t n_long, size_t n_partial,
                                  const void *out, size_t n_out) {
    if (n_rows > max_rows || nnz > 0xFFFFFFFFull || n_partial > 0x7FFFFFFFull || n_out > 0x7FFFFFFFull ||
        n_long > 0x7FFFFFFFull || n_items > 0xFFFFFFFFull)
        return VMPC_E_RANGE;
    if (!ctx || (n_out && !out) || (n_rows && !weights) || (nnz && (!rows || !vals)) || (n_items && !items) ||
        (n_long && !long_cols))
        return VMPC_E_INVAL;
    return VMPC_OK;
}

// checked arguments (fr_colsum_check); the partial sums live in the context arena.  zero_out: out is zeroed first,
// inside the stage and with an empty plan too, so that positions that no item writes are 0
template <class F>
static int fr_colsum(vmpc_ctx *ctx, const char *stage, bool zero_out, const void *weights, size_t n_rows,
                     const uint32_t *rows, const void *vals, size_t nnz, const uint32_t *items, size_t n_items,
                     const uint32_t *long_cols, size_t n_long, size_t n_partial, void *out, size_t n_out) {
    if (n_items == 0 && !zero_out) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    uint32_t *part = nullptr;
    if (n_items && n_partial) {
        VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(n_partial * 32) + 256));
        part = (uint32_t *)vmpc_ws_take(ctx, n_partial * 32);
    }
    vmpc_stage_scope sc(ctx, stage);
    if (zero_out && n_out) VMPC_HIP_CHECK(hipMemsetAsync(out, 0, n_out * 32, ctx->stream));
    if (n_items == 0) return VMPC_OK;
    k_fr_colsum<F><<<(unsigned)((n_items + FR_COLSUM_WG - 1) / FR_COLSUM_WG), FR_COLSUM_WG, 0, ctx->stream>>>(
        (const uint32_t *)weights, (uint32_t)n_rows, rows, (const uint32_t *)vals, nnz, items, n_items, part,
        (uint32_t)n_partial, (uint32_t *)out, (uint32_t)n_out);
    VMPC_KERNEL_CHECK();
    if (n_long) {
        k_fr_colfinish<F><<<(unsigned)n_long, FR_COLSUM_WG, 0, ctx->stream>>>(long_cols, part, (uint32_t)n_partial,
                                                                             (uint32_t *)out, (uint32_t)n_out);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}
