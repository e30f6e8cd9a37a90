// Pi_Nullity (AC20 p. 17-18, verifiable_mpc/ac20/nullity.py:21-40) over the Ed25519 scalar field GF(l) (csrc/fr.h): the
// "polynomial amortisation trick" L = sum_i rho^i L_i for s dense linear forms held as an s x n row-major matrix of
// 32-byte little-endian elements (row i at rows + 32 i row_stride), and the values L_i(x) of all of them at once.
//
//   vmpc_fr_rows_combine_dev  out[j] = sum_{i<s} rho^i rows[i][j]  (nullity.py:25, :32: s Python form products and
//                             sums).  A lane owns a column and runs Horner from row s-1 down: adjacent lanes read
//                             adjacent elements, so every row is read as one contiguous run, once.  The element is
//                             added into the unreduced 512-bit product acc * rho before the Barrett reduction, so ANY
//                             256-bit input is taken mod l on the way in at no cost.  Four rows are loaded ahead of
//                             the four dependent steps that consume them.
//                             When n < NL_FULL_LANES (65536 lanes: one 256-lane workgroup on each of the 256 CUs) and
//                             s >= 2 NL_MIN_SEG (32), the rows are cut into at most NL_FULL_LANES / n segments of at
//                             least NL_MIN_SEG rows; segment g is combined by the same Horner into partial row g, and
//                             a second launch of the SAME kernel combines the partial rows with rho^(segment length),
//                             which a one-lane kernel computes on the device.  No atomics, integer sums in a fixed
//                             order: deterministic.
//   vmpc_fr_rows_dot_dev      out[i] = sum_j rows[i][j] x[j] for every row, and the smallest i with out[i] != 0.
//                             Grid (rows, column segments) - the row is the fast grid dimension, so the workgroups
//                             that share a slice of x run together and find it in L2.  Products are added UNREDUCED into
//                             the wide accumulator of csrc/fr256.h (any 256-bit input is exact there), one Barrett
//                             reduction per lane; F256_ACC_MAX_PRODUCTS products fit before a carry counter can wrap
//                             and a lane adds at most NL_MAX_N, so the loop never reduces.  Lanes are added through LDS
//                             in a fixed tree, segments in a second launch in segment order.  The index comes from an
//                             atomicMin (an index: order does not matter); the values never touch an atomic.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): the table behind the kernels - no scratch.
#include "common.h"
#include "fr.h"

#define NL_WG 256
#define NL_MAX_S VMPC_FR_ROWS_MAX_S
#define NL_MAX_N VMPC_FR_ROWS_MAX_N
#define NL_FULL_LANES ((size_t)65536)   // below this many columns the direct kernel leaves CUs idle
#define NL_MIN_SEG 16                   // fewest rows per segment
#define NL_DOT_TARGET_WGS 2048

static_assert((uint64_t)NL_MAX_N < F256_ACC_MAX_PRODUCTS, "a lane of k_nl_dot would have to reduce inside its loop");

struct nl_arg {
    uint32_t v[8];
};

// element i of a vector, as it is in memory (no reduction)
__device__ __forceinline__ void nl_ld_raw(uint32_t w[8], const uint32_t *p, size_t i) {
    const uint4 *q = (const uint4 *)(p + 8 * i);
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// acc * rho + e mod l for acc, rho < l and ANY 256-bit e: the product is below l^2 < 2^506, the sum below 2^507
__device__ __forceinline__ fr nl_horner(const fr &acc, const fr &rho, const uint32_t e[8]) {
    uint32_t t[16];
    fr_mul_wide(t, acc, rho);
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        c += (uint64_t)t[i] + (i < 8 ? e[i] : 0u);
        t[i] = (uint32_t)c;
        c >>= 32;
    }
    return fr_reduce512(t);
}

// grid (column blocks, segments).  Segment g = rows [g seg_len, min(s, (g + 1) seg_len)) -> out row g (n elements):
// out[g n + j] = sum_k rho^k rows[(g seg_len + k) stride + j].  rho_mem != NULL: rho is read from there (8 words).
__global__ void __launch_bounds__(NL_WG)
k_nl_combine(const uint32_t *__restrict__ rows, uint32_t s, uint32_t n, size_t stride, nl_arg rho_arg,
             const uint32_t *__restrict__ rho_mem, uint32_t seg_len, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t lo = blockIdx.y * seg_len;
    const uint32_t hi = lo + seg_len < s ? lo + seg_len : s;
    fr rho;
#pragma unroll
    for (int k = 0; k < 8; k++) rho.v[k] = rho_mem ? rho_mem[k] : rho_arg.v[k];
    fr acc = fr_zero();
    uint32_t i = hi;
    for (; i >= lo + 4; i -= 4) {
        uint32_t e[4][8];
#pragma unroll
        for (int u = 0; u < 4; u++) nl_ld_raw(e[u], rows, (size_t)(i - 1 - u) * stride + j);
#pragma unroll
        for (int u = 0; u < 4; u++) acc = nl_horner(acc, rho, e[u]);
    }
    for (; i > lo; i--) {
        uint32_t e[8];
        nl_ld_raw(e, rows, (size_t)(i - 1) * stride + j);
        acc = nl_horner(acc, rho, e);
    }
    f256_st(out, (long long)blockIdx.y * n + j, acc);
}

// out = rho^e (one lane; e <= 2^16)
__global__ void k_nl_pow(nl_arg rho_arg, uint32_t e, uint32_t *__restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    fr rho;
#pragma unroll
    for (int k = 0; k < 8; k++) rho.v[k] = rho_arg.v[k];
    fr r = f256_one<fr>();
    for (int b = 31 - __clz(e | 1u); b >= 0; b--) {
        r = fr_mul(r, r);
        if ((e >> b) & 1u) r = fr_mul(r, rho);
    }
    f256_st(out, 0, r);
}

// the sum of the workgroup's 256 values, in a fixed tree; valid in thread 0
__device__ __forceinline__ fr nl_block_sum(uint32_t *lds, const fr &v) {
    f256_st(lds, threadIdx.x, v);
    __syncthreads();
    for (int h = NL_WG / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h)
            f256_st(lds, threadIdx.x, fr_add(f256_ld<fr>(lds, threadIdx.x), f256_ld<fr>(lds, threadIdx.x + h)));
        __syncthreads();
    }
    return f256_ld<fr>(lds, 0);
}

// grid (rows, column segments): partial[row n_segs + g] = sum over columns [g seg_len, min(n, (g + 1) seg_len))
__global__ void __launch_bounds__(NL_WG)
k_nl_dot(const uint32_t *__restrict__ rows, uint32_t n, size_t stride, const uint32_t *__restrict__ x, uint32_t seg_len,
         uint32_t *__restrict__ partial) {
    __shared__ uint32_t lds[NL_WG * 8];
    const uint32_t row = blockIdx.x, g = blockIdx.y;
    const uint32_t lo = g * seg_len;
    const uint32_t hi = n - lo < seg_len ? n : lo + seg_len;
    const uint32_t *r = rows + 8 * (size_t)row * stride;
    f256_acc acc = f256_acc_zero();
    for (uint32_t j = lo + threadIdx.x; j < hi; j += NL_WG) {
        uint32_t a[8], b[8];
        nl_ld_raw(a, r, j);
        nl_ld_raw(b, x, j);
        f256_acc_mac(acc, a, b);
    }
    const fr sum = nl_block_sum(lds, f256_acc_reduce<fr>(acc));
    if (threadIdx.x == 0) f256_st(partial, (long long)row * gridDim.y + g, sum);
}

// one workgroup per row: out[row] = the row's partial sums added in segment order (lane t takes t, t + 256, ..)
__global__ void __launch_bounds__(NL_WG)
k_nl_dot_sum(const uint32_t *__restrict__ partial, uint32_t n_segs, uint32_t *__restrict__ out,
             uint32_t *__restrict__ first_nonzero) {
    __shared__ uint32_t lds[NL_WG * 8];
    const uint32_t row = blockIdx.x;
    fr acc = fr_zero();
    for (uint32_t g = threadIdx.x; g < n_segs; g += NL_WG) acc = fr_add(acc, f256_ld<fr>(partial, (long long)row * n_segs + g));
    const fr sum = nl_block_sum(lds, acc);
    if (threadIdx.x == 0) {
        f256_st(out, row, sum);
        if (first_nonzero && !fr_is_zero(sum)) atomicMin(first_nonzero, row);   // an index: order does not matter
    }
}

// Resources:   kernel          VGPRs  scratch  LDS     waves / SIMD
//              k_nl_combine    100    0        0       4
//              k_nl_pow        5      0        0       8
//              k_nl_dot        76     0        8 KiB   6
//              k_nl_dot_sum    52     0        8 KiB   8

extern "C" int vmpc_fr_rows_combine_dev(vmpc_ctx *ctx, const void *rows, size_t s, size_t n, size_t row_stride,
                                        const uint8_t rho[32], void *out) {
    if (s > NL_MAX_S || n > NL_MAX_N || row_stride > NL_MAX_N) return VMPC_E_RANGE;
    if (!ctx || !rho || (n && !out) || (s && n && !rows) || (s > 1 && row_stride < n)) return VMPC_E_INVAL;
    nl_arg ra;
    memcpy(ra.v, rho, 32);
    if (fr_geq_l(ra.v)) return VMPC_E_NONCANON;
    if (n == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    if (s == 0) {
        VMPC_HIP_CHECK(hipMemsetAsync(out, 0, n * 32, ctx->stream));
        return VMPC_OK;
    }
    const unsigned col_blocks = (unsigned)((n + NL_WG - 1) / NL_WG);
    if (n >= NL_FULL_LANES || s < 2 * NL_MIN_SEG) {
        vmpc_stage_scope sc(ctx, "nl_combine");
        k_nl_combine<<<dim3(col_blocks, 1), NL_WG, 0, ctx->stream>>>((const uint32_t *)rows, (uint32_t)s, (uint32_t)n,
                                                                      row_stride, ra, nullptr, (uint32_t)s, (uint32_t *)out);
        VMPC_KERNEL_CHECK();
        return VMPC_OK;
    }
    // segments: as many as fill the chip, none shorter than NL_MIN_SEG rows
    size_t n_segs = (NL_FULL_LANES + n - 1) / n;
    if (n_segs > s / NL_MIN_SEG) n_segs = s / NL_MIN_SEG;
    const size_t seg_len = (s + n_segs - 1) / n_segs;
    n_segs = (s + seg_len - 1) / seg_len;
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(n_segs * n * 32) + 512));
    uint32_t *partial = (uint32_t *)vmpc_ws_take(ctx, n_segs * n * 32);
    uint32_t *rho_seg = (uint32_t *)vmpc_ws_take(ctx, 32);
    vmpc_stage_scope sc(ctx, "nl_combine_seg");
    k_nl_pow<<<1, 64, 0, ctx->stream>>>(ra, (uint32_t)seg_len, rho_seg);
    VMPC_KERNEL_CHECK();
    k_nl_combine<<<dim3(col_blocks, (unsigned)n_segs), NL_WG, 0, ctx->stream>>>(
        (const uint32_t *)rows, (uint32_t)s, (uint32_t)n, row_stride, ra, nullptr, (uint32_t)seg_len, partial);
    VMPC_KERNEL_CHECK();
    k_nl_combine<<<dim3(col_blocks, 1), NL_WG, 0, ctx->stream>>>(partial, (uint32_t)n_segs, (uint32_t)n, n, ra, rho_seg,
                                                                  (uint32_t)n_segs, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_fr_rows_dot_dev(vmpc_ctx *ctx, const void *rows, size_t s, size_t n, size_t row_stride, const void *x,
                                    void *out, uint32_t *first_nonzero) {
    if (s > NL_MAX_S || n > NL_MAX_N || row_stride > NL_MAX_N) return VMPC_E_RANGE;
    if (!ctx || (s && !out) || (s && n && (!rows || !x)) || (s > 1 && row_stride < n)) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "nl_dot");
    if (first_nonzero) VMPC_HIP_CHECK(hipMemsetAsync(first_nonzero, 0xFF, 4, ctx->stream));
    if (s == 0) return VMPC_OK;
    if (n == 0) {
        VMPC_HIP_CHECK(hipMemsetAsync(out, 0, s * 32, ctx->stream));
        return VMPC_OK;
    }
    // column segments across workgroups when there are few rows: about NL_DOT_TARGET_WGS workgroups in all, each
    // lane of a segment with at least one column
    size_t n_segs = NL_DOT_TARGET_WGS / s;
    if (n_segs < 1) n_segs = 1;
    if (n_segs > (n + NL_WG - 1) / NL_WG) n_segs = (n + NL_WG - 1) / NL_WG;
    size_t seg_len = (n + n_segs - 1) / n_segs;
    seg_len = (seg_len + NL_WG - 1) / NL_WG * NL_WG;
    n_segs = (n + seg_len - 1) / seg_len;
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(s * n_segs * 32) + 256));
    uint32_t *partial = (uint32_t *)vmpc_ws_take(ctx, s * n_segs * 32);
    k_nl_dot<<<dim3((unsigned)s, (unsigned)n_segs), NL_WG, 0, ctx->stream>>>((const uint32_t *)rows, (uint32_t)n, row_stride,
                                                                             (const uint32_t *)x, (uint32_t)seg_len, partial);
    VMPC_KERNEL_CHECK();
    k_nl_dot_sum<<<(unsigned)s, NL_WG, 0, ctx->stream>>>(partial, (uint32_t)n_segs, (uint32_t *)out, first_nonzero);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
