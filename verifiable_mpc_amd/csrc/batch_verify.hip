// The scalar side of a BATCH of compact Protocol-4/5 verifications (compressed_pivot.py protocol_5_verifier_batch,
// DESIGN.md section 17).  Proof p has round challenges c_{p,i} (i < R), a final response z'_p of 2^lb elements and a
// verifier-chosen weight w_p; with N = 2^(R + lb)
//     v_p[j] = z'_p[j mod 2^lb] * prod_{i<R} (c_{p,i} if bit (lb + R - 1 - i) of j is 0 else 1)
// are the scalars of its final check as ONE N-term MSM (csrc/frvec.hip k_fr_challenge_products).  K proofs over one
// CRS share that MSM:
//     u[j]    = sum_p w_p v_p[j]                            vmpc_fr_batch_products_dev: u_out, N residues
//     dots[p] = sum_{j < form_len} w_p v_p[j] forms[p][j]                                 dots_out, K residues
// No v_p is ever written to memory.  The index is cut at bit b = R + lb - a, a = min(R, (R + lb) / 2):
//     w_p v_p[j] = hi_p[j >> b] * lo_p[j & (2^b - 1)]
//     hi_p[s] = w_p  prod_{i<a}      (c_{p,i} if bit (a - 1 - i)       of s is 0 else 1)          2^a entries
//     lo_p[t] = z'_p[t mod 2^lb] prod_{a<=i<R} (c_{p,i} if bit (lb + R - 1 - i) of t is 0 else 1)   2^b entries
// - about 2 sqrt(N) entries per proof (64 KiB at N = 2^20) instead of N, built by doubling at ONE product per entry
// instead of up to R:
//   k_bv_tables  grid (2, K): workgroup (0, p) builds hi_p, (1, p) builds lo_p, level by level in place (a level copies
//                the table up and multiplies the lower copy by the level's challenge); hi_p is written a second time
//                TRANSPOSED (hiT[s K + p]) so that k_bv_u reads the K values of a row as one contiguous run.
//   k_bv_u       a workgroup owns 256 columns of ONE hi row, a lane one column: K products hi_p[row] * lo_p[t] added
//                UNREDUCED into the wide accumulator of csrc/fr256.h, one Barrett reduction per column.  The hi operand
//                is the same for every lane of the workgroup, so it is read through the scalar cache into SGPRs (a
//                broadcast that costs no LDS and no vector registers); the lo operand is lane-private (adjacent lanes
//                read adjacent elements), so staging it in LDS would only copy it.
//   k_bv_dot     grid (column blocks x row segments, K).  dots[p] = sum_t lo_p[t] (sum_s hi_p[s] forms[p][s 2^b + t]):
//                a lane owns t and runs over the rows s of its segment - hi_p[s] is again uniform (SGPRs), the form is
//                read row by row in contiguous runs of 256 elements, each element once - adding unreduced; then ONE
//                reduction and ONE product by lo_p[t] per lane, never a triple product.  Lanes are added through LDS in
//                a fixed tree, the segments by k_bv_dot_sum in segment order: no atomics, bit-reproducible.
// Every operand (challenges, z', weights, forms) must be a canonical residue < l, as for the other entries of
// csrc/frvec.hip; results are canonical.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): the table behind the kernels - no scratch.
#include "common.h"
#include "fr.h"

#define BV_WG 256
#define BV_TAB_WG 1024
#define BV_MAX_K VMPC_FR_BATCH_MAX_K
#define BV_MAX_ROUNDS VMPC_FR_BATCH_MAX_ROUNDS
#define BV_MAX_BITS VMPC_FR_BATCH_MAX_BITS
#define BV_DOT_TARGET_WGS 2048
#define BV_DOT_MIN_ROWS 16          // fewest hi rows per segment of k_bv_dot

static_assert((uint64_t)BV_MAX_K < F256_ACC_MAX_PRODUCTS, "a lane of k_bv_u would have to reduce inside its loop");
static_assert(((uint64_t)1 << BV_MAX_ROUNDS) < F256_ACC_MAX_PRODUCTS, "a lane of k_bv_dot would have to reduce inside its loop");
static_assert(BV_MAX_ROUNDS <= BV_MAX_BITS && BV_MAX_BITS <= 30, "32-bit column indices");

// element i of a vector, as it is in memory
__device__ __forceinline__ void bv_ld_raw(uint32_t w[8], const uint32_t *p, size_t i) {
    const uint4 *q = (const uint4 *)(p + 8 * i);
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// the same through a pointer that was itself read from memory (forms[p]): the compiler cannot see that it points into
// device memory and would emit flat loads; the address space is stated here
__device__ __forceinline__ void bv_ld_raw_global(uint32_t w[8], const uint32_t *p, size_t i) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4 *gptr;
    const gptr q = (gptr)(p + 8 * i);
    const u32x4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// one doubling level of a table of 2^m entries: T[s + 2^m] = T[s], T[s] = T[s] * c
__device__ __forceinline__ void bv_double(uint32_t *T, int m, const fr &c) {
    const uint32_t half = 1u << m;
    for (uint32_t s = threadIdx.x; s < half; s += BV_TAB_WG) {
        const fr x = f256_ld<fr>(T, s);
        f256_st(T, (long long)s + half, x);
        f256_st(T, s, fr_mul(x, c));
    }
    __syncthreads();
}

// grid (2, K).  hi: K x 2^a, lo: K x 2^b, hiT: 2^a x K
__global__ void __launch_bounds__(BV_TAB_WG)
k_bv_tables(int K, int R, int lb, int a, const uint32_t *__restrict__ chal, const uint32_t *__restrict__ zprime,
            const uint32_t *__restrict__ weights, uint32_t *hi, uint32_t *lo, uint32_t *hiT) {
    const int p = blockIdx.y;
    const int b = R + lb - a;
    const uint32_t *c = chal + 8 * (size_t)p * R;
    if (blockIdx.x == 0) {
        uint32_t *T = hi + 8 * ((size_t)p << a);
        if (threadIdx.x == 0) f256_st(T, 0, f256_ld<fr>(weights, p));
        __syncthreads();
        // bit m of s is bit (a - 1 - i) for challenge i = a - 1 - m
        for (int m = 0; m < a; m++) bv_double(T, m, f256_ld<fr>(c, a - 1 - m));
        for (uint32_t s = threadIdx.x; s < (1u << a); s += BV_TAB_WG) f256_st(hiT, (long long)s * K + p, f256_ld<fr>(T, s));
    } else {
        uint32_t *T = lo + 8 * ((size_t)p << b);
        for (uint32_t t = threadIdx.x; t < (1u << lb); t += BV_TAB_WG) f256_st(T, t, f256_ld<fr>(zprime, ((long long)p << lb) + t));
        __syncthreads();
        // bit m of t is bit (lb + R - 1 - i) for challenge i = lb + R - 1 - m (i runs from R - 1 down to a)
        for (int m = lb; m < b; m++) bv_double(T, m, f256_ld<fr>(c, lb + R - 1 - m));
    }
}

// grid (2^a * col_blocks): workgroup -> (row, block of 256 columns of that row)
__global__ void __launch_bounds__(BV_WG)
k_bv_u(int K, int b, uint32_t col_blocks, const uint32_t *__restrict__ hiT, const uint32_t *__restrict__ lo,
       uint32_t *__restrict__ u) {
    const uint32_t row = blockIdx.x / col_blocks;
    const uint32_t t = (blockIdx.x % col_blocks) * BV_WG + threadIdx.x;
    if (t >= (1u << b)) return;
    const uint32_t *h = hiT + 8 * (size_t)row * K;      // K contiguous elements, the same for the whole workgroup
    f256_acc acc = f256_acc_zero();
    int p = 0;
    for (; p + 4 <= K; p += 4) {
        uint32_t e[4][8];
#pragma unroll
        for (int q = 0; q < 4; q++) bv_ld_raw(e[q], lo, ((size_t)(p + q) << b) + t);
#pragma unroll
        for (int q = 0; q < 4; q++) f256_acc_mac(acc, h + 8 * (p + q), e[q]);
    }
    for (; p < K; p++) {
        uint32_t e[8];
        bv_ld_raw(e, lo, ((size_t)p << b) + t);
        f256_acc_mac(acc, h + 8 * p, e);
    }
    f256_st(u, ((long long)row << b) + t, f256_acc_reduce<fr>(acc));
}

// the sum of the workgroup's 256 values, in a fixed tree; valid in thread 0
__device__ __forceinline__ fr bv_block_sum(uint32_t *lds, const fr &v) {
    f256_st(lds, threadIdx.x, v);
    __syncthreads();
    for (int h = BV_WG / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h)
            f256_st(lds, threadIdx.x, fr_add(f256_ld<fr>(lds, threadIdx.x), f256_ld<fr>(lds, threadIdx.x + h)));
        __syncthreads();
    }
    return f256_ld<fr>(lds, 0);
}

// grid (col_blocks * row_segs, K): partial[p n_segs + seg], seg = row segment * col_blocks + column block, is the sum
// over the rows [g seg_rows, min(rows, (g + 1) seg_rows)) and the block's 256 columns.  rows = the hi rows that hold an
// element below form_len.
__global__ void __launch_bounds__(BV_WG)
k_bv_dot(int a, int b, uint32_t col_blocks, uint32_t rows, uint32_t seg_rows, const uint32_t *__restrict__ hi,
         const uint32_t *__restrict__ lo, const uint32_t *const *__restrict__ forms, uint32_t form_len,
         uint32_t *__restrict__ partial) {
    __shared__ uint32_t lds[BV_WG * 8];
    const uint32_t p = blockIdx.y;
    const uint32_t g = blockIdx.x / col_blocks;
    const uint32_t t = (blockIdx.x % col_blocks) * BV_WG + threadIdx.x;
    const bool live = t < (1u << b);
    const uint32_t r0 = g * seg_rows;
    const uint32_t r1 = rows - r0 < seg_rows ? rows : r0 + seg_rows;
    const uint32_t *h = hi + 8 * ((size_t)p << a);       // 2^a contiguous elements, uniform
    const uint32_t *f = forms[p];
    f256_acc acc = f256_acc_zero();
    if (live) {
        uint32_t s = r0;
        for (; s + 4 <= r1; s += 4) {
            uint32_t e[4][8];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t j = ((s + q) << b) + t;      // < 2^30
                if (j < form_len) {
                    bv_ld_raw_global(e[q], f, j);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++) e[q][k] = 0;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) f256_acc_mac(acc, h + 8 * (size_t)(s + q), e[q]);
        }
        for (; s < r1; s++) {
            const uint32_t j = (s << b) + t;
            if (j < form_len) {
                uint32_t e[8];
                bv_ld_raw_global(e, f, j);
                f256_acc_mac(acc, h + 8 * (size_t)s, e);
            }
        }
    }
    fr v = fr_zero();
    if (live) v = fr_mul(f256_acc_reduce<fr>(acc), f256_ld<fr>(lo, ((long long)p << b) + t));
    const fr sum = bv_block_sum(lds, v);
    if (threadIdx.x == 0) f256_st(partial, (long long)p * gridDim.x + blockIdx.x, sum);
}

// one workgroup per proof: dots[p] = its partial sums added in segment order (lane t takes t, t + 256, ..)
__global__ void __launch_bounds__(BV_WG)
k_bv_dot_sum(const uint32_t *__restrict__ partial, uint32_t n_segs, uint32_t *__restrict__ dots) {
    __shared__ uint32_t lds[BV_WG * 8];
    const uint32_t p = blockIdx.x;
    fr acc = fr_zero();
    for (uint32_t g = threadIdx.x; g < n_segs; g += BV_WG) acc = fr_add(acc, f256_ld<fr>(partial, (long long)p * n_segs + g));
    const fr sum = bv_block_sum(lds, acc);
    if (threadIdx.x == 0) f256_st(dots, p, sum);
}

// Resources:   kernel          VGPRs  SGPRs  scratch  LDS     waves / SIMD
//              k_bv_tables     72     66     0        0       7 (1024-lane workgroups)
//              k_bv_u          78     50     0        0       6
//              k_bv_dot        120    46     0        8 KiB   4
//              k_bv_dot_sum    52     29     0        8 KiB   8

extern "C" int vmpc_fr_batch_products_dev(vmpc_ctx *ctx, int K, int rounds, int low_bits, const void *challenges_dev,
                                          const void *zprime_dev, const void *weights_dev, const void *const *forms_dev,
                                          size_t form_len, void *u_out, void *dots_out) {
    if (K > BV_MAX_K || rounds > BV_MAX_ROUNDS || low_bits > BV_MAX_BITS || (long long)rounds + low_bits > BV_MAX_BITS)
        return VMPC_E_RANGE;
    if (!ctx || K < 1 || rounds < 0 || low_bits < 0 || (rounds && !challenges_dev) || !zprime_dev || !weights_dev ||
        !u_out || !dots_out)
        return VMPC_E_INVAL;
    const int bits = rounds + low_bits;
    const size_t N = (size_t)1 << bits;
    if (form_len > N || (form_len && !forms_dev)) return VMPC_E_INVAL;
    const int a = rounds < bits / 2 ? rounds : bits / 2;
    const int b = bits - a;
    const size_t n_hi = (size_t)1 << a, n_lo = (size_t)1 << b;
    const uint32_t col_blocks = (uint32_t)((n_lo + BV_WG - 1) / BV_WG);
    // k_bv_dot: the hi rows that reach below form_len, cut into segments of at least BV_DOT_MIN_ROWS rows while that
    // still adds workgroups below the target
    const uint32_t rows = (uint32_t)((form_len + n_lo - 1) >> b);
    size_t row_segs = BV_DOT_TARGET_WGS / ((size_t)K * col_blocks);
    if (row_segs > rows / BV_DOT_MIN_ROWS) row_segs = rows / BV_DOT_MIN_ROWS;
    if (row_segs < 1) row_segs = 1;
    const uint32_t seg_rows = rows ? (uint32_t)((rows + row_segs - 1) / row_segs) : 1;
    row_segs = rows ? (rows + seg_rows - 1) / seg_rows : 1;
    const size_t n_segs = row_segs * col_blocks;

    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t hi_bytes = (size_t)K * n_hi * 32, lo_bytes = (size_t)K * n_lo * 32, part_bytes = (size_t)K * n_segs * 32;
    VMPC_CHECK(vmpc_ws_reserve(ctx, 2 * vmpc_align(hi_bytes) + vmpc_align(lo_bytes) + vmpc_align(part_bytes) + 1024));
    uint32_t *hi = (uint32_t *)vmpc_ws_take(ctx, hi_bytes);
    uint32_t *hiT = (uint32_t *)vmpc_ws_take(ctx, hi_bytes);
    uint32_t *lo = (uint32_t *)vmpc_ws_take(ctx, lo_bytes);
    uint32_t *partial = (uint32_t *)vmpc_ws_take(ctx, part_bytes);
    {
        vmpc_stage_scope s(ctx, "bv_tables");
        k_bv_tables<<<dim3(2, (unsigned)K), BV_TAB_WG, 0, ctx->stream>>>(K, rounds, low_bits, a, (const uint32_t *)challenges_dev,
                                                                         (const uint32_t *)zprime_dev,
                                                                         (const uint32_t *)weights_dev, hi, lo, hiT);
        VMPC_KERNEL_CHECK();
    }
    {
        vmpc_stage_scope s(ctx, "bv_u");
        k_bv_u<<<(unsigned)(n_hi * col_blocks), BV_WG, 0, ctx->stream>>>(K, b, col_blocks, hiT, lo, (uint32_t *)u_out);
        VMPC_KERNEL_CHECK();
    }
    {
        vmpc_stage_scope s(ctx, "bv_dots");
        if (rows == 0) {
            VMPC_HIP_CHECK(hipMemsetAsync(dots_out, 0, (size_t)K * 32, ctx->stream));
        } else {
            k_bv_dot<<<dim3((unsigned)n_segs, (unsigned)K), BV_WG, 0, ctx->stream>>>(
                a, b, col_blocks, rows, seg_rows, hi, lo, (const uint32_t *const *)forms_dev, (uint32_t)form_len, partial);
            VMPC_KERNEL_CHECK();
            k_bv_dot_sum<<<(unsigned)K, BV_WG, 0, ctx->stream>>>(partial, (uint32_t)n_segs, (uint32_t *)dots_out);
            VMPC_KERNEL_CHECK();
        }
    }
    return VMPC_OK;
}
