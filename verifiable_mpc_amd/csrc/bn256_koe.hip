// The scalar side of the knowledge-of-exponent pivot over BN-256 (AC20 section 9,
// verifiable_mpc/ac20/knowledge_of_exponent.py): arithmetic in GF(n), n the group order (csrc/fr_bn.h).
//
//   k_frbn_polymul   c = a * b for two coefficient vectors: the prover's c_poly_lhs * c_poly_rhs
//                    (knowledge_of_exponent.py:121-123; qap_creator.Poly.__mul__ is O(n^2) Python).  n - 1 = 2^5 * odd, so
//                    there is no NTT of useful length in this field; the product is the schoolbook one.  (The INTEGERS
//                    have one: csrc/bn256_ntt.hip convolves modulo 18 NTT-friendly primes and rebuilds the same
//                    canonical residues; koe_poly_mul hands a product over when the context's mode asks for it,
//                    vmpc_ctx_set_poly_product - off by default.)
//   k_frbn_powers    scale * z^(i+1): the exponents of the trusted setup (knowledge_of_exponent.py:52-66 reaches them by
//                    2n sequential scalar multiplications of a point).
//   k_koe_stage      the product's operands (gamma, x) and L reversed from a witness and a form in device memory, and
//   k_koe_split      c[n] out of the product and zeroed in place: the opening of Protocol 8's L over BN-256 never
//                    passes z or L through the host.
//   k_koe_stage_batch  the same two for K openings of one length in one launch each: the operands as rows of matrices (the
//   k_koe_split_batch  witness on the grid's y, one gamma per row from device memory), the K coefficients n taken out by
//                      one lane per witness (vmpc_bn256_koe_stage_batch_dev, _split_batch_dev: the batch prover of
//                      DESIGN.md section 32).  The single entries keep their own kernels.
//
// Product kernel: the output-stationary tile of csrc/fr_conv.h over one SEGMENT of the index i of a.  The triangle
// (tiles near k = n meet the whole of a, tiles at the ends almost nothing) is balanced by the segments: a tile is cut
// into as many workgroups as its i-range has segments; their partial sums (reduced mod n) go to the context arena and
// k_frbn_polysum adds them.  A product whose tiles all fit one segment is written straight to `out`.
//
// The kernel takes K products a_w * b_w of one shape (grid z = w; a stride of 0 between the b rows: one b for all)
// and a WINDOW [k_lo, k_lo + k_cnt) of the outputs: only the tiles that meet the window are launched and only the window
// is written, at out_w[k - k_lo].  The segment length counts K, so a large batch ends at one or two partial sums per
// output (vmpc_bn256_fr_poly_mul_batch_dev; the two half products of csrc/bn256_qap_h.hip's h).
// vmpc_bn256_fr_poly_mul_dev is the whole window of one product: both entries call koe_poly_mul.
#include "common.h"
#include "fr_bn.h"
#include "fr_conv.h"

#define KOE_MIN_SEG 256                   // shortest segment; a multiple of FR_CONV_CHUNK
#define KOE_TARGET_WGS (1 << 12)          // full-size workgroups a large product is cut into

// [first, last] of the i that tile k0 meets, and how many segments of length seg that range touches
struct koe_span {
    long long lo, hi;
    unsigned first_seg, n_seg;
};
__host__ __device__ static inline koe_span koe_tile_span(long long k0, long long na, long long nb, long long seg) {
    koe_span s;
    s.lo = k0 - (nb - 1) > 0 ? k0 - (nb - 1) : 0;
    s.hi = k0 + FR_CONV_TILE - 1 < na - 1 ? k0 + FR_CONV_TILE - 1 : na - 1;
    s.first_seg = (unsigned)(s.lo / seg);
    s.n_seg = (unsigned)(s.hi / seg) - s.first_seg + 1;
    return s;
}

// grid (tiles of the window, most segments of a tile, products).  Tile x covers the outputs (tile_lo + x) FR_CONV_TILE ..;
// output k of product w and segment y goes to dst[w wit_stride + y seg_stride + k - base_k] if k is in the window
// [k_lo, k_hi).  Straight to `out`: seg_stride = 0 (one segment), base_k = k_lo, wit_stride = the caller's row stride.
__global__ void __launch_bounds__(FR_CONV_TILE)
k_frbn_polymul(const uint32_t *__restrict__ a, size_t a_stride, long long na, const uint32_t *__restrict__ b,
               size_t b_stride, long long nb, long long seg, unsigned tile_lo, long long k_lo, long long k_hi,
               long long base_k, uint32_t *__restrict__ dst, size_t wit_stride, size_t seg_stride) {
    __shared__ uint32_t sA[1][FR_CONV_CHUNK * 8];
    __shared__ uint32_t sB[8 * FR_CONV_BROW];
    const long long k0 = (long long)(tile_lo + blockIdx.x) * FR_CONV_TILE;
    const koe_span span = koe_tile_span(k0, na, nb, seg);
    if (blockIdx.y >= span.n_seg) return;      // (uniform) this tile has fewer segments
    const size_t w = blockIdx.z;
    const long long seg_lo = (long long)(span.first_seg + blockIdx.y) * seg;
    const uint32_t *const av[1] = {a + 8 * w * a_stride};
    const uint32_t *bw = b + 8 * w * b_stride;
    f256_acc acc[1] = {f256_acc_zero()};
    for (long long i0 = seg_lo; i0 < seg_lo + seg; i0 += FR_CONV_CHUNK) {
        if (i0 + FR_CONV_CHUNK <= span.lo || i0 > span.hi) continue;   // (uniform)
        fr_conv_chunk<frbn, 1>(sA, sB, acc, av, na, bw, nb, k0, i0);
    }
    const long long k = k0 + threadIdx.x;
    if (k >= k_lo && k < k_hi)
        frbn_store(dst + 8 * (w * wit_stride + blockIdx.y * seg_stride + (size_t)(k - base_k)), frbn_acc_reduce(acc[0]));
}

// grid (window outputs, products): out_w[k - k_lo] = the sum of tile (k / FR_CONV_TILE)'s partial sums at k
__global__ void __launch_bounds__(256)
k_frbn_polysum(const uint32_t *__restrict__ part, size_t wit_stride, size_t seg_stride, long long base_k, long long na,
               long long nb, long long seg, long long k_lo, long long k_hi, uint32_t *__restrict__ out,
               size_t out_stride) {
    const long long k = k_lo + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= k_hi) return;
    const size_t w = blockIdx.y;
    const koe_span span = koe_tile_span(k / FR_CONV_TILE * FR_CONV_TILE, na, nb, seg);
    f256_st(out + 8 * w * out_stride, k - k_lo,
            fr_partsum<frbn>(part + 8 * w * wit_stride, (long long)seg_stride, span.n_seg, k - base_k));
}

// lane g writes out[8g .. 8g+7]: z^(8g+1) by square-and-multiply on the index, then seven products by z
#define KOE_POW_RUN 8
__global__ void __launch_bounds__(256)
k_frbn_powers(const uint32_t *__restrict__ z_in, const uint32_t *__restrict__ scale_in, size_t count,
              uint32_t *__restrict__ out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t first = g * KOE_POW_RUN;
    if (first >= count) return;
    const frbn z = frbn_load(z_in);
    frbn v = frbn_load(scale_in), sq = z;
    for (size_t e = first + 1; e; e >>= 1) {
        if (e & 1) v = frbn_mul(v, sq);
        sq = frbn_mul(sq, sq);
    }
    const size_t last = first + KOE_POW_RUN < count ? first + KOE_POW_RUN : count;
    for (size_t i = first; i < last; i++) {
        frbn_store(out + 8 * i, v);
        v = frbn_mul(v, z);
    }
}

// The plan of a product: the tiles that meet the window; the segment length, a power of two that cuts the na * nb * K
// products into about KOE_TARGET_WGS workgroups' worth (more products, longer segments - fewer partial sums each) and
// stops once a segment holds the whole of a; the arena
struct koe_batch_plan {
    long long seg;
    unsigned tile_lo, tiles, max_segs;
    size_t cols, bytes;      // scalars per partial-sum row (the launched tiles' outputs); arena bytes (0: none needed)
};

static koe_batch_plan koe_batch_plan_of(size_t na, size_t nb, size_t k_lo, size_t k_cnt, size_t n_wit) {
    koe_batch_plan p;
    p.tile_lo = (unsigned)(k_lo / FR_CONV_TILE);
    p.tiles = (unsigned)((k_lo + k_cnt - 1) / FR_CONV_TILE) - p.tile_lo + 1;
    p.seg = KOE_MIN_SEG;
    while (p.seg < (long long)na &&
           p.seg * 2 * FR_CONV_TILE * KOE_TARGET_WGS <= (long long)na * (long long)nb * (long long)n_wit)
        p.seg *= 2;
    p.max_segs = 1;
    for (unsigned t = 0; t < p.tiles; t++) {
        const unsigned s =
            koe_tile_span((long long)(p.tile_lo + t) * FR_CONV_TILE, (long long)na, (long long)nb, p.seg).n_seg;
        if (s > p.max_segs) p.max_segs = s;
    }
    p.cols = (size_t)p.tiles * FR_CONV_TILE;
    p.bytes = p.max_segs > 1 ? vmpc_align(n_wit * p.max_segs * p.cols * 32) + 256 : 0;
    return p;
}

// n_wit >= 1 products of a non-empty window, checked by the entries
static int koe_poly_mul(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na, const void *b, size_t b_stride, size_t nb,
                        size_t k_lo, size_t k_cnt, void *out, size_t out_stride, size_t n_wit) {
    if (ctx->poly_product == VMPC_POLY_PRODUCT_NTT ||
        (ctx->poly_product == VMPC_POLY_PRODUCT_AUTO && (na < nb ? na : nb) >= VMPC_BN256_FR_NTT_MIN))
        return vmpc_ntt_poly_mul(ctx, a, a_stride, na, b, b_stride, nb, k_lo, k_cnt, out, out_stride, n_wit);
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const koe_batch_plan p = koe_batch_plan_of(na, nb, k_lo, k_cnt, n_wit);
    const long long lo = (long long)k_lo, hi = (long long)(k_lo + k_cnt);
    const long long base = p.max_segs > 1 ? (long long)p.tile_lo * FR_CONV_TILE : lo;
    const size_t wit_stride = p.max_segs > 1 ? p.max_segs * p.cols : out_stride;
    uint32_t *dst = (uint32_t *)out;
    if (p.max_segs > 1) {
        VMPC_CHECK(vmpc_ws_reserve(ctx, p.bytes));      // before any launch
        dst = (uint32_t *)vmpc_ws_take(ctx, n_wit * p.max_segs * p.cols * 32);
    }
    {
        vmpc_stage_scope s(ctx, "bn_fr_poly_mul");
        k_frbn_polymul<<<dim3(p.tiles, p.max_segs, (unsigned)n_wit), FR_CONV_TILE, 0, ctx->stream>>>(
            (const uint32_t *)a, a_stride, (long long)na, (const uint32_t *)b, b_stride, (long long)nb, p.seg, p.tile_lo, lo,
            hi, base, dst, wit_stride, p.max_segs > 1 ? p.cols : 0);
        VMPC_KERNEL_CHECK();
    }
    if (p.max_segs > 1) {
        vmpc_stage_scope s(ctx, "bn_fr_poly_sum");
        k_frbn_polysum<<<dim3((unsigned)((k_cnt + 255) / 256), (unsigned)n_wit), 256, 0, ctx->stream>>>(
            dst, wit_stride, p.cols, base, (long long)na, (long long)nb, p.seg, lo, hi, (uint32_t *)out, out_stride);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

// the whole product: the window [0, na + nb - 1) of one pair
extern "C" int vmpc_bn256_fr_poly_mul_dev(vmpc_ctx *ctx, const void *a, size_t na, const void *b, size_t nb,
                                          void *out) {
    if (na > VMPC_BN256_FR_POLY_MAX || nb > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !out || na == 0 || nb == 0) return VMPC_E_INVAL;
    return koe_poly_mul(ctx, a, na, na, b, nb, nb, 0, na + nb - 1, out, na + nb - 1, 1);
}

static bool koe_batch_in_range(size_t na, size_t nb, size_t k_lo, size_t k_cnt, size_t n_wit) {
    return n_wit <= VMPC_BN256_QAP_MAX_WIT && na <= VMPC_BN256_FR_POLY_MAX && nb <= VMPC_BN256_FR_POLY_MAX &&
           k_lo <= 2 * VMPC_BN256_FR_POLY_MAX && k_cnt <= 2 * VMPC_BN256_FR_POLY_MAX &&
           (k_cnt == 0 || k_lo + k_cnt + 1 <= na + nb);
}

extern "C" size_t vmpc_bn256_fr_poly_mul_batch_bytes(size_t na, size_t nb, size_t k_lo, size_t k_cnt, size_t n_wit) {
    if (!koe_batch_in_range(na, nb, k_lo, k_cnt, n_wit) || na == 0 || nb == 0 || k_cnt == 0 || n_wit == 0) return 0;
    return koe_batch_plan_of(na, nb, k_lo, k_cnt, n_wit).bytes;
}

extern "C" int vmpc_bn256_fr_poly_mul_batch_dev(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na, const void *b,
                                                size_t b_stride, size_t nb, size_t k_lo, size_t k_cnt, void *out,
                                                size_t out_stride, size_t n_wit) {
    const size_t cap = (size_t)1 << 31;
    if (!koe_batch_in_range(na, nb, k_lo, k_cnt, n_wit) || a_stride > cap || b_stride > cap || out_stride > cap ||
        (n_wit && (a_stride < na || (b_stride && b_stride < nb) || out_stride < k_cnt)))
        return VMPC_E_RANGE;
    if (!ctx || !a || !b || !out || na == 0 || nb == 0) return VMPC_E_INVAL;
    if (n_wit == 0 || k_cnt == 0) return VMPC_OK;
    return koe_poly_mul(ctx, a, a_stride, na, b, b_stride, nb, k_lo, k_cnt, out, out_stride, n_wit);
}

// ---- the opening's operands and result, device to device ----------------------------------------------------------------
// lhs = (gamma, x_0, .., x_{n-1}) and rhs = (L_{n-1}, .., L_0): the two polynomials of knowledge_of_exponent.py:116-123
// from a witness and a form that are already in device memory.  Thread i < n writes lhs[i + 1] and rhs[n - 1 - i], thread
// n writes lhs[0]; either output may be left out (the verifier wants the reversed form only).
struct koe_scalar_arg {
    uint32_t v[8];
};
__global__ void __launch_bounds__(256)
k_koe_stage(const uint32_t *__restrict__ x, koe_scalar_arg gamma, const uint32_t *__restrict__ L, size_t n,
            uint32_t *__restrict__ lhs, uint32_t *__restrict__ rhs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        if (lhs) f256_st(lhs, (long long)i + 1, f256_ld<frbn>(x, (long long)i));
        if (rhs) f256_st(rhs, (long long)(n - 1 - i), f256_ld<frbn>(L, (long long)i));
    } else if (i == n && lhs) {
        f256_st(lhs, 0, f256_copy<frbn>(gamma.v));
    }
}

// u[0] = c[n], then c[n] = 0: the opened value leaves the product and the MSM over the 2n generators skips its place
// (knowledge_of_exponent.py:124-130)
__global__ void k_koe_split(uint32_t *__restrict__ c, size_t n, uint32_t *__restrict__ u) {
    f256_st(u, 0, f256_ld<frbn>(c, (long long)n));
    f256_st(c, (long long)n, frbn_zero());
}

extern "C" int vmpc_bn256_koe_stage_dev(vmpc_ctx *ctx, const void *x, const uint8_t gamma[32], const void *L, size_t n,
                                        void *lhs, void *rhs) {
    if (n > VMPC_BN256_FR_POLY_MAX - 1) return VMPC_E_RANGE;
    if (!ctx || (!lhs && !rhs) || (lhs && (!gamma || (n && !x))) || (rhs && n && !L)) return VMPC_E_INVAL;
    koe_scalar_arg g = {};
    if (lhs) {
        memcpy(g.v, gamma, 32);
        if (!f256_is_canonical<frbn>(g.v)) return VMPC_E_NONCANON;
    }
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope s(ctx, "bn_koe_stage");
    k_koe_stage<<<(unsigned)((n + 1 + 255) / 256), 256, 0, ctx->stream>>>((const uint32_t *)x, g, (const uint32_t *)L, n,
                                                                         (uint32_t *)lhs, (uint32_t *)rhs);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_koe_split_dev(vmpc_ctx *ctx, void *c, size_t n, void *u_out) {
    if (n > VMPC_BN256_FR_POLY_MAX - 1) return VMPC_E_RANGE;
    if (!ctx || !c || !u_out || n == 0) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope s(ctx, "bn_koe_split");
    k_koe_split<<<1, 1, 0, ctx->stream>>>((uint32_t *)c, n, (uint32_t *)u_out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

// ---- the same for K openings of one length ----------------------------------------------------------
// grid (n + 1 lanes, witnesses): witness p reads row p of x and of L and gammas[p], and writes row p of lhs and of rhs (all
// strides in scalars).  x NULL: no lhs; L NULL: no rhs.
__global__ void __launch_bounds__(256)
k_koe_stage_batch(const uint32_t *__restrict__ x, size_t x_stride, const uint32_t *__restrict__ gammas,
                  const uint32_t *__restrict__ L, size_t L_stride, size_t n, uint32_t *__restrict__ lhs, size_t lhs_stride,
                  uint32_t *__restrict__ rhs, size_t rhs_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t p = blockIdx.y;
    if (i < n) {
        if (x) f256_st(lhs + 8 * p * lhs_stride, (long long)i + 1, f256_ld<frbn>(x + 8 * p * x_stride, (long long)i));
        if (L) f256_st(rhs + 8 * p * rhs_stride, (long long)(n - 1 - i), f256_ld<frbn>(L + 8 * p * L_stride, (long long)i));
    } else if (i == n && x) {
        f256_st(lhs + 8 * p * lhs_stride, 0, f256_ld<frbn>(gammas, (long long)p));
    }
}

// lane p: u[p] = c_p[n], then c_p[n] = 0
__global__ void __launch_bounds__(256)
k_koe_split_batch(uint32_t *__restrict__ c, size_t c_stride, size_t n, size_t n_wit, uint32_t *__restrict__ u) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_wit) return;
    uint32_t *row = c + 8 * p * c_stride;
    f256_st(u, (long long)p, f256_ld<frbn>(row, (long long)n));
    f256_st(row, (long long)n, frbn_zero());
}

extern "C" int vmpc_bn256_koe_stage_batch_dev(vmpc_ctx *ctx, const void *x, size_t x_stride, const void *gammas,
                                              const void *L, size_t L_stride, size_t n, size_t n_wit, void *lhs,
                                              size_t lhs_stride, void *rhs, size_t rhs_stride) {
    const size_t cap = (size_t)1 << 31;
    if (n > VMPC_BN256_FR_POLY_MAX - 1 || n_wit > VMPC_BN256_QAP_MAX_WIT || x_stride > cap || L_stride > cap ||
        lhs_stride > cap || rhs_stride > cap ||
        (n_wit && (x_stride < n || L_stride < n || lhs_stride < n + 1 || rhs_stride < n)))
        return VMPC_E_RANGE;
    if (!ctx || (!x && !L) || (x && (!lhs || !gammas)) || (L && !rhs)) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope s(ctx, "bn_koe_stage");
    k_koe_stage_batch<<<dim3((unsigned)((n + 1 + 255) / 256), (unsigned)n_wit), 256, 0, ctx->stream>>>(
        (const uint32_t *)x, x_stride, (const uint32_t *)gammas, (const uint32_t *)L, L_stride, n, (uint32_t *)lhs,
        lhs_stride, (uint32_t *)rhs, rhs_stride);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_koe_split_batch_dev(vmpc_ctx *ctx, void *c, size_t c_stride, size_t n, size_t n_wit,
                                              void *u_out) {
    if (n > VMPC_BN256_FR_POLY_MAX - 1 || n_wit > VMPC_BN256_QAP_MAX_WIT || c_stride > ((size_t)1 << 31) ||
        (n_wit && c_stride < 2 * n))
        return VMPC_E_RANGE;
    if (!ctx || !c || !u_out || n == 0) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope s(ctx, "bn_koe_split");
    k_koe_split_batch<<<(unsigned)((n_wit + 255) / 256), 256, 0, ctx->stream>>>((uint32_t *)c, c_stride, n, n_wit,
                                                                               (uint32_t *)u_out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_fr_powers_dev(vmpc_ctx *ctx, const void *z, const void *scale, size_t count, void *out) {
    if (!ctx || !z || !scale || (count && !out) || count > ((size_t)1 << 32)) return VMPC_E_INVAL;
    if (count == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope s(ctx, "bn_fr_powers");
    const size_t lanes = (count + KOE_POW_RUN - 1) / KOE_POW_RUN;
    k_frbn_powers<<<(unsigned)((lanes + 255) / 256), 256, 0, ctx->stream>>>((const uint32_t *)z, (const uint32_t *)scale,
                                                                           count, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_fr_poly_mul(const uint8_t *a, size_t na, const uint8_t *b, size_t nb, uint8_t *out) {
    if (na > VMPC_BN256_FR_POLY_MAX || nb > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!a || !b || !out || na == 0 || nb == 0) return VMPC_E_INVAL;
    vmpc_ctx *ctx = nullptr;
    VMPC_CHECK(vmpc_ctx_create(0, &ctx));
    void *da = nullptr, *db = nullptr, *dout = nullptr;
    int rc = vmpc_malloc(ctx, na * 32, &da);
    if (!rc) rc = vmpc_malloc(ctx, nb * 32, &db);
    if (!rc) rc = vmpc_malloc(ctx, (na + nb - 1) * 32, &dout);
    if (!rc) rc = vmpc_memcpy_h2d(ctx, da, a, na * 32);
    if (!rc) rc = vmpc_memcpy_h2d(ctx, db, b, nb * 32);
    if (!rc) rc = vmpc_bn256_fr_poly_mul_dev(ctx, da, na, db, nb, dout);
    if (!rc) rc = vmpc_ctx_sync(ctx);
    if (!rc) rc = vmpc_memcpy_d2h(ctx, out, dout, (na + nb - 1) * 32);
    if (da) vmpc_free(ctx, da);
    if (db) vmpc_free(ctx, db);
    if (dout) vmpc_free(ctx, dout);
    vmpc_ctx_destroy(ctx);
    return rc;
}
