// Shamir sharing mod l on vectors of shares (verifiable_mpc/ac20/mpc_ac20_cb.py:39-189 multiplies shares through
// mpc.schur_prod; here one party's half of that product and of the dealing of random sharings), GF(l) of csrc/fr.h.
//
//   vmpc_fr_share_mul_deal_dev   d_i = a_i b_i (or a_i), then a fresh degree-t sharing of every d_i for parties 1..P:
//                                out[q][i] = d_i + sum_k coeffs[k-1][i] (q+1)^k.  The Shamir dealer (b = NULL) and the
//                                local step of a share-by-share product (the party re-shares its product of shares).
//   vmpc_fr_share_combine_dev    out[dst(i)] = sum_p weights[p] parts[p][i]: the step after the exchange - weights all
//                                one add the parties' dealt sharings, the 2t-degree Lagrange weights at 0 reduce the
//                                degree of a product.  dst scatters a depth level's gates into z.
//
// The same two over GF(n), BN-256's order (fr_bn.h), for Pinocchio proofs from a shared witness:
//   vmpc_bn256_fr_share_mul_deal_dev   the dealing kernel over the other field type of csrc/fr256.h
//   vmpc_bn256_fr_share_combine_dev    out[dst(i)] = addend[i] + sum_p weights[p] parts[p][i]; n^2 needs all 512 bits, so
//                                      the products go into f256_acc (csrc/share_combine.h), not into a 16-limb sum
//
// All stream 32-byte elements, one lane per i; row p / q of a matrix is a plain vector, so at every step of the row
// loop a wavefront reads or writes 64 consecutive elements (2 KiB).  No atomics on field values: bit-reproducible.
#include "common.h"
#include "fr.h"
#include "fr_bn.h"
#include "share_combine.h"

#define SH_WG 256
#define SH_MAX_GRID 2048
#define SH_MAX_N ((size_t)1 << 31)

static inline unsigned sh_grid(size_t n) {
    const size_t g = (n + SH_WG - 1) / SH_WG;
    return (unsigned)(g > SH_MAX_GRID ? SH_MAX_GRID : (g ? g : 1));
}

// Horner in k at the node q + 1: the node is a kernel-uniform small constant, its powers are never tabulated.  The
// coefficient rows are read once per party (P t loads per lane; the rows of one i stay in L2 between parties).
template <class F>
__global__ void __launch_bounds__(SH_WG)
k_share_mul_deal(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, size_t n,
                 const uint32_t *__restrict__ coeffs, uint32_t t, uint32_t parties, uint32_t *__restrict__ out,
                 size_t out_stride) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        F d = f256_ld<F>(a, (long long)i);
        if (b) d = f256_mul(d, f256_ld<F>(b, (long long)i));
        for (uint32_t q = 0; q < parties; q++) {
            F acc = d;
            if (t) {
                const F node = f256_small<F>(q + 1);
                acc = f256_ld<F>(coeffs, (long long)((size_t)(t - 1) * n + i));
                for (uint32_t k = t - 1; k >= 1; k--)
                    acc = f256_add(f256_mul(acc, node), f256_ld<F>(coeffs, (long long)((size_t)(k - 1) * n + i)));
                acc = f256_add(f256_mul(acc, node), d);
            }
            f256_st(out, (long long)((size_t)q * out_stride + i), acc);
        }
    }
}

template <class F>
static int sh_mul_deal(vmpc_ctx *ctx, const char *stage, const void *a, const void *b, size_t n, const void *coeffs,
                       size_t t, size_t parties, void *out, size_t out_stride) {
    if (parties > VMPC_SHARE_MAX_PARTIES || n > SH_MAX_N || out_stride > SH_MAX_N) return VMPC_E_RANGE;
    if (!ctx || parties < 1 || t >= parties || out_stride < n || (n && (!a || !out || (t && !coeffs)))) return VMPC_E_INVAL;
    if (n == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, stage);
    k_share_mul_deal<F><<<sh_grid(n), SH_WG, 0, ctx->stream>>>((const uint32_t *)a, (const uint32_t *)b, n,
                                                               (const uint32_t *)coeffs, (uint32_t)t, (uint32_t)parties,
                                                               (uint32_t *)out, out_stride);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_fr_share_mul_deal_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, const void *coeffs,
                                          size_t t, size_t parties, void *out, size_t out_stride) {
    return sh_mul_deal<fr>(ctx, "share_mul_deal", a, b, n, coeffs, t, parties, out, out_stride);
}

extern "C" int vmpc_bn256_fr_share_mul_deal_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n,
                                                const void *coeffs, size_t t, size_t parties, void *out,
                                                size_t out_stride) {
    return sh_mul_deal<frbn>(ctx, "bn_share_mul_deal", a, b, n, coeffs, t, parties, out, out_stride);
}

// the weights travel as a kernel argument (2 KiB): uniform over the grid, read through the scalar data path
struct sh_weights {
    uint32_t w[VMPC_SHARE_MAX_PARTIES][8];
};

__global__ void __launch_bounds__(SH_WG)
k_share_combine(const uint32_t *__restrict__ parts, uint32_t parties, size_t n, size_t part_stride, sh_weights wts,
                const uint32_t *__restrict__ dst, uint32_t *__restrict__ out, uint32_t *__restrict__ status) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        // The sum of the unreduced products, 16 limbs = 512 bits, reduced ONCE.  Every operand is a canonical residue
        // (the weights: checked by the entry; the parts: checked below, a lane that meets another value adds nothing
        // more and writes nothing), so each product is below l^2 < 2^506 and the sum of at most
        // VMPC_SHARE_MAX_PARTIES = 64 = 2^6 of them is below 2^512: no carry leaves acc[15].
        uint32_t acc[16];
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] = 0;
        bool canonical = true;
        for (uint32_t p = 0; p < parties && canonical; p++) {
            const fr v = f256_ld<fr>(parts, (long long)((size_t)p * part_stride + i));
            if (fr_geq_l(v.v)) {
                canonical = false;
                break;
            }
            fr w;
#pragma unroll
            for (int k = 0; k < 8; k++) w.v[k] = wts.w[p][k];
            uint32_t prod[16];
            fr_mul_wide(prod, v, w);
            uint64_t c = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                c += (uint64_t)acc[k] + prod[k];
                acc[k] = (uint32_t)c;
                c >>= 32;
            }
        }
        if (!canonical) {
            atomicAdd(&status[VMPC_ST_NONCANON], 1u);        // a count of events, not a field value
            continue;
        }
        f256_st(out, dst ? (long long)dst[i] : (long long)i, fr_reduce512(acc));
    }
}
static_assert(VMPC_SHARE_MAX_PARTIES <= 64, "k_share_combine: 2^506 * parties must stay below 2^512");

extern "C" int vmpc_fr_share_combine_dev(vmpc_ctx *ctx, const void *parts, size_t parties, size_t n, size_t part_stride,
                                         const uint8_t *weights, const uint32_t *dst, void *out) {
    if (parties > VMPC_SHARE_MAX_PARTIES || n > SH_MAX_N || part_stride > SH_MAX_N) return VMPC_E_RANGE;
    if (!ctx || parties < 1 || !weights || part_stride < n || (n && (!parts || !out))) return VMPC_E_INVAL;
    sh_weights w;
    memset(&w, 0, sizeof w);
    for (size_t p = 0; p < parties; p++) {
        memcpy(w.w[p], weights + 32 * p, 32);
        if (fr_geq_l(w.w[p])) return VMPC_E_NONCANON;
    }
    if (n == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "share_combine");
    k_share_combine<<<sh_grid(n), SH_WG, 0, ctx->stream>>>((const uint32_t *)parts, (uint32_t)parties, n, part_stride, w,
                                                           dst, (uint32_t *)out, ctx->d_status);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

// ---- GF(n) ----------------------------------------------------------------------------------------------------------
// One lane per i as above; the element's sum is share_combine_element (csrc/share_combine.h): f256_acc, reduced once.
__global__ void __launch_bounds__(SH_WG)
k_bn_share_combine(const uint32_t *__restrict__ parts, uint32_t parties, size_t n, size_t part_stride, sh_weights wts,
                   const uint32_t *__restrict__ dst, const uint32_t *__restrict__ addend, uint32_t *__restrict__ out,
                   uint32_t *__restrict__ status) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        frbn r;
        if (!share_combine_element<frbn>(r, parts, parties, part_stride, i, wts.w, addend)) {
            atomicAdd(&status[VMPC_ST_NONCANON], 1u);        // a count of events, not a field value
            continue;
        }
        f256_st(out, dst ? (long long)dst[i] : (long long)i, r);
    }
}
static_assert(VMPC_SHARE_MAX_PARTIES <= F256_ACC_MAX_PRODUCTS, "k_bn_share_combine: one f256_acc per element");

extern "C" int vmpc_bn256_fr_share_combine_dev(vmpc_ctx *ctx, const void *parts, size_t parties, size_t n,
                                               size_t part_stride, const uint8_t *weights, const uint32_t *dst,
                                               const void *addend, void *out) {
    if (parties > VMPC_SHARE_MAX_PARTIES || n > SH_MAX_N || part_stride > SH_MAX_N) return VMPC_E_RANGE;
    if (!ctx || parties < 1 || !weights || part_stride < n || (n && (!parts || !out))) return VMPC_E_INVAL;
    sh_weights w;
    memset(&w, 0, sizeof w);
    for (size_t p = 0; p < parties; p++) {
        memcpy(w.w[p], weights + 32 * p, 32);
        if (f256_geq_m<frbn>(w.w[p])) return VMPC_E_NONCANON;
    }
    if (n == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_share_combine");
    k_bn_share_combine<<<sh_grid(n), SH_WG, 0, ctx->stream>>>((const uint32_t *)parts, (uint32_t)parties, n, part_stride,
                                                              w, dst, (const uint32_t *)addend, (uint32_t *)out,
                                                              ctx->d_status);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
