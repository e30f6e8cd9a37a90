// The R1CS solve on Shamir shares (demos/demo_zkp_trinocchio.py:70: qap.calculate_witness on secure values, one MPyC
// multiplication per `*` line of the flat code): one party's two halves of a ROUND of product rows over BN-256's GF(n),
// DESIGN.md section 23.  The host plan (pynocchio.ShareSolvePlan) puts the rows that need no communication into local
// phases, which run through vmpc_bn256_r1cs_solve_batch_dev as they are, and the product rows of one multiplicative
// depth into a round; csrc/r1cs_share.h is a product row's arithmetic before and after the exchange.
//
//   k_r1cs_share_mul_deal   d = (V_i . c_w)(W_i . c_w) of this party's share vector, dealt afresh with degree t to the
//                           parties: out[q][e].  d is written nowhere.
//   k_r1cs_share_finish     c_w[wire_i] = (sum_p weights[p] parts[p][e] - Y_i . c_w) inv_i from what arrived.
//
// Both have k_r1cs_level's shape: rows on x, witnesses on y, one lane per (row, witness); e = w n_r + (i - r0), so a
// wavefront reads and writes 64 consecutive elements of a table row.  No atomics on field values, no LDS.
#include <string.h>

#include "common.h"
#include "fr_bn.h"
#include "r1cs_share.h"

#define RSH_WG 256
#define RSH_MAX_STRIDE ((size_t)1 << 31)

__global__ void __launch_bounds__(RSH_WG)
k_r1cs_share_mul_deal(r1cs_csr V, r1cs_csr W, uint32_t r0, uint32_t r1, uint32_t m, const uint32_t *__restrict__ c,
                      size_t c_stride, const uint32_t *__restrict__ coeffs, uint32_t t, uint32_t parties,
                      uint32_t *__restrict__ out, size_t out_stride) {
    const uint32_t i = blockIdx.x * RSH_WG + threadIdx.x;
    if (i >= r1 - r0) return;
    const size_t w = blockIdx.y, n_r = r1 - r0;
    r1cs_share_deal_element<frbn>(V, W, r0 + i, c + 8 * w * c_stride, m, coeffs, t, parties, (size_t)gridDim.y * n_r,
                                  w * n_r + i, out, out_stride);
}

// the weights travel as a kernel argument (2 KiB): uniform over the grid, read through the scalar data path
struct rsh_weights {
    uint32_t w[VMPC_SHARE_MAX_PARTIES][8];
};

__global__ void __launch_bounds__(RSH_WG)
k_r1cs_share_finish(r1cs_csr Y, const uint32_t *__restrict__ wire, const uint32_t *__restrict__ inv, uint32_t r0,
                    uint32_t r1, uint32_t m, const uint32_t *__restrict__ parts, uint32_t parties, size_t part_stride,
                    rsh_weights wts, uint32_t *c, size_t c_stride, uint32_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * RSH_WG + threadIdx.x;
    if (i >= r1 - r0) return;
    const size_t w = blockIdx.y, n_r = r1 - r0;
    if (!r1cs_share_finish_element<frbn>(Y, wire, inv, r0 + i, c + 8 * w * c_stride, m, parts, parties, part_stride,
                                         w * n_r + i, wts.w))
        atomicAdd(&status[VMPC_ST_NONCANON], 1u);   // a count of events, not a field value
}
static_assert(VMPC_SHARE_MAX_PARTIES <= F256_ACC_MAX_PRODUCTS, "k_r1cs_share_finish: one f256_acc per element");

// the checks the two entries share; n_e: the elements of the round's tables
static int rsh_ranges(size_t r0, size_t r1, size_t m, size_t c_stride, size_t n_wit, size_t parties, size_t stride,
                      size_t *n_e) {
    const size_t n_r = r1 > r0 ? r1 - r0 : 0;
    if (parties > VMPC_SHARE_MAX_PARTIES || n_wit > VMPC_BN256_R1CS_MAX_WIT || c_stride > RSH_MAX_STRIDE ||
        stride > RSH_MAX_STRIDE || m >= RSH_MAX_STRIDE || r0 > RSH_MAX_STRIDE || r1 > RSH_MAX_STRIDE ||
        n_r * n_wit > RSH_MAX_STRIDE || c_stride < m + 1)
        return VMPC_E_RANGE;
    *n_e = n_r * n_wit;
    return VMPC_OK;
}

static dim3 rsh_grid(size_t r0, size_t r1, size_t n_wit) {
    return dim3((unsigned)((r1 - r0 + RSH_WG - 1) / RSH_WG), (unsigned)n_wit);
}

extern "C" int vmpc_bn256_r1cs_share_mul_deal_dev(vmpc_ctx *ctx, const uint32_t *v_row_ptr, const uint32_t *v_col,
                                                  const void *v_vals, const uint32_t *w_row_ptr, const uint32_t *w_col,
                                                  const void *w_vals, size_t r0, size_t r1, size_t m, const void *c,
                                                  size_t c_stride, size_t n_wit, const void *coeffs, size_t t,
                                                  size_t parties, void *out, size_t out_stride) {
    size_t n_e = 0;
    const int rc = rsh_ranges(r0, r1, m, c_stride, n_wit, parties, out_stride, &n_e);
    if (rc != VMPC_OK) return rc;
    if (!ctx || parties < 1 || t >= parties || r1 < r0 || out_stride < n_e) return VMPC_E_INVAL;
    if (n_e == 0) return VMPC_OK;
    if (!v_row_ptr || !v_col || !v_vals || !w_row_ptr || !w_col || !w_vals || !c || !out || (t && !coeffs))
        return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_r1cs_share_mul_deal");
    const r1cs_csr V = {v_row_ptr, v_col, (const uint32_t *)v_vals}, W = {w_row_ptr, w_col, (const uint32_t *)w_vals};
    k_r1cs_share_mul_deal<<<rsh_grid(r0, r1, n_wit), RSH_WG, 0, ctx->stream>>>(
        V, W, (uint32_t)r0, (uint32_t)r1, (uint32_t)m, (const uint32_t *)c, c_stride, (const uint32_t *)coeffs,
        (uint32_t)t, (uint32_t)parties, (uint32_t *)out, out_stride);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_r1cs_share_finish_dev(vmpc_ctx *ctx, const uint32_t *y_row_ptr, const uint32_t *y_col,
                                                const void *y_vals, const uint32_t *wire, const void *inv, size_t r0,
                                                size_t r1, size_t m, const void *parts, size_t parties,
                                                size_t part_stride, const uint8_t *weights, void *c, size_t c_stride,
                                                size_t n_wit) {
    size_t n_e = 0;
    const int rc = rsh_ranges(r0, r1, m, c_stride, n_wit, parties, part_stride, &n_e);
    if (rc != VMPC_OK) return rc;
    if (!ctx || parties < 1 || !weights || r1 < r0 || part_stride < n_e) return VMPC_E_INVAL;
    rsh_weights w;
    memset(&w, 0, sizeof w);
    for (size_t p = 0; p < parties; p++) {
        memcpy(w.w[p], weights + 32 * p, 32);
        if (f256_geq_m<frbn>(w.w[p])) return VMPC_E_NONCANON;
    }
    if (n_e == 0) return VMPC_OK;
    if (!y_row_ptr || !y_col || !y_vals || !wire || !inv || !parts || !c) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_r1cs_share_finish");
    const r1cs_csr Y = {y_row_ptr, y_col, (const uint32_t *)y_vals};
    k_r1cs_share_finish<<<rsh_grid(r0, r1, n_wit), RSH_WG, 0, ctx->stream>>>(
        Y, wire, (const uint32_t *)inv, (uint32_t)r0, (uint32_t)r1, (uint32_t)m, (const uint32_t *)parts,
        (uint32_t)parties, part_stride, w, (uint32_t *)c, c_stride, ctx->d_status);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
