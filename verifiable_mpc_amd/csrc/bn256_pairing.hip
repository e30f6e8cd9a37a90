// BN-256 optimal-ate pairings and the small linear combinations of the Pinocchio verifier
// (verifiable_mpc/trinocchio/pynocchio.py:276-325 `verify`: 12 pairings in 5 checks, three IO sums per proof).
//
// Kernel shape: one lane per Miller loop (k_bnp_miller: the whole Fp12 accumulator, the twist point T and the
// inputs in registers), then one lane per product for the multiply-together and the final exponentiation
// (k_bnp_final).  The Miller values pass through the context arena in Montgomery form (384 bytes per pair).
// The formulas are csrc/bn256_pairing.h; DESIGN.md section 11 has the measured latency and throughput.
#include "common.h"
#include "bn256_pairing.h"
#include "bn256_curve.h"

// 64 lanes per block: a block is one wave, so the register budget of a lane is the whole 512 VGPRs of gfx950
#define BNP_BLOCK 64
#define BNP_F12_WORDS 96        // 12 residues x 8 words

__global__ void __launch_bounds__(BNP_BLOCK)
k_bnp_miller(const uint32_t *__restrict__ g1, const uint32_t *__restrict__ g2, size_t n, uint32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fp12 f = bnp_miller_enc(g1 + 16 * i, g2 + 32 * i);
    f12_store_raw(out + BNP_F12_WORDS * i, f);
}

// product k multiplies the Miller values [offsets[k], offsets[k+1]) (offsets == nullptr: the single value k); a range
// that is not inside [0, n] is not computed: is_one 0 and an all-zero GT (no field element of GT is zero)
__global__ void __launch_bounds__(BNP_BLOCK)
k_bnp_final(const uint32_t *__restrict__ miller, size_t n, const uint32_t *__restrict__ offsets, size_t n_products,
            uint8_t *__restrict__ is_one, uint32_t *__restrict__ gt) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_products) return;
    const size_t lo = offsets ? offsets[k] : k, hi = offsets ? offsets[k + 1] : k + 1;
    if (lo > hi || hi > n) {
        if (is_one) is_one[k] = 0;
        if (gt)
            for (int w = 0; w < BNP_F12_WORDS; w++) gt[BNP_F12_WORDS * k + w] = 0;
        return;
    }
    fp12 f = f12_one();
    for (size_t j = lo; j < hi; j++) f = f12_mul(f, f12_load_raw(miller + BNP_F12_WORDS * j));
    f = bnp_final_exp(f);
    if (is_one) is_one[k] = f12_is_one(f) ? 1 : 0;
    if (gt) f12_store(gt + BNP_F12_WORDS * k, f);
}

// out[b] = (negate ? -1 : 1) (sum_i scalars[b][i] bases[i] + sum_j rows[b][j]): one lane per row, the bases
// interleaved over one chain of 256 doublings (Straus), the row points added once at the end
template <class C, class F>
__global__ void __launch_bounds__(BNP_BLOCK)
k_bnp_lincomb(const uint32_t *__restrict__ bases, int n_bases, const uint32_t *__restrict__ scalars,
              const uint32_t *__restrict__ rows, int n_rows, size_t batch, int negate, uint32_t *__restrict__ out) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const uint32_t *sc = scalars + (size_t)8 * n_bases * b;
    jac<F> acc = jac_identity<F>();
    if (n_bases) {
        for (int bit = 255; bit >= 0; bit--) {
            acc = jac_dbl<F>(acc);
            for (int i = 0; i < n_bases; i++)
                if ((sc[8 * i + (bit >> 5)] >> (bit & 31)) & 1u)
                    acc = jac_madd<F>(acc, aff_load<F>(bases + (size_t)C::AFF_WORDS * i));
        }
    }
    for (int j = 0; j < n_rows; j++)
        acc = jac_madd<F>(acc, aff_load<F>(rows + (size_t)C::AFF_WORDS * ((size_t)n_rows * b + j)));
    aff<F> r = jac_to_affine<F>(acc);
    if (negate) r.y = F::neg(r.y);
    aff_store<F>(out + (size_t)C::AFF_WORDS * b, r);
}

static unsigned bnp_blocks(size_t n) { return (unsigned)((n + BNP_BLOCK - 1) / BNP_BLOCK); }

extern "C" int vmpc_bn256_pairing_product_dev(vmpc_ctx *ctx, const void *g1, const void *g2, size_t n_pairs,
                                              const uint32_t *offsets, size_t n_products, uint8_t *is_one,
                                              void *gt_out) {
    if (!ctx || (n_pairs && (!g1 || !g2)) || (n_products && !is_one && !gt_out)) return VMPC_E_INVAL;
    if (n_pairs > 0xffffffffull) return VMPC_E_INVAL;
    if (n_products == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(n_pairs * 4 * BNP_F12_WORDS) + 256));
    uint32_t *miller = (uint32_t *)vmpc_ws_take(ctx, n_pairs * 4 * BNP_F12_WORDS);
    if (n_pairs) {
        vmpc_stage_scope s(ctx, "bn_pairing_miller");
        k_bnp_miller<<<bnp_blocks(n_pairs), BNP_BLOCK, 0, ctx->stream>>>((const uint32_t *)g1, (const uint32_t *)g2,
                                                                         n_pairs, miller);
        VMPC_KERNEL_CHECK();
    }
    vmpc_stage_scope s(ctx, "bn_pairing_final");
    k_bnp_final<<<bnp_blocks(n_products), BNP_BLOCK, 0, ctx->stream>>>(miller, n_pairs, offsets, n_products, is_one,
                                                                       (uint32_t *)gt_out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_pairing_dev(vmpc_ctx *ctx, const void *g1, const void *g2, size_t n, void *gt_out) {
    if (!ctx || (n && (!g1 || !g2 || !gt_out))) return VMPC_E_INVAL;
    if (n == 0) return VMPC_OK;
    if (n > 0xffffffffull) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(n * 4 * BNP_F12_WORDS) + 256));
    uint32_t *miller = (uint32_t *)vmpc_ws_take(ctx, n * 4 * BNP_F12_WORDS);
    {
        vmpc_stage_scope s(ctx, "bn_pairing_miller");
        k_bnp_miller<<<bnp_blocks(n), BNP_BLOCK, 0, ctx->stream>>>((const uint32_t *)g1, (const uint32_t *)g2, n,
                                                                   miller);
        VMPC_KERNEL_CHECK();
    }
    vmpc_stage_scope s(ctx, "bn_pairing_final");
    k_bnp_final<<<bnp_blocks(n), BNP_BLOCK, 0, ctx->stream>>>(miller, n, nullptr, n, nullptr, (uint32_t *)gt_out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_lincomb_batch_dev(vmpc_ctx *ctx, int group, const void *bases, size_t n_bases,
                                            const void *scalars, const void *row_points, size_t n_row_points,
                                            size_t batch, int negate, void *out) {
    if (!ctx || (group != 1 && group != 2) || (batch && !out) || (n_bases && (!bases || !scalars)) ||
        (n_row_points && !row_points) || n_bases > 4096 || n_row_points > 4096)
        return VMPC_E_INVAL;
    if (batch == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope s(ctx, "bn_lincomb_batch");
    if (group == 1)
        k_bnp_lincomb<G1, BnF1><<<bnp_blocks(batch), BNP_BLOCK, 0, ctx->stream>>>(
            (const uint32_t *)bases, (int)n_bases, (const uint32_t *)scalars, (const uint32_t *)row_points,
            (int)n_row_points, batch, negate ? 1 : 0, (uint32_t *)out);
    else
        k_bnp_lincomb<G2, BnF2><<<bnp_blocks(batch), BNP_BLOCK, 0, ctx->stream>>>(
            (const uint32_t *)bases, (int)n_bases, (const uint32_t *)scalars, (const uint32_t *)row_points,
            (int)n_row_points, batch, negate ? 1 : 0, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

// ---- host-buffer one-shots ---------------------------------------------------------------------------------------
struct bnp_host_bufs {
    vmpc_ctx *ctx = nullptr;
    void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~bnp_host_bufs() {
        if (!ctx) return;
        for (void *q : p)
            if (q) vmpc_free(ctx, q);
        vmpc_ctx_destroy(ctx);
    }
    // device copy of a host block (nullptr / 0 bytes: nothing); slot k of p
    int up(int k, const void *src, size_t bytes) {
        if (!bytes) return VMPC_OK;
        int rc = vmpc_malloc(ctx, bytes, &p[k]);
        if (!rc && src) rc = vmpc_memcpy_h2d(ctx, p[k], src, bytes);
        return rc;
    }
};

extern "C" int vmpc_bn256_pairing_product(const uint8_t *g1, const uint8_t *g2, size_t n_pairs,
                                          const uint32_t *offsets, size_t n_products, uint8_t *is_one,
                                          uint8_t *gt_out) {
    if ((n_pairs && (!g1 || !g2)) || (n_products && (!offsets || (!is_one && !gt_out)))) return VMPC_E_INVAL;
    if (n_products == 0) return VMPC_OK;
    bnp_host_bufs h;
    VMPC_CHECK(vmpc_ctx_create(0, &h.ctx));
    int rc = h.up(0, g1, n_pairs * 64);
    if (!rc) rc = h.up(1, g2, n_pairs * 128);
    if (!rc) rc = h.up(2, offsets, (n_products + 1) * 4);
    if (!rc) rc = h.up(3, nullptr, n_products);
    if (!rc) rc = h.up(4, nullptr, n_products * 384);
    if (!rc) rc = vmpc_bn256_pairing_product_dev(h.ctx, h.p[0], h.p[1], n_pairs, (const uint32_t *)h.p[2], n_products,
                                                 (uint8_t *)h.p[3], h.p[4]);
    if (!rc) rc = vmpc_ctx_sync(h.ctx);
    if (!rc && is_one) rc = vmpc_memcpy_d2h(h.ctx, is_one, h.p[3], n_products);
    if (!rc && gt_out) rc = vmpc_memcpy_d2h(h.ctx, gt_out, h.p[4], n_products * 384);
    return rc;
}

extern "C" int vmpc_bn256_pairing(const uint8_t *g1, const uint8_t *g2, size_t n, uint8_t *gt_out) {
    if (n && (!g1 || !g2 || !gt_out)) return VMPC_E_INVAL;
    if (n == 0) return VMPC_OK;
    bnp_host_bufs h;
    VMPC_CHECK(vmpc_ctx_create(0, &h.ctx));
    int rc = h.up(0, g1, n * 64);
    if (!rc) rc = h.up(1, g2, n * 128);
    if (!rc) rc = h.up(2, nullptr, n * 384);
    if (!rc) rc = vmpc_bn256_pairing_dev(h.ctx, h.p[0], h.p[1], n, h.p[2]);
    if (!rc) rc = vmpc_ctx_sync(h.ctx);
    if (!rc) rc = vmpc_memcpy_d2h(h.ctx, gt_out, h.p[2], n * 384);
    return rc;
}

extern "C" int vmpc_bn256_lincomb_batch(int group, const uint8_t *bases, size_t n_bases, const uint8_t *scalars,
                                        const uint8_t *row_points, size_t n_row_points, size_t batch, int negate,
                                        uint8_t *out) {
    const size_t pb = group == 1 ? 64 : 128;
    if ((group != 1 && group != 2) || (batch && !out) || (n_bases && (!bases || (batch && !scalars))) ||
        (n_row_points && batch && !row_points))
        return VMPC_E_INVAL;
    if (batch == 0) return VMPC_OK;
    bnp_host_bufs h;
    VMPC_CHECK(vmpc_ctx_create(0, &h.ctx));
    int rc = h.up(0, bases, n_bases * pb);
    if (!rc) rc = h.up(1, scalars, batch * n_bases * 32);
    if (!rc) rc = h.up(2, row_points, batch * n_row_points * pb);
    if (!rc) rc = h.up(3, nullptr, batch * pb);
    uint64_t bad = 0;
    if (!rc && n_bases) rc = vmpc_bn256_validate_dev(h.ctx, group, h.p[0], n_bases, &bad);
    if (!rc && n_row_points) {
        uint64_t bad_rows = 0;
        rc = vmpc_bn256_validate_dev(h.ctx, group, h.p[2], batch * n_row_points, &bad_rows);
        bad += bad_rows;
    }
    if (!rc && bad) rc = VMPC_E_NOTONCURVE;
    if (!rc) rc = vmpc_bn256_lincomb_batch_dev(h.ctx, group, h.p[0], n_bases, h.p[1], h.p[2], n_row_points, batch,
                                               negate, h.p[3]);
    if (!rc) rc = vmpc_ctx_sync(h.ctx);
    if (!rc) rc = vmpc_memcpy_d2h(h.ctx, out, h.p[3], batch * pb);
    return rc;
}
