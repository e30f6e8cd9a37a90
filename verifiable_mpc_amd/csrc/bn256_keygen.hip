// Pinocchio key generation over BN-256 (verifiable_mpc/trinocchio/pynocchio.py:101-200): the scalar side, GF(n) with n
// the group order (csrc/fr_bn.h).  Every key point is (exponent) * g1 or g2; this file makes the exponents, the
// points are vmpc_bn256_fixed_base_dev of them.
//
//   vmpc_bn256_qap_lagrange_dev   l_j(s) for j = 1..d and t(s) = prod (s - j): the Lagrange basis of the reference's
//                                 interpolation points x = 1..d (qap_creator.r1cs_to_qap_ff) at the secret s,
//                                     l_j(s) = (-1)^(d-j) A_j B_j / ((j-1)! (d-j)!),
//                                     A_j = prod_{k<j} (s - k),  B_j = prod_{k>j} (s - k).
//                                 No division by s - j, so s in {1..d} (l_j = [j = s], t = 0) and s = 0 are exact.
//                                 With Q_j = prod_{k>=j} k = d! / (j-1)!:  1/((j-1)! (d-j)!) = Q_j Q_{d-j+1} / d!^2,
//                                 so ONE Fermat inversion (of d!) serves all j.  A, B and Q are exclusive prefix
//                                 products of three generated sequences (s - k forward, s - k backward, k backward):
//                                 csrc/fr_scan.h with runs of KG_RUN elements, and a last kernel combines.
//   vmpc_bn256_qap_colsum_dev     out[c] = sum_e vals[e] basis[rows[e]] over the entries of column c: v_i(s), w_i(s),
//                                 y_i(s) of a sparse R1CS (basis = l(s)) or of a dense QAP (basis = 1, s, .., s^d, rows
//                                 = coefficient degrees).  The plan and the kernels are csrc/fr_colsum.h, shared with
//                                 vmpc_fr_cs_colsum_dev: deterministic, no atomics.
//   vmpc_bn256_keygen_exps_dev    the seven exponent vectors of the evaluation key's per-wire entries plus their
//                                 zero-knowledge tails, for the wires in idx (pynocchio.py:106-154).
#include "common.h"
#include "fr_bn.h"
#include "fr_colsum.h"
#include "fr_scan.h"

#define KG_RUN 64       // sequence elements per lane in the scans

// sequence q (csrc/fr_scan.h), element k (0 <= k < d): s - (k+1), s - (d-k), d - k; s is in device memory
struct kg_seq {
    const uint32_t *s;
    uint32_t d;
};
struct kg_seq_bound {
    frbn s;
    uint32_t d;
    __device__ frbn operator()(const frbn &v, uint32_t q, uint32_t k) const {
        const frbn i = f256_small<frbn>(q ? d - k : k + 1);
        return frbn_mul(v, q == 2 ? i : frbn_sub(s, i));
    }
};
__device__ __forceinline__ kg_seq_bound fr_scan_bind(const kg_seq &a) { return kg_seq_bound{frbn_load(a.s), a.d}; }

// sequence 2's total is d!: inv_sq = 1 / d!^2 (one Fermat inversion)
struct kg_fin {
    uint32_t *inv_sq;
    __device__ void operator()(uint32_t q, const frbn &total) const {
        if (q != 2) return;
        const frbn iv = frbn_inv(total);
        f256_st(inv_sq, 0, frbn_mul(iv, iv));
    }
};

// ell[j-1] = (-1)^(d-j) A_j B_j Q_j Q_{d-j+1} / d!^2 with A_j = pre0[j-1], B_j = pre1[d-j], Q_j = pre2[d-j+1]
__global__ void __launch_bounds__(256)
k_kg_combine(uint32_t d, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ inv_sq,
             uint32_t *__restrict__ ell, uint32_t *__restrict__ t_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // j = i + 1
    if (i >= d) return;
    const size_t st = (size_t)d + 1;
    const uint32_t *p0 = pre, *p1 = pre + 8 * st, *p2 = pre + 16 * st;
    const uint32_t j = i + 1;
    frbn v = frbn_mul(f256_ld<frbn>(p0, j - 1), f256_ld<frbn>(p1, d - j));
    v = frbn_mul(v, f256_ld<frbn>(p2, d - j + 1));
    v = frbn_mul(v, f256_ld<frbn>(p2, j));
    v = frbn_mul(v, f256_ld<frbn>(inv_sq, 0));
    if ((d - j) & 1u) v = frbn_sub(frbn_zero(), v);
    f256_st(ell, i, v);
    if (i == 0) f256_st(t_out, 0, f256_ld<frbn>(p0, d));
}

extern "C" int vmpc_bn256_qap_lagrange_dev(vmpc_ctx *ctx, const void *s, size_t d, void *ell_out, void *t_out) {
    if (d > VMPC_BN256_QAP_MAX_D) return VMPC_E_RANGE;
    if (!ctx || !s || !ell_out || !t_out || d == 0) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const uint32_t dd = (uint32_t)d;
    const size_t run_b = fr_scan_run_bytes<KG_RUN>(d, 3), pre_b = 3 * (d + 1) * 32;
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(run_b) + vmpc_align(pre_b) + 1024));
    uint32_t *run = (uint32_t *)vmpc_ws_take(ctx, run_b);
    uint32_t *pre = (uint32_t *)vmpc_ws_take(ctx, pre_b);
    uint32_t *inv_sq = (uint32_t *)vmpc_ws_take(ctx, 32);
    {
        vmpc_stage_scope sc(ctx, "bn_qap_lagrange_scan");
        VMPC_CHECK((fr_scan<frbn, KG_RUN>(ctx, kg_seq{(const uint32_t *)s, dd}, dd, 3, run, pre, kg_fin{inv_sq})));
    }
    {
        vmpc_stage_scope sc(ctx, "bn_qap_lagrange_combine");
        k_kg_combine<<<(unsigned)((d + 255) / 256), 256, 0, ctx->stream>>>(dd, pre, inv_sq, (uint32_t *)ell_out,
                                                                          (uint32_t *)t_out);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

extern "C" int vmpc_bn256_qap_colsum_dev(vmpc_ctx *ctx, const void *basis, size_t n_basis, const uint32_t *rows,
                                         const void *vals, size_t nnz, const uint32_t *items, size_t n_items,
                                         const uint32_t *long_cols, size_t n_long, size_t n_partial, void *out,
                                         size_t n_out) {
    VMPC_CHECK(fr_colsum_check(ctx, basis, n_basis, VMPC_BN256_QAP_MAX_D + 1, rows, vals, nnz, items, n_items, long_cols,
                               n_long, n_partial, out, n_out));
    if (!out) return VMPC_E_INVAL;
    return fr_colsum<frbn>(ctx, "bn_qap_colsum", false, basis, n_basis, rows, vals, nnz, items, n_items, long_cols, n_long,
                           n_partial, out, n_out);
}

// Row r < n_idx, wire i = idx[r], X_i = (v_i, w_i, y_i)(s) read from vwy (v at 0, w at n_wires, y at 2 n_wires); coef =
// (r_v, r_w, r_y, alpha_v r_v, alpha_w r_w, alpha_y r_y, beta r_v, beta r_w, beta r_y).  Vector e (stride n_idx + 3):
//   0: r_v v_i   1: r_w w_i   2: r_y y_i   3: alpha_v r_v v_i   4: alpha_w r_w w_i   5: alpha_y r_y y_i
//   6: beta (r_v v_i + r_w w_i + r_y y_i)
// Tail rows n_idx + (0, 1, 2) belong to the deltas (v, w, y): the element's t(s) term where it uses that delta, 0
// (the point at infinity) where it does not - the layout of PreparedKey's shared G1 vectors; vector 1 (the twist) uses
// its first tail row only.
__global__ void __launch_bounds__(256)
k_kg_exps(const uint32_t *__restrict__ coef, const uint32_t *__restrict__ vwy, uint64_t n_wires,
          const uint32_t *__restrict__ t_in, const uint32_t *__restrict__ idx, uint64_t n_idx,
          uint32_t *__restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t rows = n_idx + 3;
    if (r >= rows) return;
    frbn c[9];
#pragma unroll
    for (int k = 0; k < 9; k++) c[k] = f256_ld<frbn>(coef, k);
    frbn e[7];
    if (r < n_idx) {
        const uint64_t i = idx[r];
        frbn v = frbn_zero(), w = frbn_zero(), y = frbn_zero();
        if (i < n_wires) {
            v = f256_ld<frbn>(vwy, (long long)i);
            w = f256_ld<frbn>(vwy, (long long)(n_wires + i));
            y = f256_ld<frbn>(vwy, (long long)(2 * n_wires + i));
        }
        e[0] = frbn_mul(c[0], v);
        e[1] = frbn_mul(c[1], w);
        e[2] = frbn_mul(c[2], y);
        e[3] = frbn_mul(c[3], v);
        e[4] = frbn_mul(c[4], w);
        e[5] = frbn_mul(c[5], y);
        e[6] = frbn_add(frbn_add(frbn_mul(c[6], v), frbn_mul(c[7], w)), frbn_mul(c[8], y));
    } else {
        const frbn t = f256_ld<frbn>(t_in, 0);
        const int dl = (int)(r - n_idx);   // 0: delta_v, 1: delta_w, 2: delta_y
#pragma unroll
        for (int k = 0; k < 7; k++) e[k] = frbn_zero();
        if (dl == 0) {
            e[0] = frbn_mul(c[0], t);
            e[1] = frbn_mul(c[1], t);
            e[3] = frbn_mul(c[3], t);
            e[6] = frbn_mul(c[6], t);
        } else if (dl == 1) {
            e[4] = frbn_mul(c[4], t);
            e[6] = frbn_mul(c[7], t);
        } else {
            e[2] = frbn_mul(c[2], t);
            e[5] = frbn_mul(c[5], t);
            e[6] = frbn_mul(c[8], t);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) f256_st(out, (long long)(k * rows + r), e[k]);
}

extern "C" int vmpc_bn256_keygen_exps_dev(vmpc_ctx *ctx, const void *coef, const void *vwy, size_t n_wires,
                                          const void *t, const uint32_t *idx, size_t n_idx, void *out) {
    if (n_idx > 0xFFFFFFFFull || n_wires > 0xFFFFFFFFull) return VMPC_E_RANGE;
    if (!ctx || !coef || !t || !out || (n_wires && !vwy) || (n_idx && !idx)) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_keygen_exps");
    const size_t rows = n_idx + 3;
    k_kg_exps<<<(unsigned)((rows + 255) / 256), 256, 0, ctx->stream>>>(
        (const uint32_t *)coef, (const uint32_t *)vwy, n_wires, (const uint32_t *)t, idx, n_idx, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
