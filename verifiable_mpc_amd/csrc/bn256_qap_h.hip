// The Pinocchio prover's quotient polynomial h = (V W - Y) / t over BN-256's GF(n), from the row values of the R1CS
// (verifiable_mpc/trinocchio/pynocchio.py:203-225: compute_p_poly, p / qap.t, compute_h_zk_terms - quadratic Python over
// the dense QAP).  n - 1 = 2^5 * odd: no NTT; the polynomials V, W are never interpolated.  With a_j = V(j), b_j = W(j)
// (j = 1..d), w_j = t'(j) = (-1)^(d-j) (j-1)! (d-j)! and u_j = a_j / w_j,
//     V(x) / t(x) = sum_j u_j / (x - j) = sum_{k>=1} A_k x^-k,   A_k = sum_j u_j j^(k-1)   (the moments of u)
// so the polynomial part of V W / t (= h for a satisfying witness, deg Y < d) is a correlation of t's coefficients
// with the low half of the product of the two moment series.
//
//   vmpc_bn256_qap_moments_dev     out[k] = sum_{j=1..d} u[j-1] j^k for k < n_out, one or two vectors.  THE hot kernel:
//                                  d * n_out steps, but a step multiplies the running value u_j j^k by the small integer
//                                  j (frbn_mul_small), not by a field element.  A workgroup owns QH_KS consecutive k and
//                                  a range of j; lane t holds QH_J running values per vector (j = chunk base + t + 256 i),
//                                  started at the segment's first k by square-and-multiply (the power of j shared by
//                                  both vectors).  Per k a lane adds its values in nine limbs, cuts the sum into 26-bit
//                                  pieces and the wave adds each piece in 32-bit registers (DPP within rows of 16, four
//                                  readlanes across them); lane (k mod 64) keeps the wave's total.  Every 64 k the four
//                                  waves' totals go through LDS into the workgroup's nine-limb accumulators (one per k
//                                  and vector), which persist over the workgroup's chunks of j.  One partial per
//                                  (j range, k), reduced mod n, goes to the arena; k_qh_partsum adds them in a fixed
//                                  order.  Integer additions only: deterministic, no atomics.
//   vmpc_bn256_qap_h_weights_dev   ua[j-1] = a_j / w_j, ub[j-1] = b_j / w_j: with E_m = d (d-1) .. (d-m+1),
//                                  1 / ((j-1)! (d-j)!) = E_(d-j+1) E_j / d!^2 - prefix products of small integers and ONE
//                                  inversion, as vmpc_bn256_qap_lagrange_dev does for its Q_j.
//   vmpc_bn256_qap_check_dev       the smallest j with a_j b_j != y_j
//   vmpc_bn256_qap_residual_dev    sum_j rho^j (a_j b_j - y_j): what a party holding SHARES of the witness computes in
//                                  place of the check (its own rows never satisfy a_j b_j = y_j);
//                                  vmpc_bn256_qap_residual_batch_dev: K share vectors under ONE rho (section 24)
//   vmpc_bn256_qap_t_coeffs_dev    the d + 1 coefficients of t = prod (x - j): leaves of QH_LEAF factors multiplied out
//                                  in LDS, then a product tree over vmpc_bn256_fr_poly_mul_dev
//   vmpc_bn256_qap_horner_dev      P(1), .., P(d) of coefficient vectors (the dense QAP form), one lane per point
//   vmpc_bn256_qap_h_combine_dev   moments, t, deltas -> h (the halves that it reads of two products, through
//                                  vmpc_bn256_fr_poly_mul_batch_dev)
//
// For K witnesses of one QAP the moments, the weights, the check, the residual (section 24) and
// the combination have a *_batch_dev entry with rows a stride apart.  Each of these stages is ONE kernel with the
// witness on the grid's last dimension and ONE static host function (qh_moments, qh_weights, qh_check, qh_residual,
// qh_combine) that plans, reserves and launches; the single entry and the batch entry check their own arguments and
// call it, the single one with K = 1.
// The check writes one word per witness, the weights run their scan and inversion ONCE, the moments count K when they
// cut j into ranges (a large batch: one range, one partial per k), and the combination asks
// vmpc_bn256_fr_poly_mul_batch_dev only for P[0 .. d-2] and Q[d-1 .. 2d-2] of its two products.
#include <vector>

#include "common.h"
#include "fr_bn.h"
#include "fr_conv.h"
#include "fr_scan.h"
#include "qap_tleaf.h"
#include "share_combine.h"

#define QH_WG 256
#define QH_J 4                      // running values per lane and vector
#define QH_CHUNK (QH_WG * QH_J)     // j per workgroup pass
#define QH_KS 512                   // k per workgroup (LDS: 2 x 512 x 36 B accumulators + 18 KB staging)
#define QH_KB 64                    // k between two accumulator updates (one per lane of a wave)
#define QH_MAX_GROUPS 32            // j ranges (partials per k) at most
#define QH_TARGET_WGS 2048
#define QH_RUN 64                   // sequence elements per lane in the weights' scan
#define QH_MAX_STRIDE ((size_t)1 << 31)  // row strides of the batch entries, in scalars, at most
#define QH_RES_MAX_WGS 64           // workgroups (partials) of the residual at most: rows beyond 64 x 256 share lanes

// the sum of x over the 64 lanes (uniform), for lane values below 2^26: rows of 16 by DPP (xor 1, xor 2, half
// mirror, mirror leave the row's sum in every lane), the four rows by readlane
__device__ __forceinline__ uint32_t qh_wave_sum(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true);   // row_half_mirror
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true);   // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 0) + (uint32_t)__builtin_amdgcn_readlane((int)x, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 32) + (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
}

// One workgroup of the grid (k segments, j groups).  part[v][(g n_out + k)] = sum over group g's j of u_v[j-1] j^k mod n.
// Bounds: j <= d < 2^21 (frbn_mul_small); a lane's QH_J values sum below 2^258 (ten 26-bit pieces), 64 lanes' pieces
// below 2^32, a wave total below 2^264, four waves and at most 2^10 chunks below 2^276 < 2^288 (frbn_wide).
template <int NV>
__device__ __forceinline__ void
qh_moments_wg(const uint32_t *__restrict__ u0, const uint32_t *__restrict__ u1, uint32_t d, uint32_t n_out, uint32_t ks,
              uint32_t chunks_per_group, uint32_t *__restrict__ part0, uint32_t *__restrict__ part1) {
    __shared__ uint32_t sAcc[NV][QH_KS][9];
    __shared__ uint32_t sSt[QH_WG / 64][NV][9][64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t k0 = blockIdx.x * ks, g = blockIdx.y;
    for (uint32_t i = t; i < NV * QH_KS * 9; i += QH_WG) (&sAcc[0][0][0])[i] = 0;
    __syncthreads();
    const uint32_t n_chunks = (d + QH_CHUNK - 1) / QH_CHUNK;
    const uint32_t c_end = (g + 1) * chunks_per_group < n_chunks ? (g + 1) * chunks_per_group : n_chunks;
    for (uint32_t c = g * chunks_per_group; c < c_end; c++) {
        uint32_t jv[QH_J];
        frbn v[NV][QH_J];
#pragma unroll
        for (int i = 0; i < QH_J; i++) {
            const uint32_t idx = c * QH_CHUNK + i * QH_WG + t;   // j - 1
            const bool in = idx < d;
            jv[i] = in ? idx + 1 : 0;
            frbn pw = frbn_one();
            if (k0) {   // (uniform) j^k0, left to right: full squarings, small multiplications
                for (int b = 31 - __clz(k0); b >= 0; b--) {
                    pw = frbn_mul(pw, pw);
                    if ((k0 >> b) & 1u) pw = frbn_mul_small(pw, jv[i]);
                }
            }
#pragma unroll
            for (int nv = 0; nv < NV; nv++) {
                const uint32_t *u = nv ? u1 : u0;
                v[nv][i] = in ? f256_ld<frbn>(u, idx) : frbn_zero();
                if (k0) v[nv][i] = frbn_mul(v[nv][i], pw);
            }
        }
        for (uint32_t kb = 0; kb < ks; kb += QH_KB) {
            uint32_t mine[NV][10];
#pragma unroll
            for (int nv = 0; nv < NV; nv++)
#pragma unroll
                for (int q = 0; q < 10; q++) mine[nv][q] = 0;
#pragma unroll 1
            for (uint32_t kk = 0; kk < QH_KB; kk++) {
#pragma unroll
                for (int nv = 0; nv < NV; nv++) {
                    frbn_wide s = frbn_wide_zero();
#pragma unroll
                    for (int i = 0; i < QH_J; i++) frbn_wide_add_fr(s, v[nv][i]);
                    uint32_t p[10];
                    frbn_wide_split26(s, p);
#pragma unroll
                    for (int q = 0; q < 10; q++) {
                        const uint32_t tot = qh_wave_sum(p[q]);
                        mine[nv][q] = lane == kk ? tot : mine[nv][q];
                    }
#pragma unroll
                    for (int i = 0; i < QH_J; i++) v[nv][i] = frbn_mul_small(v[nv][i], jv[i]);
                }
            }
            // lane l of each wave holds the wave's total for k = k0 + kb + l: add the four into the accumulators
#pragma unroll
            for (int nv = 0; nv < NV; nv++) {
                const frbn_wide w = frbn_wide_join26(mine[nv]);
#pragma unroll
                for (int l = 0; l < 9; l++) sSt[wave][nv][l][lane] = w.v[l];
            }
            __syncthreads();
            if (t < 64 * NV) {
                const uint32_t nv = t >> 6;
                uint32_t *acc = sAcc[nv][kb + lane];
                frbn_wide a;
#pragma unroll
                for (int l = 0; l < 9; l++) a.v[l] = acc[l];
#pragma unroll
                for (int w = 0; w < QH_WG / 64; w++) {
                    frbn_wide o;
#pragma unroll
                    for (int l = 0; l < 9; l++) o.v[l] = sSt[w][nv][l][lane];
                    frbn_wide_add(a, o);
                }
#pragma unroll
                for (int l = 0; l < 9; l++) acc[l] = a.v[l];
            }
            __syncthreads();
        }
    }
    for (uint32_t i = t; i < NV * ks; i += QH_WG) {
        const uint32_t nv = i / ks, k = i % ks;
        if (k0 + k >= n_out) continue;
        frbn_wide a;
#pragma unroll
        for (int l = 0; l < 9; l++) a.v[l] = sAcc[nv][k][l];
        f256_st(nv ? part1 : part0, (long long)g * n_out + k0 + k, frbn_wide_reduce(a));
    }
}

// grid (k segments, j groups, witnesses): the workgroup above on witness blockIdx.z's rows of u0, u1 (u_stride scalars
// apart) and its `groups` x n_out partials
template <int NV>
__global__ void __launch_bounds__(QH_WG)
k_qh_moments(const uint32_t *__restrict__ u0, const uint32_t *__restrict__ u1, size_t u_stride, uint32_t d, uint32_t n_out,
             uint32_t ks, uint32_t chunks_per_group, uint32_t *__restrict__ part0, uint32_t *__restrict__ part1) {
    const size_t w = blockIdx.z, rows = 8 * w * gridDim.y * (size_t)n_out;
    qh_moments_wg<NV>(u0 + 8 * w * u_stride, NV > 1 ? u1 + 8 * w * u_stride : nullptr, d, n_out, ks, chunks_per_group,
                      part0 + rows, part1 + rows);
}

// grid (outputs, witnesses, vectors): witness y's partials of vector z, added in the order part[0][k] + part[1][k] + ..
// (csrc/fr_conv.h), into its row of out0 / out1
__global__ void __launch_bounds__(256)
k_qh_partsum(const uint32_t *__restrict__ part0, const uint32_t *__restrict__ part1, uint32_t n_out, uint32_t groups,
             uint32_t *__restrict__ out0, uint32_t *__restrict__ out1, size_t out_stride) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const size_t w = blockIdx.y;
    const uint32_t *part = (blockIdx.z ? part1 : part0) + 8 * w * groups * (size_t)n_out;
    f256_st((blockIdx.z ? out1 : out0) + 8 * w * out_stride, k, fr_partsum<frbn>(part, n_out, groups, k));
}

// The ranges of j with the witnesses counted: k segments x groups x K workgroups against QH_TARGET_WGS, at most
// QH_MAX_GROUPS.  A large batch ends at one range, one partial per k and witness.
struct qh_batch_plan {
    uint32_t ks, n_kseg, groups, cpg;
    size_t part_b, total_b;
};

static qh_batch_plan qh_moments_batch_plan(size_t d, size_t n_out, size_t n_wit) {
    qh_batch_plan p;
    p.ks = (uint32_t)(n_out >= QH_KS ? QH_KS : (n_out + QH_KB - 1) / QH_KB * QH_KB);
    p.n_kseg = (uint32_t)((n_out + p.ks - 1) / p.ks);
    const uint32_t n_chunks = (uint32_t)((d + QH_CHUNK - 1) / QH_CHUNK);
    p.groups = (uint32_t)(QH_TARGET_WGS / ((size_t)p.n_kseg * n_wit));
    if (p.groups < 1) p.groups = 1;
    if (p.groups > QH_MAX_GROUPS) p.groups = QH_MAX_GROUPS;
    if (p.groups > n_chunks) p.groups = n_chunks;
    p.cpg = (n_chunks + p.groups - 1) / p.groups;
    p.groups = (n_chunks + p.cpg - 1) / p.cpg;
    p.part_b = n_wit * p.groups * n_out * 32;
    p.total_b = 2 * vmpc_align(p.part_b) + 512;
    return p;
}

// n_wit >= 1 witnesses and n_out >= 1, checked by the entries; one witness may come with strides 0
static int qh_moments(vmpc_ctx *ctx, const void *u0, const void *u1, size_t u_stride, size_t d, size_t n_out, void *out0,
                      void *out1, size_t out_stride, size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const qh_batch_plan p = qh_moments_batch_plan(d, n_out, n_wit);
    VMPC_CHECK(vmpc_ws_reserve(ctx, p.total_b));        // before any launch
    uint32_t *part0 = (uint32_t *)vmpc_ws_take(ctx, p.part_b);
    uint32_t *part1 = (uint32_t *)vmpc_ws_take(ctx, p.part_b);
    const unsigned K = (unsigned)n_wit;
    {
        vmpc_stage_scope sc(ctx, "bn_qap_moments");
        const dim3 grid(p.n_kseg, p.groups, K);
        if (u1)
            k_qh_moments<2><<<grid, QH_WG, 0, ctx->stream>>>((const uint32_t *)u0, (const uint32_t *)u1, u_stride,
                                                             (uint32_t)d, (uint32_t)n_out, p.ks, p.cpg, part0, part1);
        else
            k_qh_moments<1><<<grid, QH_WG, 0, ctx->stream>>>((const uint32_t *)u0, nullptr, u_stride, (uint32_t)d,
                                                             (uint32_t)n_out, p.ks, p.cpg, part0, part1);
        VMPC_KERNEL_CHECK();
    }
    {
        vmpc_stage_scope sc(ctx, "bn_qap_moments_sum");
        k_qh_partsum<<<dim3((unsigned)((n_out + 255) / 256), K, u1 ? 2 : 1), 256, 0, ctx->stream>>>(
            part0, part1, (uint32_t)n_out, p.groups, (uint32_t *)out0, (uint32_t *)out1, out_stride);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

extern "C" int vmpc_bn256_qap_moments_dev(vmpc_ctx *ctx, const void *u0, const void *u1, size_t d, size_t n_out,
                                          void *out0, void *out1) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_out > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !u0 || !out0 || (u1 && !out1) || d == 0) return VMPC_E_INVAL;
    if (n_out == 0) return VMPC_OK;
    return qh_moments(ctx, u0, u1, 0, d, n_out, out0, out1, 0, 1);
}

extern "C" size_t vmpc_bn256_qap_moments_batch_bytes(size_t d, size_t n_out, size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_out > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT || d == 0 ||
        n_out == 0 || n_wit == 0)
        return 0;
    return qh_moments_batch_plan(d, n_out, n_wit).total_b;
}

extern "C" int vmpc_bn256_qap_moments_batch_dev(vmpc_ctx *ctx, const void *u0, const void *u1, size_t u_stride, size_t d,
                                                size_t n_out, void *out0, void *out1, size_t out_stride, size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_out > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT ||
        u_stride > QH_MAX_STRIDE || out_stride > QH_MAX_STRIDE || (n_wit && (u_stride < d || out_stride < n_out)))
        return VMPC_E_RANGE;
    if (!ctx || !u0 || !out0 || (u1 && !out1) || d == 0) return VMPC_E_INVAL;
    if (n_out == 0 || n_wit == 0) return VMPC_OK;
    return qh_moments(ctx, u0, u1, u_stride, d, n_out, out0, out1, out_stride, n_wit);
}

// ---- the weights 1 / w_j --------------------------------------------------------------------------------------------
// E[m] = d (d-1) .. (d-m+1) for m = 0..d (E[d] = d!): exclusive prefix products of e_k = d - k (csrc/fr_scan.h)
struct qh_seq {
    uint32_t d;
    __device__ frbn operator()(const frbn &v, uint32_t, uint32_t k) const { return frbn_mul_small(v, d - k); }
};

// the total is d!: inv_sq = 1 / d!^2 (one Fermat inversion)
struct qh_fin {
    uint32_t *inv_sq;
    __device__ void operator()(uint32_t, const frbn &total) const {
        const frbn iv = frbn_inv(total);
        f256_st(inv_sq, 0, frbn_mul(iv, iv));
    }
};

// grid (rows, witnesses): ua[j-1] = a_j f_j, ub[j-1] = b_j f_j on witness blockIdx.y's rows, f_j = (-1)^(d-j) E[d-j+1]
// E[j] / d!^2 = 1 / w_j; E and inv_sq are the QAP's, computed once
__global__ void __launch_bounds__(256)
k_qh_weights(uint32_t d, const uint32_t *__restrict__ E, const uint32_t *__restrict__ inv_sq,
             const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, size_t ab_stride,
             uint32_t *__restrict__ ua, uint32_t *__restrict__ ub, size_t u_stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d) return;
    const size_t w = blockIdx.y;
    const uint32_t j = i + 1;
    frbn f = frbn_mul(frbn_mul(f256_ld<frbn>(E, d - j + 1), f256_ld<frbn>(E, j)), f256_ld<frbn>(inv_sq, 0));
    if ((d - j) & 1u) f = frbn_sub(frbn_zero(), f);
    f256_st(ua + 8 * w * u_stride, i, frbn_mul(f256_ld<frbn>(a + 8 * w * ab_stride, i), f));
    if (b) f256_st(ub + 8 * w * u_stride, i, frbn_mul(f256_ld<frbn>(b + 8 * w * ab_stride, i), f));
}

// n_wit >= 1 witnesses, checked by the entries; one witness may come with strides 0
static int qh_weights(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t d, void *ua, void *ub,
                      size_t u_stride, size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const uint32_t dd = (uint32_t)d;
    const size_t run_b = fr_scan_run_bytes<QH_RUN>(d, 1);
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(run_b) + vmpc_align((d + 1) * 32) + 1024));
    uint32_t *run = (uint32_t *)vmpc_ws_take(ctx, run_b);
    uint32_t *E = (uint32_t *)vmpc_ws_take(ctx, (d + 1) * 32);
    uint32_t *inv_sq = (uint32_t *)vmpc_ws_take(ctx, 32);
    vmpc_stage_scope sc(ctx, "bn_qap_h_weights");
    VMPC_CHECK((fr_scan<frbn, QH_RUN>(ctx, qh_seq{dd}, dd, 1, run, E, qh_fin{inv_sq})));
    k_qh_weights<<<dim3((unsigned)((d + 255) / 256), (unsigned)n_wit), 256, 0, ctx->stream>>>(
        dd, E, inv_sq, (const uint32_t *)a, (const uint32_t *)b, ab_stride, (uint32_t *)ua, (uint32_t *)ub, u_stride);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_qap_h_weights_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t d, void *ua, void *ub) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !a || !ua || (b && !ub) || d == 0) return VMPC_E_INVAL;
    return qh_weights(ctx, a, b, 0, d, ua, ub, 0, 1);
}

extern "C" int vmpc_bn256_qap_h_weights_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t d,
                                                  void *ua, void *ub, size_t u_stride, size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT || ab_stride > QH_MAX_STRIDE ||
        u_stride > QH_MAX_STRIDE || (n_wit && (ab_stride < d || u_stride < d)))
        return VMPC_E_RANGE;
    if (!ctx || !a || !ua || (b && !ub) || d == 0) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    return qh_weights(ctx, a, b, ab_stride, d, ua, ub, u_stride, n_wit);
}

// ---- the witness check ----------------------------------------------------------------------------------------------
// grid (rows, witnesses): first_bad[w] = witness w's smallest bad row (rows `stride` scalars apart)
__global__ void __launch_bounds__(256)
k_qh_check(uint32_t d, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, const uint32_t *__restrict__ y,
           size_t stride, uint32_t *__restrict__ first_bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d) return;
    const size_t w = blockIdx.y, off = 8 * w * stride;
    // an index, not a field value: the minimum does not depend on the order
    if (!f256_equal(frbn_mul(f256_ld<frbn>(a + off, i), f256_ld<frbn>(b + off, i)), f256_ld<frbn>(y + off, i)))
        atomicMin(first_bad + w, i);
}

// n_wit >= 1 witnesses, checked by the entries; one witness may come with stride 0
static int qh_check(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t stride, size_t d,
                    uint32_t *first_bad, size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_qap_check");
    VMPC_HIP_CHECK(hipMemsetAsync(first_bad, 0xFF, 4 * n_wit, ctx->stream));
    k_qh_check<<<dim3((unsigned)((d + 255) / 256), (unsigned)n_wit), 256, 0, ctx->stream>>>(
        (uint32_t)d, (const uint32_t *)a, (const uint32_t *)b, (const uint32_t *)y, stride, first_bad);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_bn256_qap_check_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t d,
                                        uint32_t *first_bad) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !y || !first_bad || d == 0) return VMPC_E_INVAL;
    return qh_check(ctx, a, b, y, 0, d, first_bad, 1);
}

extern "C" int vmpc_bn256_qap_check_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t stride,
                                              size_t d, uint32_t *first_bad, size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT || stride > QH_MAX_STRIDE ||
        (n_wit && stride < d))
        return VMPC_E_RANGE;
    if (!ctx || !a || !b || !y || !first_bad || d == 0) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    return qh_check(ctx, a, b, y, stride, d, first_bad, n_wit);
}

// ---- the residual of a share vector ---------------------------------------------------------------------------------
struct qh_scalar {
    uint32_t v[8];
};

// grid (workgroups, witnesses).  part[w groups + g] = sum over workgroup g's rows i of witness w of rho^i (a_i b_i - y_i)
// mod n, the row at the point j = i + 1 carrying rho^i (rows `stride` scalars apart; ONE rho for every witness).
// Lane L of a witness's lanes owns the rows L, L + S, L + 2S, .. (S = all lanes of one witness): it starts its power at
// rho^L (square and multiply) and advances it by rho^S (`step`, from the host), adding the unreduced products into its
// own f256_acc (at most 2^20 / S of them), reduced once.  The workgroup's 256 residues are added through LDS in a fixed
// tree.
__global__ void __launch_bounds__(QH_WG)
k_qh_residual(uint32_t d, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, const uint32_t *__restrict__ y,
              size_t stride, qh_scalar rho, qh_scalar step, uint32_t *__restrict__ part) {
    __shared__ frbn sR[QH_WG];
    const uint32_t t = threadIdx.x, first = blockIdx.x * QH_WG + t, S = gridDim.x * QH_WG;
    const size_t w = blockIdx.y, off = 8 * w * stride;
    frbn r = frbn_zero();
    if (first < d) {
        const frbn rh = f256_copy<frbn>(rho.v), st = f256_copy<frbn>(step.v);
        frbn pw = frbn_one();
        if (first) {
            for (int bit = 31 - __clz(first); bit >= 0; bit--) {
                pw = frbn_mul(pw, pw);
                if ((first >> bit) & 1u) pw = frbn_mul(pw, rh);
            }
        }
        frbn_acc acc = frbn_acc_zero();
        for (uint32_t i = first; i < d; i += S) {
            const frbn e = frbn_sub(frbn_mul(f256_ld<frbn>(a + off, i), f256_ld<frbn>(b + off, i)),
                                    f256_ld<frbn>(y + off, i));
            frbn_acc_mac(acc, pw.v, e.v);
            pw = frbn_mul(pw, st);
        }
        r = frbn_acc_reduce(acc);
    }
    sR[t] = r;
    __syncthreads();
    for (uint32_t h = QH_WG / 2; h >= 1; h >>= 1) {
        if (t < h) sR[t] = frbn_add(sR[t], sR[t + h]);
        __syncthreads();
    }
    if (t == 0) f256_st(part, w * gridDim.x + blockIdx.x, sR[0]);
}

// n_wit >= 1 witnesses, checked by the entries; one witness may come with stride 0.  out: n_wit consecutive scalars.
static int qh_residual(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t stride, size_t d,
                       const uint8_t rho[32], void *out, size_t n_wit) {
    qh_scalar r, step;
    memcpy(r.v, rho, 32);
    if (f256_geq_m<frbn>(r.v)) return VMPC_E_NONCANON;
    size_t groups = (d + QH_WG - 1) / QH_WG;
    if (groups > QH_RES_MAX_WGS) groups = QH_RES_MAX_WGS;
    // rho^S for the S = groups x 256 lanes of a witness, on the host (S has one or two bits set above the eighth)
    frbn pw = frbn_one();
    const frbn rh = f256_copy<frbn>(r.v);
    for (int bit = 31; bit >= 0; bit--) {
        pw = frbn_mul(pw, pw);
        if (((uint32_t)(groups * QH_WG) >> bit) & 1u) pw = frbn_mul(pw, rh);
    }
    memcpy(step.v, pw.v, 32);
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(n_wit * groups * 32) + 256));
    uint32_t *part = (uint32_t *)vmpc_ws_take(ctx, n_wit * groups * 32);
    {
        vmpc_stage_scope sc(ctx, "bn_qap_residual");
        k_qh_residual<<<dim3((unsigned)groups, (unsigned)n_wit), QH_WG, 0, ctx->stream>>>(
            (uint32_t)d, (const uint32_t *)a, (const uint32_t *)b, (const uint32_t *)y, stride, r, step, part);
        VMPC_KERNEL_CHECK();
    }
    {
        vmpc_stage_scope sc(ctx, "bn_qap_residual_sum");
        k_qh_partsum<<<dim3(1, (unsigned)n_wit), 256, 0, ctx->stream>>>(part, nullptr, 1, (uint32_t)groups,
                                                                        (uint32_t *)out, nullptr, 1);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

extern "C" int vmpc_bn256_qap_residual_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t d,
                                           const uint8_t rho[32], void *out) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !y || !rho || !out || d == 0) return VMPC_E_INVAL;
    return qh_residual(ctx, a, b, y, 0, d, rho, out, 1);
}

extern "C" int vmpc_bn256_qap_residual_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y,
                                                 size_t stride, size_t d, const uint8_t rho[32], void *out,
                                                 size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT || stride > QH_MAX_STRIDE ||
        (n_wit && stride < d))
        return VMPC_E_RANGE;
    if (!ctx || !a || !b || !y || !rho || !out || d == 0) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    return qh_residual(ctx, a, b, y, stride, d, rho, out, n_wit);
}

// ---- t's coefficients -----------------------------------------------------------------------------------------------
// leaf l: prod (x - j) over j = l QH_LEAF + 1 .. min((l+1) QH_LEAF, d), its deg + 1 coefficients at dst + 32 (l QH_LEAF + l)
// (leaves packed one after the other).  The product itself: csrc/qap_tleaf.h.
__global__ void __launch_bounds__(QH_WG) k_qh_tleaf(uint32_t d, uint32_t *__restrict__ dst) {
    __shared__ frbn sP[2][QH_LEAF + 1];
    const uint32_t t = threadIdx.x, l = blockIdx.x;
    const uint32_t j0 = l * QH_LEAF + 1, j1 = j0 + QH_LEAF - 1 < d ? j0 + QH_LEAF - 1 : d;
    const int cur = qh_tleaf_product(t, j0, j1, sP);
    const uint32_t deg = j1 - j0 + 1;
    if (t <= deg) f256_st(dst, (long long)l * (QH_LEAF + 1) + t, sP[cur][t]);
}

extern "C" int vmpc_bn256_qap_t_coeffs_dev(vmpc_ctx *ctx, size_t d, void *scratch, void *out) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !out || d == 0 || (d > QH_LEAF && !scratch)) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t leaves = (d + QH_LEAF - 1) / QH_LEAF;
    if (leaves == 1) {
        vmpc_stage_scope sc(ctx, "bn_qap_t_leaf");
        k_qh_tleaf<<<1, QH_WG, 0, ctx->stream>>>((uint32_t)d, (uint32_t *)out);
        VMPC_KERNEL_CHECK();
        return VMPC_OK;
    }
    // two level buffers of d + leaves scalars each: a level's polynomials lie one after the other
    const size_t level_b = (d + leaves) * 32;
    char *buf[2] = {(char *)scratch, (char *)scratch + level_b};
    {
        vmpc_stage_scope sc(ctx, "bn_qap_t_leaf");
        k_qh_tleaf<<<(unsigned)leaves, QH_WG, 0, ctx->stream>>>((uint32_t)d, (uint32_t *)buf[0]);
        VMPC_KERNEL_CHECK();
    }
    std::vector<size_t> off(leaves), len(leaves);
    for (size_t l = 0; l < leaves; l++) {
        off[l] = l * (QH_LEAF + 1);
        len[l] = (l + 1 < leaves ? QH_LEAF : d - l * QH_LEAF) + 1;
    }
    int cur = 0;
    while (off.size() > 1) {
        std::vector<size_t> noff, nlen;
        size_t pos = 0;
        const bool last = off.size() == 2;
        char *dst = last ? (char *)out : buf[cur ^ 1];
        for (size_t i = 0; i + 1 < off.size(); i += 2) {
            VMPC_CHECK(vmpc_bn256_fr_poly_mul_dev(ctx, buf[cur] + 32 * off[i], len[i], buf[cur] + 32 * off[i + 1],
                                                  len[i + 1], dst + 32 * pos));
            noff.push_back(pos);
            nlen.push_back(len[i] + len[i + 1] - 1);
            pos += nlen.back();
        }
        if (off.size() & 1) {
            const size_t i = off.size() - 1;
            VMPC_HIP_CHECK(hipMemcpyAsync(dst + 32 * pos, buf[cur] + 32 * off[i], 32 * len[i], hipMemcpyDeviceToDevice,
                                          ctx->stream));
            noff.push_back(pos);
            nlen.push_back(len[i]);
        }
        off.swap(noff);
        len.swap(nlen);
        cur ^= 1;
    }
    return VMPC_OK;
}

// ---- values at the integer points (dense QAP form) ------------------------------------------------------------------
// out[p d + i] = sum_k coeffs[p n_coeffs + k] (i + 1)^k: Horner with small multipliers, one lane per point
__global__ void __launch_bounds__(256)
k_qh_horner(const uint32_t *__restrict__ coeffs, uint32_t n_coeffs, uint32_t d, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (i >= d) return;
    const uint32_t *c = coeffs + 8 * (size_t)p * n_coeffs;
    frbn acc = frbn_zero();
    for (uint32_t k = n_coeffs; k-- > 0;) acc = frbn_add(frbn_mul_small(acc, i + 1), f256_ld<frbn>(c, k));
    f256_st(out, (long long)p * d + i, acc);
}

extern "C" int vmpc_bn256_qap_horner_dev(vmpc_ctx *ctx, const void *coeffs, size_t n_coeffs, size_t n_polys, size_t d,
                                         void *out) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_coeffs > VMPC_BN256_FR_POLY_MAX || n_polys > 65535) return VMPC_E_RANGE;
    if (!ctx || !out || d == 0 || (n_coeffs && !coeffs)) return VMPC_E_INVAL;
    if (n_polys == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_qap_horner");
    k_qh_horner<<<dim3((unsigned)((d + 255) / 256), (unsigned)n_polys), 256, 0, ctx->stream>>>(
        (const uint32_t *)coeffs, (uint32_t)n_coeffs, (uint32_t)d, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

// ---- the combination ------------------------------------------------------------------------------------------------
// A[i] = A_(i+1), B[i] = B_(i+1) (the moments), P = A * B.  crev[r] = C_(d-r) with
//     C_k = P[k-2] (k >= 2) + delta_v B_k + delta_w A_k
// grid (r, witnesses): witness blockIdx.y's moments (ab_stride apart), its three deltas and its row of the scratch
// (sc_stride apart: P at 0, crev at d).  P holds only P[0 .. d-2], all that C_2 .. C_d read.
__global__ void __launch_bounds__(256)
k_qh_cmid(uint32_t d, const uint32_t *__restrict__ A, const uint32_t *__restrict__ B, size_t ab_stride,
          const uint32_t *__restrict__ deltas, uint32_t *__restrict__ scratch, size_t sc_stride) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d) return;
    const size_t w = blockIdx.y;
    const uint32_t *P = scratch + 8 * w * sc_stride;
    const uint32_t i = d - 1 - r;   // C_(i+1)
    frbn c = i ? f256_ld<frbn>(P, i - 1) : frbn_zero();
    if (deltas) {
        const uint32_t *dl = deltas + 24 * w;
        c = frbn_add(c, frbn_mul(f256_ld<frbn>(dl, 0), f256_ld<frbn>(B + 8 * w * ab_stride, i)));
        c = frbn_add(c, frbn_mul(f256_ld<frbn>(dl, 1), f256_ld<frbn>(A + 8 * w * ab_stride, i)));
    }
    f256_st(scratch + 8 * (w * sc_stride + d), r, c);
}

// Q = (t_1 .. t_d) * crev: h_e = Q[d-1+e] + delta_v delta_w t_e - [e = 0] delta_y for e < d, h_d = delta_v delta_w t_d.
// grid (e, witnesses); the scratch row holds only the window Q[d-1 .. 2d-2] of the second product, at 2 d.
__global__ void __launch_bounds__(256)
k_qh_final(uint32_t d, const uint32_t *__restrict__ scratch, size_t sc_stride, const uint32_t *__restrict__ tc,
           const uint32_t *__restrict__ deltas, uint32_t *__restrict__ out, size_t out_stride) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > d) return;
    const size_t w = blockIdx.y;
    const uint32_t *Q = scratch + 8 * (w * sc_stride + 2 * (size_t)d);
    frbn h = e < d ? f256_ld<frbn>(Q, e) : frbn_zero();
    if (deltas) {
        const uint32_t *dl = deltas + 24 * w;
        h = frbn_add(h, frbn_mul(frbn_mul(f256_ld<frbn>(dl, 0), f256_ld<frbn>(dl, 1)), f256_ld<frbn>(tc, e)));
        if (e == 0) h = frbn_sub(h, f256_ld<frbn>(dl, 2));
    }
    f256_st(out + 8 * w * out_stride, e, h);
}

// n_wit >= 1 witnesses with ab_stride >= d, checked by the entries
static int qh_combine(vmpc_ctx *ctx, const void *A, const void *B, size_t ab_stride, const void *t, size_t d,
                      const void *deltas, void *scratch, void *out, size_t out_stride, size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    // scratch row of a witness: P[0 .. d-2] (d - 1, one unused), crev (d), Q[d-1 .. 2d-2] (d)
    const size_t sc = 3 * d;
    char *P = (char *)scratch, *crev = P + 32 * d, *Q = crev + 32 * d;
    // the larger of the two products' arenas now: once the first kernel is queued nothing can fail for want of memory
    const size_t b1 = vmpc_bn256_fr_poly_mul_batch_bytes(d, d, 0, d - 1, n_wit);
    const size_t b2 = vmpc_bn256_fr_poly_mul_batch_bytes(d, d, d - 1, d, n_wit);
    VMPC_CHECK(vmpc_ws_reserve(ctx, b1 > b2 ? b1 : b2));
    const dim3 grid((unsigned)((d + 1 + 255) / 256), (unsigned)n_wit);
    VMPC_CHECK(vmpc_bn256_fr_poly_mul_batch_dev(ctx, A, ab_stride, d, B, ab_stride, d, 0, d - 1, P, sc, n_wit));
    {
        vmpc_stage_scope s(ctx, "bn_qap_h_cmid");
        k_qh_cmid<<<grid, 256, 0, ctx->stream>>>((uint32_t)d, (const uint32_t *)A, (const uint32_t *)B, ab_stride,
                                                 (const uint32_t *)deltas, (uint32_t *)scratch, sc);
        VMPC_KERNEL_CHECK();
    }
    VMPC_CHECK(vmpc_bn256_fr_poly_mul_batch_dev(ctx, crev, sc, d, (const char *)t + 32, 0, d, d - 1, d, Q, sc, n_wit));
    {
        vmpc_stage_scope s(ctx, "bn_qap_h_final");
        k_qh_final<<<grid, 256, 0, ctx->stream>>>((uint32_t)d, (const uint32_t *)scratch, sc, (const uint32_t *)t,
                                                  (const uint32_t *)deltas, (uint32_t *)out, out_stride);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

extern "C" int vmpc_bn256_qap_h_combine_dev(vmpc_ctx *ctx, const void *A, const void *B, const void *t, size_t d,
                                            const void *deltas, void *scratch, void *out) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !A || !B || !t || !scratch || !out || d == 0) return VMPC_E_INVAL;
    return qh_combine(ctx, A, B, d, t, d, deltas, scratch, out, d + 1, 1);
}

extern "C" int vmpc_bn256_qap_h_combine_batch_dev(vmpc_ctx *ctx, const void *A, const void *B, size_t ab_stride,
                                                  const void *t, size_t d, const void *deltas, void *scratch, void *out,
                                                  size_t out_stride, size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT || ab_stride > QH_MAX_STRIDE ||
        out_stride > QH_MAX_STRIDE || (n_wit && (ab_stride < d || out_stride < d + 1)))
        return VMPC_E_RANGE;
    if (!ctx || !A || !B || !t || !scratch || !out || d == 0) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    return qh_combine(ctx, A, B, ab_stride, t, d, deltas, scratch, out, out_stride, n_wit);
}
