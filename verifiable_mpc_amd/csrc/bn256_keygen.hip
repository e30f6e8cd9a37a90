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
//                                 each lane multiplies a run of KG_RUN elements, one workgroup per sequence scans the
//                                 run products, each lane rescans its run, and a last kernel combines.
//   vmpc_bn256_qap_colsum_dev     out[c] = sum_e vals[e] basis[rows[e]] over the entries of column c: v_i(s), w_i(s),
//                                 y_i(s) of a sparse R1CS (basis = l(s)) or of a dense QAP (basis = 1, s, .., s^d, rows
//                                 = coefficient degrees).  The host cuts the column-ordered entries into items of at most
//                                 KG_PIECE entries; one lane sums an item (unreduced products in frbn_acc, one
//                                 reduction) and writes the column's value, or, for a column of several items, a
//                                 partial sum that a second kernel adds up (one workgroup per long column, a fixed
//                                 tree): deterministic, no atomics.
//   vmpc_bn256_keygen_exps_dev    the seven exponent vectors of the evaluation key's per-wire entries plus their
//                                 zero-knowledge tails, for the wires in idx (pynocchio.py:106-154).
#include "common.h"
#include "fr_bn.h"

#define KG_RUN 64       // sequence elements per lane in the scans
#define KG_SCAN 256     // threads of the run-product scan (one workgroup per sequence)
#define KG_PARTIAL 0x80000000u

__device__ __forceinline__ frbn kg_small(uint32_t k) {
    frbn r = frbn_zero();
    r.v[0] = k;
    return r;
}

__device__ __forceinline__ frbn kg_ld(const void *p, long long i) {
    const uint4 *q = (const uint4 *)((const uint32_t *)p + 8 * i);
    const uint4 x = q[0], y = q[1];
    const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    return frbn_load(w);
}

__device__ __forceinline__ void kg_st(void *p, long long i, const frbn &a) {
    uint4 *q = (uint4 *)((uint32_t *)p + 8 * i);
    q[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    q[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}

// element k (0 <= k < d) of sequence q: s - (k+1), s - (d-k), d - k
__device__ __forceinline__ frbn kg_elem(int q, const frbn &s, uint32_t d, uint32_t k) {
    if (q == 0) return frbn_sub(s, kg_small(k + 1));
    if (q == 1) return frbn_sub(s, kg_small(d - k));
    return kg_small(d - k);
}

// run[q][l] = product of sequence q over [l KG_RUN, (l+1) KG_RUN) n [0, d)
__global__ void __launch_bounds__(256)
k_kg_runprod(const uint32_t *__restrict__ s_in, uint32_t d, uint32_t lanes, uint32_t *__restrict__ run) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    const int q = blockIdx.y;
    if (l >= lanes) return;
    const frbn s = frbn_load(s_in);
    const uint32_t k0 = l * KG_RUN, k1 = k0 + KG_RUN < d ? k0 + KG_RUN : d;
    frbn p = kg_elem(q, s, d, k0);
    for (uint32_t k = k0 + 1; k < k1; k++) p = frbn_mul(p, kg_elem(q, s, d, k));
    kg_st(run, (long long)q * lanes + l, p);
}

// one workgroup per sequence: run[q][*] -> its exclusive prefix products, total[q] = the product of all.  Thread t owns
// a contiguous block of the lanes; the 256 block products are scanned in LDS (Hillis-Steele, log2 256 steps).  The
// workgroup of sequence 2 (total d!) then writes inv_sq = 1 / d!^2 (one Fermat inversion).
__global__ void __launch_bounds__(KG_SCAN)
k_kg_runscan(uint32_t lanes, uint32_t *__restrict__ run, uint32_t *__restrict__ total, uint32_t *__restrict__ inv_sq) {
    __shared__ frbn buf[2][KG_SCAN];
    const int t = threadIdx.x, q = blockIdx.x;
    uint32_t *r = run + 8 * (size_t)q * lanes;
    const uint32_t per = (lanes + KG_SCAN - 1) / KG_SCAN;
    const uint32_t b0 = t * per < lanes ? t * per : lanes, b1 = b0 + per < lanes ? b0 + per : lanes;
    frbn p = frbn_one();
    for (uint32_t i = b0; i < b1; i++) p = frbn_mul(p, kg_ld(r, i));
    int cur = 0;
    buf[cur][t] = p;
    __syncthreads();
    for (int off = 1; off < KG_SCAN; off <<= 1) {
        frbn v = buf[cur][t];
        if (t >= off) v = frbn_mul(buf[cur][t - off], v);
        buf[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    frbn acc = t ? buf[cur][t - 1] : frbn_one();   // exclusive prefix of this thread's block
    for (uint32_t i = b0; i < b1; i++) {
        const frbn x = kg_ld(r, i);
        kg_st(r, i, acc);
        acc = frbn_mul(acc, x);
    }
    if (t == KG_SCAN - 1) {
        kg_st(total, q, acc);
        if (q == 2) {
            const frbn iv = frbn_inv(acc);
            kg_st(inv_sq, 0, frbn_mul(iv, iv));
        }
    }
}

// pre[q][k] = exclusive prefix product of sequence q at k (k < d); pre[q][d] = total[q]
__global__ void __launch_bounds__(256)
k_kg_runfill(const uint32_t *__restrict__ s_in, uint32_t d, uint32_t lanes, const uint32_t *__restrict__ run,
             const uint32_t *__restrict__ total, uint32_t *__restrict__ pre) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    const int q = blockIdx.y;
    if (l >= lanes) return;
    const frbn s = frbn_load(s_in);
    uint32_t *out = pre + 8 * (size_t)q * (d + 1);
    frbn v = kg_ld(run, (long long)q * lanes + l);
    const uint32_t k0 = l * KG_RUN, k1 = k0 + KG_RUN < d ? k0 + KG_RUN : d;
    for (uint32_t k = k0; k < k1; k++) {
        kg_st(out, k, v);
        v = frbn_mul(v, kg_elem(q, s, d, k));
    }
    if (l == lanes - 1) kg_st(out, d, kg_ld(total, q));
}

// ell[j-1] = (-1)^(d-j) A_j B_j Q_j Q_{d-j+1} / d!^2 with A_j = pre0[j-1], B_j = pre1[d-j], Q_j = pre2[d-j+1]
__global__ void __launch_bounds__(256)
k_kg_combine(uint32_t d, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ inv_sq,
             uint32_t *__restrict__ ell, uint32_t *__restrict__ t_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // j = i + 1
    if (i >= d) return;
    const size_t st = (size_t)d + 1;
    const uint32_t *p0 = pre, *p1 = pre + 8 * st, *p2 = pre + 16 * st;
    const uint32_t j = i + 1;
    frbn v = frbn_mul(kg_ld(p0, j - 1), kg_ld(p1, d - j));
    v = frbn_mul(v, kg_ld(p2, d - j + 1));
    v = frbn_mul(v, kg_ld(p2, j));
    v = frbn_mul(v, kg_ld(inv_sq, 0));
    if ((d - j) & 1u) v = frbn_sub(frbn_zero(), v);
    kg_st(ell, i, v);
    if (i == 0) kg_st(t_out, 0, kg_ld(p0, d));
}

extern "C" int vmpc_bn256_qap_lagrange_dev(vmpc_ctx *ctx, const void *s, size_t d, void *ell_out, void *t_out) {
    if (d > VMPC_BN256_QAP_MAX_D) return VMPC_E_RANGE;
    if (!ctx || !s || !ell_out || !t_out || d == 0) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const uint32_t dd = (uint32_t)d;
    const uint32_t lanes = (uint32_t)((d + KG_RUN - 1) / KG_RUN);
    const size_t run_b = 3 * (size_t)lanes * 32, pre_b = 3 * (d + 1) * 32;
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(run_b) + vmpc_align(pre_b) + vmpc_align(4 * 32) + 1024));
    uint32_t *run = (uint32_t *)vmpc_ws_take(ctx, run_b);
    uint32_t *pre = (uint32_t *)vmpc_ws_take(ctx, pre_b);
    uint32_t *small = (uint32_t *)vmpc_ws_take(ctx, 4 * 32);   // total[3], inv_sq
    const dim3 g((lanes + 255) / 256, 3);
    {
        vmpc_stage_scope sc(ctx, "bn_qap_lagrange_scan");
        k_kg_runprod<<<g, 256, 0, ctx->stream>>>((const uint32_t *)s, dd, lanes, run);
        VMPC_KERNEL_CHECK();
        k_kg_runscan<<<3, KG_SCAN, 0, ctx->stream>>>(lanes, run, small, small + 24);
        VMPC_KERNEL_CHECK();
        k_kg_runfill<<<g, 256, 0, ctx->stream>>>((const uint32_t *)s, dd, lanes, run, small, pre);
        VMPC_KERNEL_CHECK();
    }
    {
        vmpc_stage_scope sc(ctx, "bn_qap_lagrange_combine");
        k_kg_combine<<<(unsigned)((d + 255) / 256), 256, 0, ctx->stream>>>(dd, pre, small + 24, (uint32_t *)ell_out,
                                                                          (uint32_t *)t_out);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

// one lane per item (start, end, dst): dst < n_out -> out[dst]; dst = KG_PARTIAL | p -> part[p].  Entries whose row
// is not below n_basis, items that leave [0, nnz) and destinations out of range add / write nothing.
__global__ void __launch_bounds__(256)
k_kg_colsum(const uint32_t *__restrict__ basis, uint32_t n_basis, const uint32_t *__restrict__ rows,
            const uint32_t *__restrict__ vals, uint64_t nnz, const uint32_t *__restrict__ items, uint64_t n_items,
            uint32_t *__restrict__ part, uint64_t n_partial, uint32_t *__restrict__ out, uint64_t n_out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_items) return;
    const uint32_t e0 = items[3 * k], e1 = items[3 * k + 1], dst = items[3 * k + 2];
    frbn_acc acc = frbn_acc_zero();
    for (uint64_t e = e0; e < e1 && e < nnz; e++) {
        const uint32_t r = rows[e];
        if (r >= n_basis) continue;
        const frbn a = kg_ld(vals, (long long)e), b = kg_ld(basis, r);
        frbn_acc_mac(acc, a.v, b.v);
    }
    const frbn v = frbn_acc_reduce(acc);
    if (dst & KG_PARTIAL) {
        if ((dst & ~KG_PARTIAL) < n_partial) kg_st(part, dst & ~KG_PARTIAL, v);
    } else if (dst < n_out) {
        kg_st(out, dst, v);
    }
}

// one workgroup per long column (col, first, count): out[col] = sum of part[first .. first + count), fixed order
__global__ void __launch_bounds__(256)
k_kg_colfinish(const uint32_t *__restrict__ longs, const uint32_t *__restrict__ part, uint64_t n_partial,
               uint32_t *__restrict__ out, uint64_t n_out) {
    __shared__ frbn red[256];
    const int t = threadIdx.x;
    const uint32_t col = longs[3 * blockIdx.x], first = longs[3 * blockIdx.x + 1], count = longs[3 * blockIdx.x + 2];
    frbn s = frbn_zero();
    for (uint64_t i = t; i < count; i += 256)
        if ((uint64_t)first + i < n_partial) s = frbn_add(s, kg_ld(part, (long long)(first + i)));
    red[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] = frbn_add(red[t], red[t + h]);
        __syncthreads();
    }
    if (t == 0 && col < n_out) kg_st(out, col, red[0]);
}

extern "C" int vmpc_bn256_qap_colsum_dev(vmpc_ctx *ctx, const void *basis, size_t n_basis, const uint32_t *rows,
                                         const void *vals, size_t nnz, const uint32_t *items, size_t n_items,
                                         const uint32_t *long_cols, size_t n_long, size_t n_partial, void *out,
                                         size_t n_out) {
    if (n_basis > VMPC_BN256_QAP_MAX_D + 1 || nnz > 0xFFFFFFFFull || n_partial > 0x7FFFFFFFull ||
        n_out > 0x7FFFFFFFull || n_long > 0x7FFFFFFFull || n_items > 0xFFFFFFFFull)
        return VMPC_E_RANGE;
    if (!ctx || !out || (n_basis && !basis) || (nnz && (!rows || !vals)) || (n_items && !items) ||
        (n_long && !long_cols))
        return VMPC_E_INVAL;
    if (n_items == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    uint32_t *part = nullptr;
    if (n_partial) {
        VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(n_partial * 32) + 256));
        part = (uint32_t *)vmpc_ws_take(ctx, n_partial * 32);
    }
    vmpc_stage_scope sc(ctx, "bn_qap_colsum");
    k_kg_colsum<<<(unsigned)((n_items + 255) / 256), 256, 0, ctx->stream>>>(
        (const uint32_t *)basis, (uint32_t)n_basis, rows, (const uint32_t *)vals, nnz, items, n_items, part, n_partial,
        (uint32_t *)out, n_out);
    VMPC_KERNEL_CHECK();
    if (n_long) {
        k_kg_colfinish<<<(unsigned)n_long, 256, 0, ctx->stream>>>(long_cols, part, n_partial, (uint32_t *)out, n_out);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
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
    for (int k = 0; k < 9; k++) c[k] = kg_ld(coef, k);
    frbn e[7];
    if (r < n_idx) {
        const uint64_t i = idx[r];
        frbn v = frbn_zero(), w = frbn_zero(), y = frbn_zero();
        if (i < n_wires) {
            v = kg_ld(vwy, (long long)i);
            w = kg_ld(vwy, (long long)(n_wires + i));
            y = kg_ld(vwy, (long long)(2 * n_wires + i));
        }
        e[0] = frbn_mul(c[0], v);
        e[1] = frbn_mul(c[1], w);
        e[2] = frbn_mul(c[2], y);
        e[3] = frbn_mul(c[3], v);
        e[4] = frbn_mul(c[4], w);
        e[5] = frbn_mul(c[5], y);
        e[6] = frbn_add(frbn_add(frbn_mul(c[6], v), frbn_mul(c[7], w)), frbn_mul(c[8], y));
    } else {
        const frbn t = kg_ld(t_in, 0);
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
    for (int k = 0; k < 7; k++) kg_st(out, (long long)(k * rows + r), e[k]);
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
