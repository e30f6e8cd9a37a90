// The moments A_k = sum_{j=1..d} u_j j^(k-1) of csrc/bn256_qap_h.hip in O(d log^2 d): a subproduct tree over the points
// 1 .. d with its products through the NTT over the integers (csrc/bn256_ntt.hip), DESIGN.md section 26.  The same
// canonical residues as vmpc_bn256_qap_moments_batch_dev, bit for bit: every value on the way is an exact field element.
//
//     sum_{k>=0} A_(k+1) z^k = sum_j u_j / (1 - j z) = R(z) / D(z)
//     N(x) = sum_j u_j prod_{i != j} (x - i),  T(x) = prod_j (x - j),  R = N's coefficients reversed (d of them),
//     D = T's reversed (D(0) = 1):   out[k] = (R D^-1 mod z^n_out)[k]
//
// Geometry (csrc/qap_mtree_plan.h): a full binary tree of 2^L leaves of s <= 128 points over 1 .. d' = s 2^L >= d; the
// points beyond d carry u_j = 0 and change N and T by the same factor.
//
//   the plan, once per (d, n_max) - vmpc_bn256_qap_mtree_build_dev
//     k_mt_tleaf      grid (leaves): the leaf's T in LDS (csrc/qap_tleaf.h, the code of k_qh_tleaf)
//     levels          T_parent = T_left T_right: ONE batched NTT product per level (vmpc_ntt_poly_mul, a product per
//                     parent, the operands strided over the level below)
//     k_mt_dseries    D = T_root reversed, cut or zero-filled to n_max; g = 1
//     Newton          g <- g (2 - D g) mod z^(2k), k doubling up to n_max: two windowed NTT products per step and
//                     k_mt_two_minus between them
//   per call - vmpc_bn256_qap_moments_tree_batch_dev
//     k_mt_nleaf      grid (leaves, witnesses, vectors), one workgroup per leaf and row: N_leaf = sum_j u_j T_leaf /
//                     (x - j).  Lane j divides T_leaf by (x - j) synthetically (frbn_mul_small: q_i = T_(i+1) +
//                     j q_(i+1)) and multiplies each q_i by u_j (ONE full product per coefficient and point, u reduced
//                     on load); eight coefficients at a time go through LDS and are added over j in a fixed order
//                     (sixteen runs of eight, then the sixteen).
//     levels          N_parent = N_left T_right + N_right T_left for ALL nodes, both vectors and all witnesses in one
//                     launch sequence per level (vmpc_ntt_tree_level): a sibling's T is transformed once per node, the
//                     two products are added in the residue domain before the one inverse transform (the bound:
//                     csrc/qap_mtree_plan.h), and the launches do not depend on d / s or on K.
//     k_mt_reverse    R's low min(d', n_out) coefficients of every row
//     series          one batched NTT product per vector with the shared b = D^-1, window [0, n_out), at out_stride
//
// The witnesses are cut into groups that keep a level's residues within the NTT's arena cap
// (vmpc_ctx_set_ntt_arena_cap); a group boundary changes no value.  Integer sums in a fixed order, no atomics.
#include "common.h"
#include "fr_bn.h"
#include "qap_mtree_plan.h"
#include "qap_tleaf.h"

#define MT_WG 256
#define MT_LEAF_WG 128              // k_mt_nleaf: one lane per point of the leaf
#define MT_LEAF_CO 8                // coefficients per pass through LDS
#define MT_MAX_STRIDE ((size_t)1 << 31)

static_assert(QAP_MTREE_S_MAX == QH_LEAF, "the tree's leaves are the leaves of t's product tree");
static_assert(QAP_MTREE_S_MAX == MT_LEAF_WG, "k_mt_nleaf has one lane per point");

// leaf l: prod (x - j) over j = l s + 1 .. (l + 1) s, its s + 1 coefficients at dst + 32 l (s + 1)
__global__ void __launch_bounds__(MT_WG) k_mt_tleaf(uint32_t s, uint32_t *__restrict__ dst) {
    __shared__ frbn sP[2][QH_LEAF + 1];
    const uint32_t t = threadIdx.x, l = blockIdx.x;
    const int cur = qh_tleaf_product(t, l * s + 1, (l + 1) * s, sP);
    if (t <= s) f256_st(dst, (long long)l * (s + 1) + t, sP[cur][t]);
}

// grid (leaves, witnesses, vectors).  nout[row][l s + i] = coefficient i < s of sum_j u_j T_l / (x - j) over the leaf's
// points j = l s + 1 .. (l + 1) s (u_j = 0 beyond d), row = vector x witnesses + witness, rows d' = leaves x s apart.
__global__ void __launch_bounds__(MT_LEAF_WG)
k_mt_nleaf(const uint32_t *__restrict__ tleaf, uint32_t s, uint32_t d, const uint32_t *__restrict__ u0,
           const uint32_t *__restrict__ u1, size_t u_stride, uint32_t *__restrict__ nout) {
    __shared__ frbn sT[QAP_MTREE_S_MAX + 1];
    __shared__ frbn sP[MT_LEAF_CO][MT_LEAF_WG];
    __shared__ frbn sQ[MT_LEAF_CO][MT_LEAF_WG / 8];
    const uint32_t t = threadIdx.x, l = blockIdx.x;
    const size_t w = blockIdx.y, row = (size_t)blockIdx.z * gridDim.y + w;
    const uint32_t *u = (blockIdx.z ? u1 : u0) + 8 * w * u_stride;
    uint32_t *dst = nout + 8 * (row * gridDim.x + l) * (size_t)s;
    for (uint32_t i = t; i <= s; i += MT_LEAF_WG) sT[i] = f256_ld<frbn>(tleaf, (long long)l * (s + 1) + i);
    const uint32_t j = l * s + t + 1;                    // this lane's point
    const bool mine = t < s && j <= d;
    const frbn uj = mine ? f256_ld<frbn>(u, j - 1) : frbn_zero();
    __syncthreads();
    frbn q = frbn_zero();
    for (uint32_t k0 = 0; k0 < s; k0 += MT_LEAF_CO) {    // the coefficients s - 1 - k, from the top
        const uint32_t nk = s - k0 < MT_LEAF_CO ? s - k0 : MT_LEAF_CO;
        for (uint32_t c = 0; c < nk; c++) {
            const uint32_t i = s - 1 - (k0 + c);
            q = i == s - 1 ? frbn_one() : frbn_add(sT[i + 1], frbn_mul_small(q, j));
            sP[c][t] = mine ? frbn_mul(uj, q) : frbn_zero();
        }
        __syncthreads();
        {
            const uint32_t c = t >> 4, part = t & 15;
            if (c < nk) {
                frbn a = sP[c][8 * part];
                for (uint32_t i = 1; i < 8; i++) a = frbn_add(a, sP[c][8 * part + i]);
                sQ[c][part] = a;
            }
        }
        __syncthreads();
        if (t < nk) {
            frbn a = sQ[t][0];
            for (uint32_t i = 1; i < MT_LEAF_WG / 8; i++) a = frbn_add(a, sQ[t][i]);
            f256_st(dst, s - 1 - (k0 + t), a);
        }
    }
}

// grid (n / 256, rows' y, rows' z): dst_row[i] = src_row[top - i] for i < n (0 where i > top), rows a stride apart
__global__ void __launch_bounds__(MT_WG)
k_mt_reverse(const uint32_t *__restrict__ src, size_t src_stride, uint32_t top, uint32_t n, uint32_t *__restrict__ dst,
             size_t dst_stride) {
    const uint32_t i = blockIdx.x * MT_WG + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    f256_st(dst + 8 * row * dst_stride, i, i <= top ? f256_ld<frbn>(src + 8 * row * src_stride, top - i) : frbn_zero());
}

// D = the root's d' + 1 coefficients reversed, n of them (zeros beyond d'); g[0] = 1, the inverse mod z
__global__ void __launch_bounds__(MT_WG)
k_mt_dseries(const uint32_t *__restrict__ root, uint32_t dp, uint32_t n, uint32_t *__restrict__ D,
             uint32_t *__restrict__ g) {
    const uint32_t i = blockIdx.x * MT_WG + threadIdx.x;
    if (i >= n) return;
    f256_st(D, i, i <= dp ? f256_ld<frbn>(root, dp - i) : frbn_zero());
    if (i == 0) f256_st(g, 0, frbn_one());
}

// e <- 2 - e on n coefficients
__global__ void __launch_bounds__(MT_WG) k_mt_two_minus(uint32_t *__restrict__ e, uint32_t n) {
    const uint32_t i = blockIdx.x * MT_WG + threadIdx.x;
    if (i >= n) return;
    frbn c = frbn_zero();
    if (i == 0) c.v[0] = 2;
    f256_st(e, i, frbn_sub(c, f256_ld<frbn>(e, i)));
}

// ---- host ------------------------------------------------------------------------------------------------------------
static bool mt_in_range(size_t d, size_t n_max) {
    return d + 1 <= VMPC_BN256_FR_POLY_MAX && n_max <= VMPC_BN256_FR_POLY_MAX;
}

// the largest arena of the build's products: a level's T products and the Newton steps
static size_t mt_build_arena(const qap_mtree_plan &p, size_t n_max, size_t cap) {
    size_t b = 0;
    for (uint32_t l = 0; l < p.L; l++) {
        const size_t m = (size_t)p.s << l, x = vmpc_ntt_poly_mul_bytes(m + 1, m + 1, false, (size_t)1 << (p.L - l - 1), cap);
        b = x > b ? x : b;
    }
    for (size_t k = 1; k < n_max;) {
        const size_t k2 = 2 * k < n_max ? 2 * k : n_max, x = vmpc_ntt_poly_mul_bytes(k2, k, false, 1, cap);
        b = x > b ? x : b;
        k = k2;
    }
    return b;
}

static int mt_build(vmpc_ctx *ctx, size_t d, size_t n_max, void *plan) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const qap_mtree_plan p = qap_mtree_plan_of(d, n_max);
    char *base = (char *)plan;
    // the largest arena now: once the first kernel is queued nothing can fail for want of memory
    VMPC_CHECK(vmpc_ws_reserve(ctx, mt_build_arena(p, n_max, vmpc_ntt_arena_cap(ctx))));
    {
        vmpc_stage_scope sc(ctx, "bn_qap_mtree_tleaf");
        k_mt_tleaf<<<1u << p.L, MT_WG, 0, ctx->stream>>>(p.s, (uint32_t *)(base + 32 * p.lvl_off[0]));
        VMPC_KERNEL_CHECK();
    }
    for (uint32_t l = 0; l < p.L; l++) {
        const size_t m = (size_t)p.s << l;
        const char *lvl = base + 32 * p.lvl_off[l];
        VMPC_CHECK(vmpc_ntt_poly_mul(ctx, lvl, 2 * (m + 1), m + 1, lvl + 32 * (m + 1), 2 * (m + 1), m + 1, 0, 2 * m + 1,
                                     base + 32 * p.lvl_off[l + 1], 2 * m + 1, (size_t)1 << (p.L - l - 1)));
    }
    if (n_max == 0) return VMPC_OK;
    uint32_t *g = (uint32_t *)(base + 32 * p.dinv_off), *D = (uint32_t *)(base + 32 * p.tmp_off);
    uint32_t *e = D + 8 * n_max;
    {
        vmpc_stage_scope sc(ctx, "bn_qap_mtree_dseries");
        k_mt_dseries<<<(unsigned)((n_max + MT_WG - 1) / MT_WG), MT_WG, 0, ctx->stream>>>(
            (const uint32_t *)(base + 32 * p.lvl_off[p.L]), (uint32_t)p.dp, (uint32_t)n_max, D, g);
        VMPC_KERNEL_CHECK();
    }
    // g = D^-1 mod z^k -> mod z^k2: e = 2 - (D mod z^k2) g, g <- g e.  The second product reads all of g before its
    // last kernel writes the window (the stream's order): it may go back into g.
    for (size_t k = 1; k < n_max;) {
        const size_t k2 = 2 * k < n_max ? 2 * k : n_max;
        VMPC_CHECK(vmpc_ntt_poly_mul(ctx, D, k2, k2, g, k, k, 0, k2, e, k2, 1));
        {
            vmpc_stage_scope sc(ctx, "bn_qap_mtree_newton");
            k_mt_two_minus<<<(unsigned)((k2 + MT_WG - 1) / MT_WG), MT_WG, 0, ctx->stream>>>(e, (uint32_t)k2);
            VMPC_KERNEL_CHECK();
        }
        VMPC_CHECK(vmpc_ntt_poly_mul(ctx, e, k2, k2, g, k, k, 0, k2, g, k2, 1));
        k = k2;
    }
    return VMPC_OK;
}

// witnesses per group and the arena of a call: the residues of the largest level (T's once, the rows' children and
// parents) within `cap`, but never less than one witness; and the final products of a group
struct mt_call_plan {
    size_t group, bytes;
};

static mt_call_plan mt_call_plan_of(const qap_mtree_plan &p, size_t n_out, size_t n_wit, int nv, size_t cap) {
    mt_call_plan c;
    c.group = n_wit;
    c.bytes = 0;
    for (uint32_t l = 0; l < p.L; l++) {
        const size_t m = (size_t)p.s << l, nodes = (size_t)1 << (p.L - l);
        const size_t one = vmpc_ntt_tree_level_bytes(m, nodes, nv);
        const size_t per = vmpc_ntt_tree_level_bytes(m, nodes, 2 * nv) - one;     // a witness more
        const size_t fit = cap > one ? 1 + (cap - one) / per : 1;
        if (fit < c.group) c.group = fit;
    }
    if (c.group > n_wit) c.group = n_wit;
    if (c.group < 1) c.group = 1;
    for (uint32_t l = 0; l < p.L; l++) {
        const size_t b = vmpc_ntt_tree_level_bytes((size_t)p.s << l, (size_t)1 << (p.L - l), nv * c.group);
        c.bytes = b > c.bytes ? b : c.bytes;
    }
    const size_t na = p.dp < n_out ? p.dp : n_out, fin = vmpc_ntt_poly_mul_bytes(na, n_out, true, c.group, cap);
    c.bytes = fin > c.bytes ? fin : c.bytes;
    return c;
}

// n_wit >= 1 witnesses and 1 <= n_out <= n_max, checked by the entry
static int mt_moments(vmpc_ctx *ctx, const void *plan, size_t d, size_t n_max, const void *u0, const void *u1,
                      size_t u_stride, size_t n_out, void *out0, void *out1, size_t out_stride, void *scratch,
                      size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const qap_mtree_plan p = qap_mtree_plan_of(d, n_max);
    const int nv = u1 ? 2 : 1;
    const mt_call_plan c = mt_call_plan_of(p, n_out, n_wit, nv, vmpc_ntt_arena_cap(ctx));
    VMPC_CHECK(vmpc_ws_reserve(ctx, c.bytes));        // before any launch
    const char *base = (const char *)plan;
    const size_t na = p.dp < n_out ? p.dp : n_out;
    // two buffers of the group's rows (vector-major), d' scalars a row
    uint32_t *buf[2] = {(uint32_t *)scratch, (uint32_t *)scratch + 8 * 2 * c.group * p.dp};
    for (size_t w0 = 0; w0 < n_wit; w0 += c.group) {
        const size_t g = n_wit - w0 < c.group ? n_wit - w0 : c.group;
        int cur = 0;
        {
            vmpc_stage_scope sc(ctx, "bn_qap_mtree_nleaf");
            k_mt_nleaf<<<dim3(1u << p.L, (unsigned)g, nv), MT_LEAF_WG, 0, ctx->stream>>>(
                (const uint32_t *)(base + 32 * p.lvl_off[0]), p.s, (uint32_t)d, (const uint32_t *)u0 + 8 * w0 * u_stride,
                u1 ? (const uint32_t *)u1 + 8 * w0 * u_stride : nullptr, u_stride, buf[0]);
            VMPC_KERNEL_CHECK();
        }
        for (uint32_t l = 0; l < p.L; l++, cur ^= 1)
            VMPC_CHECK(vmpc_ntt_tree_level(ctx, base + 32 * p.lvl_off[l], (size_t)p.s << l, (int)(p.L - l), buf[cur],
                                           buf[cur ^ 1], g, nv));
        {
            vmpc_stage_scope sc(ctx, "bn_qap_mtree_reverse");
            k_mt_reverse<<<dim3((unsigned)((na + MT_WG - 1) / MT_WG), (unsigned)g, nv), MT_WG, 0, ctx->stream>>>(
                buf[cur], p.dp, (uint32_t)(p.dp - 1), (uint32_t)na, buf[cur ^ 1], p.dp);
            VMPC_KERNEL_CHECK();
        }
        for (int v = 0; v < nv; v++)
            VMPC_CHECK(vmpc_ntt_poly_mul(ctx, buf[cur ^ 1] + 8 * v * g * p.dp, p.dp, na, base + 32 * p.dinv_off, 0, n_out,
                                         0, n_out, (char *)(v ? out1 : out0) + 32 * w0 * out_stride, out_stride, g));
    }
    return VMPC_OK;
}

extern "C" size_t vmpc_bn256_qap_mtree_bytes(size_t d, size_t n_max) {
    if (!mt_in_range(d, n_max) || d == 0) return 0;
    return 32 * qap_mtree_plan_of(d, n_max).total;
}

extern "C" int vmpc_bn256_qap_mtree_build_dev(vmpc_ctx *ctx, size_t d, size_t n_max, void *plan) {
    if (!mt_in_range(d, n_max)) return VMPC_E_RANGE;
    if (!ctx || !plan || d == 0) return VMPC_E_INVAL;
    return mt_build(ctx, d, n_max, plan);
}

extern "C" size_t vmpc_bn256_qap_moments_tree_batch_bytes(size_t d, size_t n_out, size_t n_wit) {
    if (!mt_in_range(d, n_out) || n_wit > VMPC_BN256_QAP_MAX_WIT || d == 0 || n_out == 0 || n_wit == 0) return 0;
    return mt_call_plan_of(qap_mtree_plan_of(d, n_out), n_out, n_wit, 2, vmpc_ntt_arena_cap(nullptr)).bytes;
}

extern "C" size_t vmpc_bn256_qap_moments_tree_scratch_bytes(size_t d, size_t n_wit) {
    if (d + 1 > VMPC_BN256_FR_POLY_MAX || n_wit > VMPC_BN256_QAP_MAX_WIT || d == 0) return 0;
    return 32 * qap_mtree_scratch_scalars(d, n_wit);
}

extern "C" int vmpc_bn256_qap_moments_tree_batch_dev(vmpc_ctx *ctx, const void *plan, size_t d, size_t n_max,
                                                     const void *u0, const void *u1, size_t u_stride, size_t n_out,
                                                     void *out0, void *out1, size_t out_stride, void *scratch,
                                                     size_t n_wit) {
    if (!mt_in_range(d, n_max) || n_out > n_max || n_wit > VMPC_BN256_QAP_MAX_WIT || u_stride > MT_MAX_STRIDE ||
        out_stride > MT_MAX_STRIDE || (n_wit && (u_stride < d || out_stride < n_out)))
        return VMPC_E_RANGE;
    if (!ctx || !plan || !u0 || !out0 || (u1 && !out1) || !scratch || d == 0) return VMPC_E_INVAL;
    if (n_out == 0 || n_wit == 0) return VMPC_OK;
    return mt_moments(ctx, plan, d, n_max, u0, u1, u_stride, n_out, out0, out1, out_stride, scratch, n_wit);
}
