// Protocol 8 (circuit satisfiability, verifiable_mpc/ac20/circuit_sat_cb.py:59-252) from a sparse circuit, over the
// Ed25519 scalar field GF(l) (csrc/fr.h) and over the BN-256 scalar field GF(n) (csrc/fr_bn.h): every kernel and host
// body below is a template on the field F of csrc/fr256.h, stated once; the vmpc_fr_cs_* entries instantiate it at fr,
// the vmpc_bn256_fr_cs_* entries (the knowledge-of-exponent variant) at frbn.  Neither field has
// an NTT of useful length (l - 1 = 2^2 * odd, n - 1 = 2^5 * odd) and f, g, h are never interpolated; the one long
// convolution, the extension's, can go through the multi-prime NTT over the INTEGERS instead
// (csrc/bn256_ntt.hip, vmpc_ctx_set_cs_extension; "the NTT route" below).
//
// With m multiplication gates, z = (x, f(0), g(0), h(0), h(1), .., h(2m)) and M = m + 1 nodes 1..M that carry
// v = a || r_a (f) and b || r_b (g):
//
//   vmpc_fr_cs_triples_dev    a_i, b_i = the affine forms of gate i's wires at (x, gamma), gamma_i = a_i b_i written
//                             straight into z (gamma_i = h(i + 1)); one launch per depth level.  With check != 0 the
//                             gammas in z are the caller's and the smallest i with a_i b_i != gamma_i is reported
//                             (circuit_builder.py:133-151 evaluates the forms one gate after the other in Python).
//   vmpc_fr_cs_triples_batch_dev  the same for K witnesses of ONE circuit in one launch: the witness on blockIdx.y, z and the
//                             row values K rows of one allocation.  The single entry is K = 1 of
//                             the same kernel and host function, as for the extension below.
//   vmpc_fr_cs_tables_dev     k! and 1 / k! for k <= K: two product scans (csrc/fr_scan.h) and ONE inversion.  Everything below is
//                             products of these: 1 / k = (k-1)! / k!, the barycentric weights
//                             w_j = (-1)^(M-j) / ((j-1)! (M-j)!), l(x) = prod_j (x - j) = (x-1)! / (x-M-1)! for x > M.
//   vmpc_fr_cs_extend_dev     f(x) = l(x) sum_j u_j / (x - j), u_j = v_j w_j, at x = 0 and x = m+2 .. 2m, the same for
//                             g, h(x) = f(x) g(x) into z (circuit_sat_r1cs.py:380-388 interpolates and multiplies
//                             coefficient lists, qap_creator.py:154-164; circuit_sat_cb.py:89 evaluates h 2m times).
//                             For x > M every 1 / (x - j) is T[x - j], T[k] = 1 / k: the sums are coefficients m+1 ..
//                             2m-1 of the product of u (M terms) with T - THE hot kernel, k_cs_corr, m^2
//                             multiply-accumulates for f and for g.  The tile of csrc/fr_conv.h, shared with
//                             k_frbn_polymul (csrc/bn256_koe.hip); f and g share the staged T.  Every x meets every j,
//                             so the work per tile is uniform; the range of j is cut into segments for occupancy, their
//                             partial sums added in a fixed order.  Integer sums only: deterministic.
//                             Under VMPC_CS_EXTENSION_NTT (and _AUTO from VMPC_FR_CS_EXT_NTT_MIN gates) k_cs_corr is
//                             replaced by the cyclic product of the 2K rows u_f, u_g with T modulo 18 primes and the
//                             GF(l) reconstruction of its window, written where k_cs_corr's ONE segment would be: same
//                             canonical residues, every other kernel unchanged.
//   vmpc_fr_cs_extend_fg_dev  the same f(x), g(x) left apart and unmultiplied, for a witness that is a vector of Shamir
//                             shares: the extension is linear in v, the product is the parties' (csrc/mpc_share.hip)
//   vmpc_fr_cs_extend_batch_dev  vmpc_fr_cs_extend_dev for K witnesses: T and the weights once, the correlation on a grid
//                             (tiles, segments, witness), the segment length chosen with K counted.  cs_extend() is the
//                             one implementation of all three entries; the two single ones pass K = 1.
//   vmpc_fr_cs_lagrange_dev   the Lagrange vector of the nodes 0..K at c (ac20/recombine.py:5-32, a double loop):
//                             lambda_j = prod_{i != j} (c - i) * (-1)^(K-j) / (j! (K-j)!) - prefix and suffix products
//                             of (c - i), no inversion at all, so a c on a node cannot divide by zero here (the
//                             Python caller still refuses it, as the reference does).
//   vmpc_fr_cs_colsum_dev     out[dst(c)] = sum over the entries e of column c of vals[e] weights[rows[e]]: the
//                             transposed sparse mat-vec that turns row weights (the Lagrange vector, powers of rho)
//                             into the coefficients of the forms of f(c), g(c) and the outputs
//                             (circuit_builder.py:517-545 builds dense forms per gate), every other position zero.
//                             Plan and kernels: csrc/fr_colsum.h, shared with vmpc_bn256_qap_colsum_dev.
//   vmpc_fr_cs_first_diff_dev the smallest i with a[i] != b[i] (the verifier's L == proof["L"])
//
// The GF(n) entries take the arguments of their GF(l) namesakes.  The two that need scratch besides their outputs
// (tables, lagrange) take it from the CALLER - a vmpc_bn256_fr_cs_*_scratch_bytes() query and a pointer - where the GF(l)
// entries take it from the context arena and hand the taken pointers to the same body; the extension and the column sum
// reserve inside cs_extend<F> / fr_colsum<F> for either field.  The share form (_fg) exists over both fields (the M-party
// provers: DESIGN.md sections 18 and 30), and so do the batch forms (vmpc_bn256_fr_cs_triples_batch_dev,
// vmpc_bn256_fr_cs_extend_batch_dev: the batch prover of the knowledge-of-exponent variant).
#include "common.h"
#include "fr.h"
#include "fr_bn.h"
#include "fr_colsum.h"
#include "fr_conv.h"
#include "fr_scan.h"

#define CS_WG 256
#define CS_RUN 32                       // sequence elements per lane in the product scans
#define CS_MIN_SEG 256                  // shortest segment of j; a multiple of FR_CONV_CHUNK
#define CS_TARGET_WGS 8192

// ---- multiplication triples ---------------------------------------------------------------------------------------------
// column c of a form reads z[c] for c < n_x (an input) and z[g_off + c - n_x] otherwise (gamma_(c - n_x))
struct cs_z_map {
    uint32_t n_x, g_off;
    __device__ uint32_t operator()(uint32_t c) const { return c < n_x ? c : g_off + (c - n_x); }
};

template <class F>
__device__ F cs_row_eval(const uint32_t *__restrict__ rp, const uint32_t *__restrict__ col, const uint32_t *__restrict__ val,
                         const uint32_t *__restrict__ cst, uint32_t row, uint32_t n_x, uint32_t g_off,
                         const uint32_t *__restrict__ z) {
    return f256_add(fr_sparse_dot<F>(col, val, rp[row], rp[row + 1], z, cs_z_map{n_x, g_off}), f256_ld<F>(cst, row));
}

// grid (gates, witnesses): the forms and the level's gate list are the circuit's, z / a_out / b_out rows w of K (strides
// in scalars), first_bad one word per witness.  a_out and b_out may be one buffer (check == 2): no __restrict__ on them.
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_triples(const uint32_t *__restrict__ a_rp, const uint32_t *__restrict__ a_col, const uint32_t *__restrict__ a_val,
             const uint32_t *__restrict__ a_cst, const uint32_t *__restrict__ b_rp, const uint32_t *__restrict__ b_col,
             const uint32_t *__restrict__ b_val, const uint32_t *__restrict__ b_cst, const uint32_t *__restrict__ gates,
             uint32_t n_gates, uint32_t n_x, uint32_t g_off, uint32_t *z, size_t z_stride, uint32_t *a_out,
             uint32_t *b_out, size_t ab_stride, int check, uint32_t *__restrict__ first_bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_gates) return;
    const size_t w = blockIdx.y;
    z += w * z_stride * 8;
    a_out += w * ab_stride * 8;
    b_out += w * ab_stride * 8;
    const uint32_t i = gates ? gates[t] : t;
    const F a = cs_row_eval<F>(a_rp, a_col, a_val, a_cst, i, n_x, g_off, z);
    const F b = cs_row_eval<F>(b_rp, b_col, b_val, b_cst, i, n_x, g_off, z);
    f256_st(a_out, i, a);
    f256_st(b_out, i, b);
    if (check == 2) return;   // the forms' values only (the output rows)
    const F p = f256_mul(a, b);
    if (check) {
        if (!f256_equal(p, f256_ld<F>(z, (long long)g_off + i))) atomicMin(first_bad + w, i);   // an index: order does not matter
    } else {
        f256_st(z, (long long)g_off + i, p);
    }
}

// n_wit >= 1 witnesses, checked by the entries; one witness may come with strides 0
template <class F>
static int cs_triples(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                      const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_vals,
                      const void *b_const, const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset, void *z,
                      size_t z_stride, void *a_out, void *b_out, size_t ab_stride, size_t n_wit, int check,
                      uint32_t *first_bad) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, check ? "cs_triples_check" : "cs_triples");
    if (check == 1) VMPC_HIP_CHECK(hipMemsetAsync(first_bad, 0xFF, 4 * n_wit, ctx->stream));
    k_cs_triples<F><<<dim3((unsigned)((n_gates + CS_WG - 1) / CS_WG), (unsigned)n_wit), CS_WG, 0, ctx->stream>>>(
        a_row_ptr, a_col, (const uint32_t *)a_vals, (const uint32_t *)a_const, b_row_ptr, b_col, (const uint32_t *)b_vals,
        (const uint32_t *)b_const, gates, (uint32_t)n_gates, (uint32_t)n_x, (uint32_t)gamma_offset, (uint32_t *)z, z_stride,
        (uint32_t *)a_out, (uint32_t *)b_out, ab_stride, check, first_bad);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

// the single entry of either field: the checks, then one witness with strides 0
template <class F>
static int cs_triples_one(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                          const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_vals,
                          const void *b_const, const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset,
                          void *z, void *a_out, void *b_out, int check, uint32_t *first_bad) {
    if (n_gates > VMPC_FR_CS_MAX_M || n_x > ((size_t)1 << 30) || gamma_offset > ((size_t)1 << 30)) return VMPC_E_RANGE;
    if (!ctx || !a_row_ptr || !b_row_ptr || !a_const || !b_const || !z || !a_out || !b_out || (check == 1 && !first_bad) ||
        check < 0 || check > 2)
        return VMPC_E_INVAL;
    if (n_gates == 0) return VMPC_OK;
    return cs_triples<F>(ctx, a_row_ptr, a_col, a_vals, a_const, b_row_ptr, b_col, b_vals, b_const, gates, n_gates, n_x,
                         gamma_offset, z, 0, a_out, b_out, 0, 1, check, first_bad);
}

extern "C" int vmpc_fr_cs_triples_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                                      const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col,
                                      const void *b_vals, const void *b_const, const uint32_t *gates, size_t n_gates,
                                      size_t n_x, size_t gamma_offset, void *z, void *a_out, void *b_out, int check,
                                      uint32_t *first_bad) {
    return cs_triples_one<fr>(ctx, a_row_ptr, a_col, a_vals, a_const, b_row_ptr, b_col, b_vals, b_const, gates, n_gates, n_x,
                              gamma_offset, z, a_out, b_out, check, first_bad);
}

extern "C" int vmpc_bn256_fr_cs_triples_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col,
                                            const void *a_vals, const void *a_const, const uint32_t *b_row_ptr,
                                            const uint32_t *b_col, const void *b_vals, const void *b_const,
                                            const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset, void *z,
                                            void *a_out, void *b_out, int check, uint32_t *first_bad) {
    return cs_triples_one<frbn>(ctx, a_row_ptr, a_col, a_vals, a_const, b_row_ptr, b_col, b_vals, b_const, gates, n_gates,
                                n_x, gamma_offset, z, a_out, b_out, check, first_bad);
}

// the batch entry of either field: the checks, then n_wit witnesses with the caller's strides
template <class F>
static int cs_triples_many(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                           const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_vals,
                           const void *b_const, const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset,
                           void *z, size_t z_stride, void *a_out, void *b_out, size_t ab_stride, size_t n_wit, int check,
                           uint32_t *first_bad) {
    if (n_gates > VMPC_FR_CS_MAX_M || n_x > ((size_t)1 << 30) || gamma_offset > ((size_t)1 << 30) ||
        n_wit > VMPC_FR_CS_MAX_WIT || z_stride > ((size_t)1 << 31) || ab_stride > ((size_t)1 << 31) ||
        (n_gates && n_wit && (z_stride < gamma_offset + (check == 2 ? 0 : n_gates) || ab_stride < n_gates)))
        return VMPC_E_RANGE;
    if (!ctx || !a_row_ptr || !b_row_ptr || !a_const || !b_const || !z || !a_out || !b_out || (check == 1 && !first_bad) ||
        check < 0 || check > 2)
        return VMPC_E_INVAL;
    if (n_gates == 0 || n_wit == 0) return VMPC_OK;
    return cs_triples<F>(ctx, a_row_ptr, a_col, a_vals, a_const, b_row_ptr, b_col, b_vals, b_const, gates, n_gates, n_x,
                         gamma_offset, z, z_stride, a_out, b_out, ab_stride, n_wit, check, first_bad);
}

extern "C" int vmpc_fr_cs_triples_batch_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col,
                                            const void *a_vals, const void *a_const, const uint32_t *b_row_ptr,
                                            const uint32_t *b_col, const void *b_vals, const void *b_const,
                                            const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset, void *z,
                                            size_t z_stride, void *a_out, void *b_out, size_t ab_stride, size_t n_wit,
                                            int check, uint32_t *first_bad) {
    return cs_triples_many<fr>(ctx, a_row_ptr, a_col, a_vals, a_const, b_row_ptr, b_col, b_vals, b_const, gates, n_gates,
                               n_x, gamma_offset, z, z_stride, a_out, b_out, ab_stride, n_wit, check, first_bad);
}

extern "C" int vmpc_bn256_fr_cs_triples_batch_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col,
                                                  const void *a_vals, const void *a_const, const uint32_t *b_row_ptr,
                                                  const uint32_t *b_col, const void *b_vals, const void *b_const,
                                                  const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset,
                                                  void *z, size_t z_stride, void *a_out, void *b_out, size_t ab_stride,
                                                  size_t n_wit, int check, uint32_t *first_bad) {
    return cs_triples_many<frbn>(ctx, a_row_ptr, a_col, a_vals, a_const, b_row_ptr, b_col, b_vals, b_const, gates, n_gates,
                                 n_x, gamma_offset, z, z_stride, a_out, b_out, ab_stride, n_wit, check, first_bad);
}

// ---- factorial tables ---------------------------------------------------------------------------------------------------
// exclusive prefix products (csrc/fr_scan.h) of 1, 2, .., K (k! at index k) and of K, K-1, .., 1 (K! / (K-k)! at index k)
template <class F>
struct cs_fact_seq {
    uint32_t K;
    __device__ F operator()(const F &v, uint32_t q, uint32_t k) const {
        return f256_mul(v, f256_small<F>(q ? K - k : k + 1));
    }
};

// 1 / K! is the one inversion (Fermat), by the thread that holds K!
template <class F>
struct cs_fact_fin {
    uint32_t *inv_top;
    __device__ void operator()(uint32_t q, const F &total) const {
        if (q == 0) f256_st(inv_top, 0, f256_inv(total));
    }
};

// fact[k] = k!, ifact[k] = (1 / K!) (k+1) (k+2) .. K
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_ifact(uint32_t K, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ inv_top,
           uint32_t *__restrict__ fact, uint32_t *__restrict__ ifact) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > K) return;
    f256_st(fact, k, f256_ld<F>(pre, k));
    f256_st(ifact, k, f256_mul(f256_ld<F>(inv_top, 0), f256_ld<F>(pre, (long long)K + 1 + K - k)));
}

// The scratch of the two scans (tables, lagrange): the 2 (K + 1) prefix products, the runs' products and, for the
// tables, 1 / K!.  The GF(l) entries take it from the arena, the GF(n) entries from their caller, at these offsets.
struct cs_scan_scratch {
    size_t pre_b, run_b, bytes;
    explicit cs_scan_scratch(size_t K)
        : pre_b(2 * (K + 1) * 32), run_b(fr_scan_run_bytes<CS_RUN>(K, 2)),
          bytes(vmpc_align(pre_b) + vmpc_align(run_b) + vmpc_align(32)) {}
    uint32_t *pre(void *base) const { return (uint32_t *)base; }
    uint32_t *run(void *base) const { return (uint32_t *)((char *)base + vmpc_align(pre_b)); }
    uint32_t *inv_top(void *base) const { return (uint32_t *)((char *)base + vmpc_align(pre_b) + vmpc_align(run_b)); }
};

static int cs_tables_check(const vmpc_ctx *ctx, size_t K, const void *fact, const void *ifact) {
    if (K > 2 * VMPC_FR_CS_MAX_M + 1) return VMPC_E_RANGE;
    if (!ctx || !fact || !ifact || K == 0) return VMPC_E_INVAL;
    return VMPC_OK;
}

// checked arguments; pre, run, inv_top: the caller's (cs_scan_scratch)
template <class F>
static int cs_tables(vmpc_ctx *ctx, size_t K, uint32_t *pre, uint32_t *run, uint32_t *inv_top, void *fact, void *ifact) {
    const uint32_t n = (uint32_t)K + 1;
    vmpc_stage_scope sc(ctx, "cs_tables");
    VMPC_CHECK((fr_scan<F, CS_RUN>(ctx, cs_fact_seq<F>{(uint32_t)K}, (uint32_t)K, 2, run, pre, cs_fact_fin<F>{inv_top})));
    k_cs_ifact<F><<<(n + CS_WG - 1) / CS_WG, CS_WG, 0, ctx->stream>>>((uint32_t)K, pre, inv_top, (uint32_t *)fact,
                                                                     (uint32_t *)ifact);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_fr_cs_tables_dev(vmpc_ctx *ctx, size_t K, void *fact, void *ifact) {
    VMPC_CHECK(cs_tables_check(ctx, K, fact, ifact));
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const cs_scan_scratch s(K);
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(s.pre_b) + vmpc_align(s.run_b) + 1024));
    uint32_t *pre = (uint32_t *)vmpc_ws_take(ctx, s.pre_b);
    uint32_t *run = (uint32_t *)vmpc_ws_take(ctx, s.run_b);
    uint32_t *inv_top = (uint32_t *)vmpc_ws_take(ctx, 32);
    return cs_tables<fr>(ctx, K, pre, run, inv_top, fact, ifact);
}

extern "C" size_t vmpc_bn256_fr_cs_tables_scratch_bytes(size_t K) {
    return K == 0 || K > 2 * VMPC_FR_CS_MAX_M + 1 ? 0 : cs_scan_scratch(K).bytes;
}

extern "C" int vmpc_bn256_fr_cs_tables_dev(vmpc_ctx *ctx, size_t K, void *fact, void *ifact, void *scratch) {
    VMPC_CHECK(cs_tables_check(ctx, K, fact, ifact));
    if (!scratch) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const cs_scan_scratch s(K);
    return cs_tables<frbn>(ctx, K, s.pre(scratch), s.run(scratch), s.inv_top(scratch), fact, ifact);
}

// ---- Lagrange vector of the nodes 0..K at c -----------------------------------------------------------------------------
// exclusive prefix products of c - 0, c - 1, .. (pre) and of c - K, c - (K-1), .. (sfx)
template <class F>
struct cs_node_seq {
    F c;
    uint32_t K;
    __device__ F operator()(const F &v, uint32_t q, uint32_t k) const {
        return f256_mul(v, f256_sub(c, f256_small<F>(q ? K - k : k)));
    }
};

template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_lagrange(uint32_t K, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ ifact, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > K) return;
    F v = f256_mul(f256_ld<F>(ifact, j), f256_ld<F>(ifact, K - j));
    v = f256_mul(f256_mul(v, f256_ld<F>(pre, j)), f256_ld<F>(pre, (long long)K + 1 + K - j));
    if ((K - j) & 1u) v = f256_neg(v);
    f256_st(out, j, v);
}

// VMPC_E_RANGE, VMPC_E_INVAL, then VMPC_E_NONCANON for a c that is not below the modulus; cv: c as an element
template <class F>
static int cs_lagrange_check(const vmpc_ctx *ctx, const uint8_t c[32], size_t K, const void *ifact, const void *out, F &cv) {
    if (K > 2 * VMPC_FR_CS_MAX_M + 1) return VMPC_E_RANGE;
    if (!ctx || !c || !ifact || !out) return VMPC_E_INVAL;
    memcpy(cv.v, c, 32);
    return f256_is_canonical<F>(cv.v) ? VMPC_OK : VMPC_E_NONCANON;
}

// checked arguments; pre, run: the caller's (cs_scan_scratch)
template <class F>
static int cs_lagrange(vmpc_ctx *ctx, const F &cv, size_t K, uint32_t *pre, uint32_t *run, const void *ifact, void *out) {
    const uint32_t n = (uint32_t)K + 1;
    vmpc_stage_scope sc(ctx, "cs_lagrange");
    VMPC_CHECK((fr_scan<F, CS_RUN>(ctx, cs_node_seq<F>{cv, (uint32_t)K}, (uint32_t)K, 2, run, pre)));
    k_cs_lagrange<F><<<(n + CS_WG - 1) / CS_WG, CS_WG, 0, ctx->stream>>>((uint32_t)K, pre, (const uint32_t *)ifact,
                                                                        (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_fr_cs_lagrange_dev(vmpc_ctx *ctx, const uint8_t c[32], size_t K, const void *ifact, void *out) {
    fr cv;
    VMPC_CHECK(cs_lagrange_check(ctx, c, K, ifact, out, cv));
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const cs_scan_scratch s(K);
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_align(s.pre_b) + vmpc_align(s.run_b) + 1024));
    uint32_t *pre = (uint32_t *)vmpc_ws_take(ctx, s.pre_b);
    uint32_t *run = (uint32_t *)vmpc_ws_take(ctx, s.run_b);
    return cs_lagrange<fr>(ctx, cv, K, pre, run, ifact, out);
}

extern "C" size_t vmpc_bn256_fr_cs_lagrange_scratch_bytes(size_t K) {
    return K > 2 * VMPC_FR_CS_MAX_M + 1 ? 0 : cs_scan_scratch(K).bytes;
}

extern "C" int vmpc_bn256_fr_cs_lagrange_dev(vmpc_ctx *ctx, const uint8_t c[32], size_t K, const void *ifact, void *out,
                                             void *scratch) {
    frbn cv;
    VMPC_CHECK(cs_lagrange_check(ctx, c, K, ifact, out, cv));
    if (!scratch) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const cs_scan_scratch s(K);
    return cs_lagrange<frbn>(ctx, cv, K, s.pre(scratch), s.run(scratch), ifact, out);
}

// ---- extension of f, g to 0 and m+2 .. 2m ------------------------------------------------------------------------------
// uf[j-1] = a[j-1] w_j, ug[j-1] = b[j-1] w_j (j = 1..M); T[k] = 1 / k (k = 1..n_t-1), T[0] = 0
// Every kernel of the extension takes the witness from the grid's last dimension: witness w reads rows w of a, b
// (ab_stride scalars apart) and writes row w of the z tails (z_stride apart); uf, ug, s0 and the partial sums are K rows
// of the workspace, T and the weights are the circuit's and computed once.
// grid (max(M, n_t), witnesses); T by witness 0 only
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_prep(uint32_t M, uint32_t n_t, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, size_t ab_stride,
          const uint32_t *__restrict__ fact, const uint32_t *__restrict__ ifact, uint32_t *__restrict__ uf,
          uint32_t *__restrict__ ug, uint32_t *__restrict__ T) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t w = blockIdx.y;
    if (i < M) {
        const uint32_t j = i + 1;
        F wt = f256_mul(f256_ld<F>(ifact, j - 1), f256_ld<F>(ifact, M - j));
        if ((M - j) & 1u) wt = f256_neg(wt);
        f256_st(uf + w * M * 8, i, f256_mul(f256_ld<F>(a + w * ab_stride * 8, i), wt));
        f256_st(ug + w * M * 8, i, f256_mul(f256_ld<F>(b + w * ab_stride * 8, i), wt));
    }
    if (w == 0 && i < n_t) f256_st(T, i, i ? f256_mul(f256_ld<F>(fact, i - 1), f256_ld<F>(ifact, i)) : f256_zero<F>());
}

// one workgroup per witness: s0[2 w] = sum_i uf[i] T[i+1], s0[2 w + 1] = the same for ug (lane t takes i = t, t + 256,
// ..; the lanes' sums are added in lane order)
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_dot0(uint32_t M, const uint32_t *__restrict__ uf, const uint32_t *__restrict__ ug, const uint32_t *__restrict__ T,
          uint32_t *__restrict__ s0) {
    __shared__ F part[2][CS_WG];
    const uint32_t t = threadIdx.x;
    const size_t w = blockIdx.x;
    uf += w * M * 8;
    ug += w * M * 8;
    f256_acc af = f256_acc_zero(), ag = f256_acc_zero();
    for (uint32_t i = t; i < M; i += CS_WG) {
        const F y = f256_ld<F>(T, (long long)i + 1), xf = f256_ld<F>(uf, i), xg = f256_ld<F>(ug, i);
        f256_acc_mac(af, xf.v, y.v);
        f256_acc_mac(ag, xg.v, y.v);
    }
    part[0][t] = f256_acc_reduce<F>(af);
    part[1][t] = f256_acc_reduce<F>(ag);
    __syncthreads();
    if (t < 2) {
        F s = part[t][0];
        for (uint32_t i = 1; i < CS_WG; i++) s = f256_add(s, part[t][i]);
        f256_st(s0, (long long)(2 * w + t), s);
    }
}

// grid (tiles, segments, witnesses).  Row (w n_seg + s) of part_f: part_f[row n_out + o] = sum over segment s's i of
// uf_w[i] T[k_lo + o - i], o < n_out; part_g alike.
template <class F>
__global__ void __launch_bounds__(FR_CONV_TILE)
k_cs_corr(const uint32_t *__restrict__ uf, const uint32_t *__restrict__ ug, long long M, const uint32_t *__restrict__ T,
          long long n_t, long long k_lo, long long n_out, long long seg, uint32_t *__restrict__ part_f,
          uint32_t *__restrict__ part_g) {
    __shared__ uint32_t sU[2][FR_CONV_CHUNK * 8];
    __shared__ uint32_t sT[8 * FR_CONV_BROW];
    const long long o0 = (long long)blockIdx.x * FR_CONV_TILE, k0 = k_lo + o0;
    const long long seg_lo = (long long)blockIdx.y * seg;
    const size_t w = blockIdx.z;
    const uint32_t *const u[2] = {uf + w * (size_t)M * 8, ug + w * (size_t)M * 8};
    f256_acc acc[2] = {f256_acc_zero(), f256_acc_zero()};
    for (long long i0 = seg_lo; i0 < seg_lo + seg && i0 < M; i0 += FR_CONV_CHUNK)
        fr_conv_chunk<F, 2>(sU, sT, acc, u, M, T, n_t, k0, i0);
    const long long o = o0 + threadIdx.x;
    if (o < n_out) {
        const long long row = (long long)w * gridDim.y + blockIdx.y;
        f256_st(part_f, row * n_out + o, f256_acc_reduce<F>(acc[0]));
        f256_st(part_g, row * n_out + o, f256_acc_reduce<F>(acc[1]));
    }
}

// grid (outputs, witnesses).  zt = z + n of witness w: zt[0] = f(0), zt[1] = g(0), zt[2] = h(0), zt[2 + x] = h(x).
// Lane o < n_out: x = m + 2 + o; lane n_out: x = 0 and h(m + 1) = r_a r_b.
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_finish(uint32_t m, uint32_t n_out, uint32_t n_seg, const uint32_t *__restrict__ part_f,
            const uint32_t *__restrict__ part_g, const uint32_t *__restrict__ s0, const uint32_t *__restrict__ a,
            const uint32_t *__restrict__ b, size_t ab_stride, const uint32_t *__restrict__ fact,
            const uint32_t *__restrict__ ifact, uint32_t *__restrict__ zt, size_t z_stride) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t M = m + 1;
    const size_t w = blockIdx.y;
    zt += w * z_stride * 8;
    if (o < n_out) {
        const size_t rows = w * n_seg * (size_t)n_out * 8;
        const F sf = fr_partsum<F>(part_f + rows, n_out, n_seg, o), sg = fr_partsum<F>(part_g + rows, n_out, n_seg, o);
        const uint32_t x = m + 2 + o;
        const F lx = f256_mul(f256_ld<F>(fact, x - 1), f256_ld<F>(ifact, x - M - 1));
        f256_st(zt, 2 + (long long)x, f256_mul(f256_mul(lx, sf), f256_mul(lx, sg)));
    } else if (o == n_out) {
        // l(0) = (-1)^M M!, 1 / (0 - j) = -T[j]: f(0) = (-1)^(M+1) M! s0
        F l0 = f256_ld<F>(fact, M);
        if (!(M & 1u)) l0 = f256_neg(l0);
        const F f0 = f256_mul(l0, f256_ld<F>(s0, (long long)(2 * w))), g0 = f256_mul(l0, f256_ld<F>(s0, (long long)(2 * w + 1)));
        f256_st(zt, 0, f0);
        f256_st(zt, 1, g0);
        f256_st(zt, 2, f256_mul(f0, g0));
        // m = 0: z ends at h(0)
        if (m) f256_st(zt, 2 + (long long)M, f256_mul(f256_ld<F>(a + w * ab_stride * 8, m), f256_ld<F>(b + w * ab_stride * 8, m)));
    }
}

// the same sums of ONE witness with f and g kept apart and nothing multiplied: f_out[0] = f(0), f_out[1 + o] =
// f(m + 2 + o) for o < n_out, g alike (the shares of a secret-shared witness: a product of shares is not local,
// csrc/mpc_share.hip)
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_finish_fg(uint32_t m, uint32_t n_out, uint32_t n_seg, const uint32_t *__restrict__ part_f,
               const uint32_t *__restrict__ part_g, const uint32_t *__restrict__ s0, const uint32_t *__restrict__ fact,
               const uint32_t *__restrict__ ifact, uint32_t *__restrict__ f_out, uint32_t *__restrict__ g_out) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t M = m + 1;
    if (o < n_out) {
        const F sf = fr_partsum<F>(part_f, n_out, n_seg, o), sg = fr_partsum<F>(part_g, n_out, n_seg, o);
        const uint32_t x = m + 2 + o;
        const F lx = f256_mul(f256_ld<F>(fact, x - 1), f256_ld<F>(ifact, x - M - 1));
        f256_st(f_out, 1 + (long long)o, f256_mul(lx, sf));
        f256_st(g_out, 1 + (long long)o, f256_mul(lx, sg));
    } else if (o == n_out) {
        F l0 = f256_ld<F>(fact, M);
        if (!(M & 1u)) l0 = f256_neg(l0);
        f256_st(f_out, 0, f256_mul(l0, f256_ld<F>(s0, 0)));
        f256_st(g_out, 0, f256_mul(l0, f256_ld<F>(s0, 1)));
    }
}

// ---- the NTT route ------------------------------------------------------------------------------------------------------
// The sums k_cs_corr computes are the coefficients k = m+1 .. 2m-1 of u (M = m + 1 terms) x T (n_t = 2m + 2 terms).  In a
// CYCLIC product of length L, coefficient k also collects the full product's coefficients k + L, k + 2L, ..  The full
// product ends at index (M - 1) + (n_t - 1) = 3m + 1 and the smallest k wanted is m + 1: with L >= 2m + 2 the first
// alias, k + L >= 3m + 3, is past the end, so the window is alias-free for EVERY L >= 2m + 2 - not only for
// L >= 3m + 2, the whole product's length - and L is the smallest power of two >= 2m + 2 (m = 3: L = 8 = 2m + 2, met
// with equality).  A window coefficient is still a sum of at most M <= 2^20 products of residues < l:
// below 2^20 l^2 < 2^526, within the 551 bits of the 18 primes (csrc/ntt31.h).  Over GF(n) the residues are below
// n < 2^256: a window coefficient is below 2^20 n^2 < 2^532, inside the same 551 bits, and is reduced mod n instead.
// m < 2 has no correlation; at m = 2^20 (VMPC_FR_CS_MAX_M) 2m + 2 exceeds the longest transform, 2^21 points: 0, and
// the direct kernel is taken whatever the mode.
extern "C" size_t vmpc_fr_cs_extend_ntt_len(size_t m) {
    if (m < 2 || m > VMPC_FR_CS_MAX_M || 2 * m + 2 > ((size_t)1 << 21)) return 0;
    size_t L = 2;
    while (L < 2 * m + 2) L *= 2;
    return L;
}

static bool cs_extend_by_ntt(int mode, size_t m) {
    if (vmpc_fr_cs_extend_ntt_len(m) == 0) return false;
    return mode == VMPC_CS_EXTENSION_NTT || (mode == VMPC_CS_EXTENSION_AUTO && m >= VMPC_FR_CS_EXT_NTT_MIN);
}

extern "C" int vmpc_ctx_set_cs_extension(vmpc_ctx *ctx, int mode) {
    if (!ctx || mode < VMPC_CS_EXTENSION_DIRECT || mode > VMPC_CS_EXTENSION_NTT) return VMPC_E_INVAL;
    ctx->cs_extension = mode;
    return VMPC_OK;
}

extern "C" int vmpc_ctx_get_cs_extension(vmpc_ctx *ctx, int *mode) {
    if (!ctx || !mode) return VMPC_E_INVAL;
    *mode = ctx->cs_extension;
    return VMPC_OK;
}

// The segment length with the witnesses counted: tiles x segments x K workgroups against CS_TARGET_WGS.  A large batch
// ends at one segment per witness, so the partial sums never exceed K n_out scalars per polynomial beyond what the grid
// needs.  On the NTT route (ntt_cap > 0: the NTT's arena cap in force) there is ONE "segment", the reconstructed window,
// and the arena also holds the residues of T and of a group of the 2K rows u_f, u_g.
struct cs_batch_plan {
    long long seg;
    unsigned tiles, n_seg;
    size_t part_b, total_b;
    bool ntt;
    vmpc_ntt_plan np;
};

static cs_batch_plan cs_extend_batch_plan(size_t m, size_t n_wit, size_t ntt_cap = 0) {
    const long long M = (long long)m + 1, n_t = 2 * (long long)m + 2, n_out = m >= 2 ? (long long)m - 1 : 0;
    cs_batch_plan p;
    p.ntt = ntt_cap != 0;
    p.np = {};
    p.tiles = (unsigned)((n_out + FR_CONV_TILE - 1) / FR_CONV_TILE);
    p.seg = CS_MIN_SEG;
    while ((long long)p.tiles * ((M + p.seg - 1) / p.seg) * (long long)n_wit > CS_TARGET_WGS && p.seg < M) p.seg *= 2;
    p.n_seg = (unsigned)((M + p.seg - 1) / p.seg);
    if (p.ntt) p.n_seg = 1;
    p.part_b = vmpc_align(n_wit * (size_t)p.n_seg * (size_t)(n_out ? n_out : 1) * 32);
    p.total_b = 2 * vmpc_align(n_wit * (size_t)M * 32) + vmpc_align((size_t)n_t * 32) + 2 * p.part_b +
                vmpc_align(n_wit * 64) + 2048;
    if (p.ntt) {
        int log_l = 1;
        while (((size_t)1 << log_l) < vmpc_fr_cs_extend_ntt_len(m)) log_l++;
        p.np = vmpc_ntt_plan_at(log_l, true, 2 * n_wit, ntt_cap);
        p.total_b += p.np.bytes;
    }
    return p;
}

// the window of the cyclic products reduced into the field of F: the GF(l) or the GF(n) reconstruction of csrc/bn256_ntt.hip
static int cs_ntt_rows_mul(fr *, vmpc_ctx *ctx, const vmpc_ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb, uint32_t *ra,
                           const void *a, size_t na, size_t rows, const void *b, size_t nb, size_t k_lo, size_t k_cnt,
                           void *out) {
    return vmpc_ntt_fr_rows_mul(ctx, p, st, rb, ra, a, na, na, rows, b, nb, k_lo, k_cnt, out, k_cnt);
}
static int cs_ntt_rows_mul(frbn *, vmpc_ctx *ctx, const vmpc_ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb,
                           uint32_t *ra, const void *a, size_t na, size_t rows, const void *b, size_t nb, size_t k_lo,
                           size_t k_cnt, void *out) {
    return vmpc_ntt_frbn_rows_mul(ctx, p, st, rb, ra, a, na, na, rows, b, nb, k_lo, k_cnt, out, k_cnt);
}

// n_wit >= 1 witnesses, checked by the entries.  z_tail: k_cs_finish writes f(0), g(0) and the products of every
// witness; otherwise (one witness) k_cs_finish_fg writes f_out, g_out.
template <class F>
static int cs_extend(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t m, const void *fact,
                     const void *ifact, void *z_tail, size_t z_stride, void *f_out, void *g_out, size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const long long M = (long long)m + 1, n_t = 2 * (long long)m + 2;
    const long long n_out = m >= 2 ? (long long)m - 1 : 0, k_lo = (long long)m + 1;
    const bool by_ntt = cs_extend_by_ntt(ctx->cs_extension, m);
    const cs_batch_plan p = cs_extend_batch_plan(m, n_wit, by_ntt ? vmpc_ntt_arena_cap(ctx) : 0);
    VMPC_CHECK(vmpc_ws_reserve(ctx, p.total_b));        // before any launch: a batch too large for the arena does nothing
    uint32_t *uf, *ug, *T, *pf, *pg, *rb = nullptr, *ra = nullptr;
    if (p.ntt) {
        // u_f and u_g one after the other, the 2K rows of ONE product; their windows alike
        uf = (uint32_t *)vmpc_ws_take(ctx, 2 * n_wit * (size_t)M * 32);
        ug = uf + n_wit * (size_t)M * 8;
        T = (uint32_t *)vmpc_ws_take(ctx, (size_t)n_t * 32);
        pf = (uint32_t *)vmpc_ws_take(ctx, 2 * n_wit * (size_t)n_out * 32);
        pg = pf + n_wit * (size_t)n_out * 8;
    } else {
        uf = (uint32_t *)vmpc_ws_take(ctx, n_wit * (size_t)M * 32);
        ug = (uint32_t *)vmpc_ws_take(ctx, n_wit * (size_t)M * 32);
        T = (uint32_t *)vmpc_ws_take(ctx, (size_t)n_t * 32);
        pf = (uint32_t *)vmpc_ws_take(ctx, p.part_b);
        pg = (uint32_t *)vmpc_ws_take(ctx, p.part_b);
    }
    uint32_t *s0 = (uint32_t *)vmpc_ws_take(ctx, n_wit * 64);
    if (p.ntt) {
        rb = (uint32_t *)vmpc_ws_take(ctx, p.np.row_bytes * p.np.b_rows);
        ra = (uint32_t *)vmpc_ws_take(ctx, p.np.row_bytes * p.np.group);
    }
    const unsigned K = (unsigned)n_wit;
    {
        vmpc_stage_scope sc(ctx, "cs_extend_prep");
        k_cs_prep<F><<<dim3((unsigned)((n_t + CS_WG - 1) / CS_WG), K), CS_WG, 0, ctx->stream>>>(
            (uint32_t)M, (uint32_t)n_t, (const uint32_t *)a, (const uint32_t *)b, ab_stride, (const uint32_t *)fact,
            (const uint32_t *)ifact, uf, ug, T);
        VMPC_KERNEL_CHECK();
        k_cs_dot0<F><<<K, CS_WG, 0, ctx->stream>>>((uint32_t)M, uf, ug, T, s0);
        VMPC_KERNEL_CHECK();
    }
    if (p.ntt) {
        // T is split and transformed once per call, the rows in groups the NTT's arena cap and a grid dimension hold
        const vmpc_ntt_stages st = {"cs_extend_ntt_split", "cs_extend_ntt_fwd", "cs_extend_ntt_inv", "cs_extend_ntt_crt"};
        VMPC_CHECK(cs_ntt_rows_mul((F *)nullptr, ctx, p.np, st, rb, ra, uf, (size_t)M, 2 * n_wit, T, (size_t)n_t,
                                   (size_t)k_lo, (size_t)n_out, pf));
    } else if (n_out) {
        vmpc_stage_scope sc(ctx, "cs_extend_corr");
        k_cs_corr<F><<<dim3(p.tiles, p.n_seg, K), FR_CONV_TILE, 0, ctx->stream>>>(uf, ug, M, T, n_t, k_lo, n_out, p.seg, pf,
                                                                                 pg);
        VMPC_KERNEL_CHECK();
    }
    {
        vmpc_stage_scope sc(ctx, "cs_extend_finish");
        const unsigned grid = (unsigned)((n_out + 1 + CS_WG - 1) / CS_WG);
        if (z_tail)
            k_cs_finish<F><<<dim3(grid, K), CS_WG, 0, ctx->stream>>>(
                (uint32_t)m, (uint32_t)n_out, p.n_seg, pf, pg, s0, (const uint32_t *)a, (const uint32_t *)b, ab_stride,
                (const uint32_t *)fact, (const uint32_t *)ifact, (uint32_t *)z_tail, z_stride);
        else
            k_cs_finish_fg<F><<<grid, CS_WG, 0, ctx->stream>>>((uint32_t)m, (uint32_t)n_out, p.n_seg, pf, pg, s0,
                                                               (const uint32_t *)fact, (const uint32_t *)ifact,
                                                               (uint32_t *)f_out, (uint32_t *)g_out);
        VMPC_KERNEL_CHECK();
    }
    return VMPC_OK;
}

extern "C" int vmpc_fr_cs_extend_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact,
                                     const void *ifact, void *z_tail) {
    if (m > VMPC_FR_CS_MAX_M) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !fact || !ifact || !z_tail) return VMPC_E_INVAL;
    return cs_extend<fr>(ctx, a, b, 0, m, fact, ifact, z_tail, 0, nullptr, nullptr, 1);
}

extern "C" int vmpc_bn256_fr_cs_extend_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact,
                                           const void *ifact, void *z_tail) {
    if (m > VMPC_FR_CS_MAX_M) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !fact || !ifact || !z_tail) return VMPC_E_INVAL;
    return cs_extend<frbn>(ctx, a, b, 0, m, fact, ifact, z_tail, 0, nullptr, nullptr, 1);
}

extern "C" int vmpc_fr_cs_extend_fg_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact,
                                        const void *ifact, void *f_out, void *g_out) {
    if (m > VMPC_FR_CS_MAX_M) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !fact || !ifact || !f_out || !g_out) return VMPC_E_INVAL;
    return cs_extend<fr>(ctx, a, b, 0, m, fact, ifact, nullptr, 0, f_out, g_out, 1);
}

extern "C" int vmpc_bn256_fr_cs_extend_fg_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact,
                                              const void *ifact, void *f_out, void *g_out) {
    if (m > VMPC_FR_CS_MAX_M) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !fact || !ifact || !f_out || !g_out) return VMPC_E_INVAL;
    return cs_extend<frbn>(ctx, a, b, 0, m, fact, ifact, nullptr, 0, f_out, g_out, 1);
}

extern "C" size_t vmpc_fr_cs_extend_batch_bytes(size_t m, size_t n_wit) {
    if (m > VMPC_FR_CS_MAX_M || n_wit > VMPC_FR_CS_MAX_WIT || n_wit == 0) return 0;
    return cs_extend_batch_plan(m, n_wit).total_b;
}

// the same for the route ctx's mode (and its NTT arena cap) gives this m: what a call on ctx reserves
extern "C" size_t vmpc_fr_cs_extend_batch_bytes_ctx(const vmpc_ctx *ctx, size_t m, size_t n_wit) {
    if (m > VMPC_FR_CS_MAX_M || n_wit > VMPC_FR_CS_MAX_WIT || n_wit == 0) return 0;
    const bool ntt = ctx && cs_extend_by_ntt(ctx->cs_extension, m);
    return cs_extend_batch_plan(m, n_wit, ntt ? vmpc_ntt_arena_cap(ctx) : 0).total_b;
}

// the plan does not depend on the field (32-byte scalars, the same 18 primes): the GF(n) queries are the GF(l) ones
extern "C" size_t vmpc_bn256_fr_cs_extend_batch_bytes(size_t m, size_t n_wit) {
    return vmpc_fr_cs_extend_batch_bytes(m, n_wit);
}

extern "C" size_t vmpc_bn256_fr_cs_extend_batch_bytes_ctx(const vmpc_ctx *ctx, size_t m, size_t n_wit) {
    return vmpc_fr_cs_extend_batch_bytes_ctx(ctx, m, n_wit);
}

// the batch entry of either field: the checks, then n_wit witnesses with the caller's strides
template <class F>
static int cs_extend_many(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t m, const void *fact,
                          const void *ifact, void *z_tail, size_t z_stride, size_t n_wit) {
    if (m > VMPC_FR_CS_MAX_M || n_wit > VMPC_FR_CS_MAX_WIT || ab_stride > ((size_t)1 << 31) ||
        z_stride > ((size_t)1 << 31) || (n_wit && (ab_stride < m + 1 || z_stride < 2 * m + 3)))
        return VMPC_E_RANGE;
    if (!ctx || !a || !b || !fact || !ifact || !z_tail) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    return cs_extend<F>(ctx, a, b, ab_stride, m, fact, ifact, z_tail, z_stride, nullptr, nullptr, n_wit);
}

extern "C" int vmpc_fr_cs_extend_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t m,
                                           const void *fact, const void *ifact, void *z_tail, size_t z_stride,
                                           size_t n_wit) {
    return cs_extend_many<fr>(ctx, a, b, ab_stride, m, fact, ifact, z_tail, z_stride, n_wit);
}

extern "C" int vmpc_bn256_fr_cs_extend_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t m,
                                                 const void *fact, const void *ifact, void *z_tail, size_t z_stride,
                                                 size_t n_wit) {
    return cs_extend_many<frbn>(ctx, a, b, ab_stride, m, fact, ifact, z_tail, z_stride, n_wit);
}

// ---- transposed sparse mat-vec -----------------------------------------------------------------------------------------
extern "C" int vmpc_fr_cs_colsum_dev(vmpc_ctx *ctx, const void *weights, size_t n_rows, const uint32_t *rows,
                                     const void *vals, size_t nnz, const uint32_t *items, size_t n_items,
                                     const uint32_t *long_cols, size_t n_long, size_t n_partial, void *out, size_t n_out) {
    VMPC_CHECK(fr_colsum_check(ctx, weights, n_rows, (size_t)1 << 31, rows, vals, nnz, items, n_items, long_cols, n_long,
                               n_partial, out, n_out));
    return fr_colsum<fr>(ctx, "cs_colsum", true, weights, n_rows, rows, vals, nnz, items, n_items, long_cols, n_long,
                         n_partial, out, n_out);      // true: positions that no column maps to stay zero
}

extern "C" int vmpc_bn256_fr_cs_colsum_dev(vmpc_ctx *ctx, const void *weights, size_t n_rows, const uint32_t *rows,
                                           const void *vals, size_t nnz, const uint32_t *items, size_t n_items,
                                           const uint32_t *long_cols, size_t n_long, size_t n_partial, void *out,
                                           size_t n_out) {
    VMPC_CHECK(fr_colsum_check(ctx, weights, n_rows, (size_t)1 << 31, rows, vals, nnz, items, n_items, long_cols, n_long,
                               n_partial, out, n_out));
    return fr_colsum<frbn>(ctx, "cs_colsum", true, weights, n_rows, rows, vals, nnz, items, n_items, long_cols, n_long,
                           n_partial, out, n_out);
}

// ---- comparison --------------------------------------------------------------------------------------------------------
// the values compared are what f256_ld makes of the words: over GF(n) two encodings of one residue are equal
template <class F>
__global__ void __launch_bounds__(CS_WG)
k_cs_first_diff(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t n, uint32_t *__restrict__ first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!f256_equal(f256_ld<F>(a, i), f256_ld<F>(b, i))) atomicMin(first, i);
}

template <class F>
static int cs_first_diff(vmpc_ctx *ctx, const void *a, const void *b, size_t n, uint32_t *first_diff) {
    if (n > ((size_t)1 << 31)) return VMPC_E_RANGE;
    if (!ctx || !first_diff || (n && (!a || !b))) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "cs_first_diff");
    VMPC_HIP_CHECK(hipMemsetAsync(first_diff, 0xFF, 4, ctx->stream));
    if (n == 0) return VMPC_OK;
    k_cs_first_diff<F><<<(unsigned)((n + CS_WG - 1) / CS_WG), CS_WG, 0, ctx->stream>>>((const uint32_t *)a,
                                                                                       (const uint32_t *)b, (uint32_t)n,
                                                                                       first_diff);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

extern "C" int vmpc_fr_cs_first_diff_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, uint32_t *first_diff) {
    return cs_first_diff<fr>(ctx, a, b, n, first_diff);
}

extern "C" int vmpc_bn256_fr_cs_first_diff_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n,
                                               uint32_t *first_diff) {
    return cs_first_diff<frbn>(ctx, a, b, n, first_diff);
}
