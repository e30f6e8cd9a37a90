// Polynomial products over GF(n) of BN-256 in O(d log d): an NTT over the INTEGERS.  GF(n) itself has no NTT of useful
// length (csrc/bn256_koe.hip); the coefficients - any 32-byte values, not reduced first - are taken modulo NTT31_NP = 18
// primes c 2^22 + 1 < 2^31 (csrc/ntt31.h, csrc/ntt31_consts.h), convolved in each prime field, and the exact integer
// coefficient (< 2^532 < the primes' product) is rebuilt by Garner's digits and reduced mod n: the canonical residue the
// schoolbook kernel writes, bit for bit.  Same contract as vmpc_bn256_fr_poly_mul_batch_dev: K products of one shape, a
// window of the outputs, one b for all products when b_stride is 0.
//
//   layout         residues are uint32 in Montgomery form, prime-major: res[prime][row][L], L the power of two
//                  >= na + nb - 1 (at least 2), a row one operand of one product.
//   k_ntt_split    grid (L / 256, rows): a lane loads one scalar and stores its 18 residues (zeros past the operand).
//   k_ntt_lds      grid (L / B, prime, rows), B = min(L, NTT_LDS_LEN): the log B LOW stages of a transform on a
//                  contiguous block in LDS.  A transform of up to NTT_LDS_LEN points is this kernel alone.
//   k_ntt_cols     grid (L / (64 2^m), prime, rows): m <= 6 HIGH stages on a tile of 2^m rows x 64 consecutive
//                  columns (256-byte runs).  A longer transform is one or two of these passes plus k_ntt_lds: at the
//                  cap, L = 2^21, 5 + 5 + 11 stages.
//                  Forward is decimation in frequency (high stages first, output bit-reversed), inverse decimation in
//                  time from that order (low stages first): no permutation pass.  The pointwise product is fused into
//                  the load of the inverse's first pass (always k_ntt_lds).
//   twiddles       w^e for the 2^21-th root w and e < 2^20 is hi[e >> 10] lo[e & 1023]: two tables of 1024 entries per
//                  prime and direction (288 KiB in all), independent of L, built on the device once per context.  The
//                  stages of k_ntt_lds only meet e = 0 mod 1024: one table entry, staged in LDS, no product.
//   k_ntt_crt      grid (window outputs / 256, products): a lane gathers the 18 residues of one output of the window,
//                  multiplies by L^-1 (the inverse transform's scale is folded in here), runs Garner and Horner fully
//                  unrolled and stores the canonical residue.  Only the window is rebuilt; the transforms are whole.
//
// Arena: the residues of the shared b (or of a group's b rows) and of a group of a rows; n_wit is cut into groups so that
// the arena stays below NTT_ARENA_MAX (one row at the cap is 18 x 2^21 x 4 B = 151 MB).  A group boundary changes no
// value: every row is transformed on its own.  Integer sums in a fixed order, no atomics.
//
// Nothing but the last Horner reduction belongs to GF(n): k_ntt_crt and the loop over the groups (ntt_poly_mul_in, which
// works in residue buffers its caller took from the arena and reserves nothing) are templates over the field, and
// vmpc_ntt_fr_rows_mul is their GF(l) instantiation for Protocol 8's extension (csrc/circuit_sat.hip, DESIGN.md section
// 28), which plans a WRAPPED transform (vmpc_ntt_plan_at: L shorter than the whole product, its window alias-free).
//
// vmpc_ntt_tree_level (internal; csrc/bn256_qap_mtree.hip): one level of a subproduct tree,
// N_parent = N_left T_right + N_right T_left for all nodes and rows in one launch sequence - k_ntt_split_nodes,
// k_ntt_lds_pair and k_ntt_crt_nodes around the transform kernels above, which take the level's many short transforms
// as one flat row.
#include "common.h"
#include "fr_bn.h"
#include "ntt31.h"

#define NTT_WG 256
#define NTT_LDS_LOG 11
#define NTT_LDS_LEN (1 << NTT_LDS_LOG)
#define NTT_COL_W_LOG 6                   // a column tile is 64 consecutive values wide
#define NTT_COL_MAX_STAGES 6              // and at most 2^6 rows high: 4096 values, 16 KiB of LDS
#define NTT_TW_HALF 1024                  // entries of the lo and of the hi twiddle table
#define NTT_TW_PER_PRIME (2 * NTT_TW_HALF)
#define NTT_ARENA_MAX ((size_t)1 << 30)
#define NTT_MAX_GROUP ((size_t)65535)    // rows of one launch: a grid's y and z dimensions hold no more

static_assert(NTT_LDS_LEN == VMPC_BN256_FR_NTT_LDS_LEN, "the header's constant is this kernel's block length");

struct ntt_scale {
    uint32_t linv[NTT31_NP];
};

// table[dir][prime][0 .. 1023] = w^j, [1024 .. 2047] = w^(1024 j); w the 2^21-th root (dir 1: its inverse); canonical
__global__ void __launch_bounds__(NTT_WG) k_ntt_twiddles(uint32_t *__restrict__ table) {
    const uint32_t W[NTT31_NP] = NTT31_ROOT, WI[NTT31_NP] = NTT31_ROOT_INV;
    const int pr = blockIdx.x, dir = blockIdx.y;
    const ntt31_prime q = ntt31_prime_of(pr);
    const uint32_t w = ntt31_pow(dir ? WI[pr] : W[pr], 1u << (NTT31_TWO_ADICITY - 21), q);
    uint32_t *t = table + ((size_t)dir * NTT31_NP + pr) * NTT_TW_PER_PRIME;
    for (uint32_t j = threadIdx.x; j < NTT_TW_PER_PRIME; j += NTT_WG)
        t[j] = ntt31_pow(w, j < NTT_TW_HALF ? j : (j - NTT_TW_HALF) * NTT_TW_HALF, q);
}

// dst[prime][row][i] = src_row[i] mod prime for i < n, 0 for n <= i < L
__global__ void __launch_bounds__(NTT_WG)
k_ntt_split(const uint32_t *__restrict__ src, size_t stride, uint32_t n, uint32_t L, uint32_t rows,
            uint32_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x * NTT_WG + threadIdx.x;
    if (i >= L) return;
    const size_t row = blockIdx.y;
    uint32_t x[8];
    if (i < n) {
        const uint32_t *s = src + 8 * (row * stride + i);
#pragma unroll
        for (int l = 0; l < 8; l++) x[l] = s[l];
    }
#pragma unroll
    for (int pr = 0; pr < NTT31_NP; pr++)
        dst[((size_t)pr * rows + row) * L + i] = i < n ? ntt31_reduce256(x, ntt31_prime_of(pr)) : 0u;
}

// the log_b stages of a block of B = 2^log_b values staged in sx, sw the hi twiddle table (k_ntt_lds, k_ntt_lds_pair)
template <bool INV>
__device__ __forceinline__ void ntt_lds_stages(uint32_t *sx, const uint32_t *sw, uint32_t B, int log_b,
                                               const ntt31_prime &q) {
    for (int s = 0; s < log_b; s++) {
        const int lh = INV ? s : log_b - 1 - s;        // half-distance 2^lh
        const uint32_t h = 1u << lh;
        for (uint32_t t = threadIdx.x; t < B / 2; t += NTT_WG) {
            const uint32_t r = t & (h - 1), i = ((t >> lh) << (lh + 1)) | r;
            uint32_t a = sx[i], b = sx[i + h];
            const uint32_t w = sw[r << (10 - lh)];      // w^(r 2^(20 - lh)): a multiple of 1024 (lh <= 10)
            if (INV) ntt31_dit(a, b, w, q);
            else ntt31_dif(a, b, w, q);
            sx[i] = a;
            sx[i + h] = b;
        }
        __syncthreads();
    }
}

// The low stages (halves 1 .. B / 2) of a transform of x's rows, in place, on the block blockIdx.x of B = 2^log_b values.
// INV: decimation in time with the inverse twiddles, after x[i] *= y[i] (y: y_rows rows, 1 = one row for all).
template <bool INV>
__global__ void __launch_bounds__(NTT_WG)
k_ntt_lds(uint32_t *__restrict__ x, uint32_t rows, const uint32_t *__restrict__ y, uint32_t y_rows, uint32_t L,
          int log_b, const uint32_t *__restrict__ table) {
    __shared__ uint32_t sx[NTT_LDS_LEN];
    __shared__ uint32_t sw[NTT_TW_HALF];
    const int pr = blockIdx.y;
    const ntt31_prime q = ntt31_prime_of(pr);
    const uint32_t B = 1u << log_b, row = blockIdx.z;
    const size_t off = ((size_t)pr * rows + row) * L + (size_t)blockIdx.x * B;
    const uint32_t *tw = table + ((size_t)(INV ? 1 : 0) * NTT31_NP + pr) * NTT_TW_PER_PRIME + NTT_TW_HALF;
    for (uint32_t i = threadIdx.x; i < NTT_TW_HALF; i += NTT_WG) sw[i] = tw[i];
    if (INV) {
        const size_t yoff = ((size_t)pr * y_rows + (y_rows == 1 ? 0 : row)) * L + (size_t)blockIdx.x * B;
        for (uint32_t i = threadIdx.x; i < B; i += NTT_WG)
            sx[i] = ntt31_mul(x[off + i], ntt31_csub(y[yoff + i], q.p), q);
    } else {
        for (uint32_t i = threadIdx.x; i < B; i += NTT_WG) sx[i] = x[off + i];
    }
    __syncthreads();
    ntt_lds_stages<INV>(sx, sw, B, log_b, q);
    for (uint32_t i = threadIdx.x; i < B; i += NTT_WG) x[off + i] = sx[i];
}

// ---- a level of a subproduct tree (csrc/bn256_qap_mtree.hip): many short transforms, flat --------------------------
// A level has `rows` rows of `nodes` children each, every child one transform of L = 2^log_l points: too many for a
// grid dimension, so the transforms lie one after the other (res[prime][row nodes + node][L]) and the kernels above
// take them as ONE row of rows x nodes x L values - their stages never look beyond the 2^log_l block they are given.

// dst[prime][row nodes + node][i] = src[row row_stride + node node_stride + i] mod prime for i < n, 0 for n <= i < L;
// grid (nodes L / 256, rows' y, rows' z), row = z gridDim.y + y
__global__ void __launch_bounds__(NTT_WG)
k_ntt_split_nodes(const uint32_t *__restrict__ src, size_t row_stride, size_t node_stride, uint32_t n, int log_l,
                  uint32_t nodes, uint32_t *__restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * NTT_WG + threadIdx.x, per_row = (size_t)nodes << log_l;
    if (e >= per_row) return;
    const size_t row = (size_t)blockIdx.z * gridDim.y + blockIdx.y, rows = (size_t)gridDim.y * gridDim.z;
    const uint32_t node = (uint32_t)(e >> log_l), i = (uint32_t)e & ((1u << log_l) - 1);
    uint32_t x[8];
    if (i < n) {
        const uint32_t *s = src + 8 * (row * row_stride + node * node_stride + i);
#pragma unroll
        for (int l = 0; l < 8; l++) x[l] = s[l];
    }
#pragma unroll
    for (int pr = 0; pr < NTT31_NP; pr++)
        dst[((size_t)pr * rows + row) * per_row + e] = i < n ? ntt31_reduce256(x, ntt31_prime_of(pr)) : 0u;
}

// The inverse's first pass for the parents of a level: parent p of row r starts from x[2p] y[2p+1] + x[2p+1] y[2p]
// (x: the rows' child transforms, y: the level's T transforms, ONE set for all rows), the two products added in the
// residue domain (csrc/qap_mtree_plan.h has the bound), and goes to z[prime][r nodes / 2 + p][L].
// grid (rows (nodes / 2) (L / B), prime); nodes = 2^log_nodes >= 2
__global__ void __launch_bounds__(NTT_WG)
k_ntt_lds_pair(const uint32_t *__restrict__ x, const uint32_t *__restrict__ y, uint32_t *__restrict__ z, uint32_t rows,
               int log_nodes, int log_l, int log_b, const uint32_t *__restrict__ table) {
    __shared__ uint32_t sx[NTT_LDS_LEN];
    __shared__ uint32_t sw[NTT_TW_HALF];
    const int pr = blockIdx.y;
    const ntt31_prime q = ntt31_prime_of(pr);
    const uint32_t B = 1u << log_b;
    const size_t L = (size_t)1 << log_l, nodes = (size_t)1 << log_nodes;
    const size_t tp = blockIdx.x >> (log_l - log_b);                       // row (nodes / 2) + p
    const size_t inb = (size_t)(blockIdx.x & ((1u << (log_l - log_b)) - 1)) * B;
    const size_t row = tp >> (log_nodes - 1), p = tp & ((nodes >> 1) - 1);
    const size_t x0 = (((size_t)pr * rows + row) * nodes + 2 * p) * L + inb, x1 = x0 + L;
    const size_t y0 = ((size_t)pr * nodes + 2 * p) * L + inb, y1 = y0 + L;
    const size_t z0 = ((size_t)pr * rows * (nodes >> 1) + tp) * L + inb;
    const uint32_t *tw = table + ((size_t)NTT31_NP + pr) * NTT_TW_PER_PRIME + NTT_TW_HALF;
    for (uint32_t i = threadIdx.x; i < NTT_TW_HALF; i += NTT_WG) sw[i] = tw[i];
    for (uint32_t i = threadIdx.x; i < B; i += NTT_WG)
        sx[i] = ntt31_add(ntt31_mul(x[x0 + i], ntt31_csub(y[y1 + i], q.p), q),
                          ntt31_mul(x[x1 + i], ntt31_csub(y[y0 + i], q.p), q), q.p);
    __syncthreads();
    ntt_lds_stages<true>(sx, sw, B, log_b, q);
    for (uint32_t i = threadIdx.x; i < B; i += NTT_WG) z[z0 + i] = sx[i];
}

// m high stages, on the index bits [hb - m, hb), of a transform of x's rows, in place.  A tile: the 2^m values of those
// bits x 64 consecutive values of the bits [0, 6); blockIdx.x counts the other bits, [6, hb - m) and [hb, log L).
template <bool INV>
__global__ void __launch_bounds__(NTT_WG)
k_ntt_cols(uint32_t *__restrict__ x, uint32_t rows, uint32_t L, int hb, int m, const uint32_t *__restrict__ table) {
    __shared__ uint32_t sx[1 << (NTT_COL_MAX_STAGES + NTT_COL_W_LOG)];
    const int pr = blockIdx.y;
    const ntt31_prime q = ntt31_prime_of(pr);
    const int low_bits = hb - m - NTT_COL_W_LOG;
    const uint32_t ql = blockIdx.x & ((1u << low_bits) - 1), qh = blockIdx.x >> low_bits;
    const uint32_t base = (qh << hb) | (ql << NTT_COL_W_LOG);
    const int rs = hb - m;                               // a tile row is 2^rs values from the next
    uint32_t *xr = x + ((size_t)pr * rows + blockIdx.z) * L;
    const uint32_t *lo = table + ((size_t)(INV ? 1 : 0) * NTT31_NP + pr) * NTT_TW_PER_PRIME, *hi = lo + NTT_TW_HALF;
    const uint32_t count = 1u << (m + NTT_COL_W_LOG);
    for (uint32_t e = threadIdx.x; e < count; e += NTT_WG)
        sx[e] = xr[base + ((e >> NTT_COL_W_LOG) << rs) + (e & 63)];
    __syncthreads();
    for (int k = 0; k < m; k++) {
        const int s = INV ? k : m - 1 - k;               // tile-row bit s is index bit rs + s
        const int t = rs + s;
        for (uint32_t u = threadIdx.x; u < count / 2; u += NTT_WG) {
            const uint32_t c = u & 63, rr = u >> NTT_COL_W_LOG;
            const uint32_t r0 = ((rr >> s) << (s + 1)) | (rr & ((1u << s) - 1));
            const uint32_t e0 = (r0 << NTT_COL_W_LOG) | c, e1 = e0 + (64u << s);
            const uint32_t pos = (base + (r0 << rs) + c) & ((1u << t) - 1);      // the index mod the half-distance
            const uint32_t ex = pos << (20 - t);                                  // < 2^20
            const uint32_t w = ntt31_csub(ntt31_mul(hi[ex >> 10], lo[ex & 1023], q), q.p);
            uint32_t a = sx[e0], b = sx[e1];
            if (INV) ntt31_dit(a, b, w, q);
            else ntt31_dif(a, b, w, q);
            sx[e0] = a;
            sx[e1] = b;
        }
        __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < count; e += NTT_WG)
        xr[base + ((e >> NTT_COL_W_LOG) << rs) + (e & 63)] = sx[e];
}

// out_row[k - k_lo] = the integer coefficient k of row's product, mod the modulus of F (frbn: n; fr: l, the Protocol 8
// extension of csrc/circuit_sat.hip), for k in [k_lo, k_lo + k_cnt).  The coefficient is the CYCLIC product's: the
// caller has chosen L so that nothing aliases into the window.
template <class F>
__global__ void __launch_bounds__(NTT_WG)
k_ntt_crt(const uint32_t *__restrict__ res, uint32_t rows, uint32_t L, uint32_t k_lo, uint32_t k_cnt, ntt_scale sc,
          uint32_t *__restrict__ out, size_t out_stride) {
    const uint32_t j = blockIdx.x * NTT_WG + threadIdx.x;
    if (j >= k_cnt) return;
    const size_t row = blockIdx.y;
    uint32_t r[NTT31_NP];
#pragma unroll
    for (int pr = 0; pr < NTT31_NP; pr++) r[pr] = res[((size_t)pr * rows + row) * L + k_lo + j];
    f256_store(out + 8 * (row * out_stride + j), ntt31_crt_in<F>(r, sc.linv));
}

// a tree level's parents: out[tr k_cnt + j] = coefficient j < k_cnt of the flat transform tr, mod n (the parents of a
// row tile it: k_cnt = two children's coefficients); grid (transforms k_cnt / 256)
__global__ void __launch_bounds__(NTT_WG)
k_ntt_crt_nodes(const uint32_t *__restrict__ res, size_t transforms, int log_l, uint32_t k_cnt, ntt_scale sc,
                uint32_t *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * NTT_WG + threadIdx.x;
    if (e >= transforms * k_cnt) return;
    const size_t tr = e / k_cnt, at = (tr << log_l) + (e - tr * k_cnt);
    uint32_t r[NTT31_NP];
#pragma unroll
    for (int pr = 0; pr < NTT31_NP; pr++) r[pr] = res[((size_t)pr * transforms << log_l) + at];
    frbn_store(out + 8 * e, ntt31_crt(r, sc.linv));
}

// ---- host ----------------------------------------------------------------------------------------------------------
typedef vmpc_ntt_plan ntt_plan;      // csrc/common.h: log_l, L, row_bytes, group, b_rows, bytes

// the plan of n_wit products by transforms of 2^log_l points.  A group's rows lie on a grid's y (k_ntt_split,
// k_ntt_crt) or z (the transforms): at most 65535 of them, whatever the cap holds.
ntt_plan vmpc_ntt_plan_at(int log_l, bool shared_b, size_t n_wit, size_t cap) {
    ntt_plan p;
    p.log_l = log_l;
    p.L = (size_t)1 << p.log_l;
    p.row_bytes = (size_t)NTT31_NP * p.L * 4;
    const size_t fit = cap / p.row_bytes;                  // rows the cap holds
    size_t g = shared_b ? (fit > 1 ? fit - 1 : 1) : (fit > 2 ? fit / 2 : 1);
    if (g > NTT_MAX_GROUP) g = NTT_MAX_GROUP;
    p.group = g < n_wit ? g : n_wit;
    p.b_rows = shared_b ? 1 : p.group;
    p.bytes = vmpc_align(p.row_bytes * p.b_rows) + vmpc_align(p.row_bytes * p.group) + 512;
    return p;
}

// the whole product: L the power of two >= na + nb - 1
static ntt_plan ntt_plan_of(size_t na, size_t nb, bool shared_b, size_t n_wit, size_t cap) {
    int log_l = 1;
    while (((size_t)1 << log_l) < na + nb - 1) log_l++;
    return vmpc_ntt_plan_at(log_l, shared_b, n_wit, cap);
}

static int ntt_tables(vmpc_ctx *ctx) {
    if (ctx->ntt_twiddles) return VMPC_OK;
    VMPC_HIP_CHECK(hipMalloc(&ctx->ntt_twiddles, (size_t)2 * NTT31_NP * NTT_TW_PER_PRIME * 4));
    k_ntt_twiddles<<<dim3(NTT31_NP, 2), NTT_WG, 0, ctx->stream>>>((uint32_t *)ctx->ntt_twiddles);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

// the high stages of a transform longer than NTT_LDS_LEN: one pass of up to 6 stages, or two of about half each
template <bool INV>
static int ntt_high_stages(vmpc_ctx *ctx, uint32_t *x, size_t rows, const ntt_plan &p) {
    const int high = p.log_l - NTT_LDS_LOG;
    if (high <= 0) return VMPC_OK;
    const uint32_t *tw = (const uint32_t *)ctx->ntt_twiddles;
    int m[2] = {high, 0};
    if (high > NTT_COL_MAX_STAGES) {
        m[0] = (high + 1) / 2;
        m[1] = high - m[0];
    }
    // forward: from the top bit down; inverse: from bit NTT_LDS_LOG up
    int hb = INV ? NTT_LDS_LOG : p.log_l;
    for (int i = 0; i < 2 && m[i]; i++) {
        if (INV) hb += m[i];
        k_ntt_cols<INV><<<dim3((unsigned)(p.L >> (m[i] + NTT_COL_W_LOG)), NTT31_NP, (unsigned)rows), NTT_WG, 0,
                          ctx->stream>>>(x, (uint32_t)rows, (uint32_t)p.L, hb, m[i], tw);
        VMPC_KERNEL_CHECK();
        if (!INV) hb -= m[i];
    }
    return VMPC_OK;
}

static int ntt_split(vmpc_ctx *ctx, const char *stage, const void *src, size_t stride, size_t n, size_t rows,
                     const ntt_plan &p, uint32_t *dst) {
    vmpc_stage_scope s(ctx, stage);
    k_ntt_split<<<dim3((unsigned)((p.L + NTT_WG - 1) / NTT_WG), (unsigned)rows), NTT_WG, 0, ctx->stream>>>(
        (const uint32_t *)src, stride, (uint32_t)n, (uint32_t)p.L, (uint32_t)rows, dst);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

static int ntt_forward_launch(vmpc_ctx *ctx, uint32_t *x, size_t rows, const ntt_plan &p) {
    VMPC_CHECK(ntt_high_stages<false>(ctx, x, rows, p));
    const int log_b = p.log_l < NTT_LDS_LOG ? p.log_l : NTT_LDS_LOG;
    k_ntt_lds<false><<<dim3((unsigned)(p.L >> log_b), NTT31_NP, (unsigned)rows), NTT_WG, 0, ctx->stream>>>(
        x, (uint32_t)rows, nullptr, 0, (uint32_t)p.L, log_b, (const uint32_t *)ctx->ntt_twiddles);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

static int ntt_forward(vmpc_ctx *ctx, const char *stage, uint32_t *x, size_t rows, const ntt_plan &p) {
    vmpc_stage_scope s(ctx, stage);
    return ntt_forward_launch(ctx, x, rows, p);
}

// x *= y pointwise, then the inverse transform of x (not yet scaled by 1 / L: k_ntt_crt does that)
static int ntt_inverse(vmpc_ctx *ctx, const char *stage, uint32_t *x, size_t rows, const uint32_t *y, size_t y_rows,
                       const ntt_plan &p) {
    vmpc_stage_scope s(ctx, stage);
    const int log_b = p.log_l < NTT_LDS_LOG ? p.log_l : NTT_LDS_LOG;
    k_ntt_lds<true><<<dim3((unsigned)(p.L >> log_b), NTT31_NP, (unsigned)rows), NTT_WG, 0, ctx->stream>>>(
        x, (uint32_t)rows, y, (uint32_t)y_rows, (uint32_t)p.L, log_b, (const uint32_t *)ctx->ntt_twiddles);
    VMPC_KERNEL_CHECK();
    return ntt_high_stages<true>(ctx, x, rows, p);
}

// The product in residue buffers the CALLER has taken from the arena (no reservation here): rb holds
// p.row_bytes x p.b_rows bytes, ra p.row_bytes x p.group.  n_wit >= 1 rows of a in groups of p.group, b one row for all
// (b_stride 0) or a row per product; the transforms have 2^p.log_l points whatever na + nb is, and out_w[k - k_lo] is
// coefficient k of the CYCLIC product of that length, mod the modulus of F - the caller knows that nothing aliases
// into [k_lo, k_lo + k_cnt) (vmpc_ntt_poly_mul: L >= na + nb - 1; cs_extend of csrc/circuit_sat.hip: its own argument).
// The integer bound is the caller's as well: every coefficient a sum of at most 2^20 products of 32-byte values.
template <class F>
static int ntt_poly_mul_in(vmpc_ctx *ctx, const ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb, uint32_t *ra,
                           const void *a, size_t a_stride, size_t na, const void *b, size_t b_stride, size_t nb,
                           size_t k_lo, size_t k_cnt, void *out, size_t out_stride, size_t n_wit) {
    const bool shared_b = b_stride == 0;
    VMPC_CHECK(ntt_tables(ctx));
    ntt_scale sc;
    const uint32_t P[NTT31_NP] = NTT31_PRIMES;
    for (int i = 0; i < NTT31_NP; i++) sc.linv[i] = ntt31_inv_pow2(p.log_l, P[i]);
    for (size_t w0 = 0; w0 < n_wit; w0 += p.group) {
        const size_t g = n_wit - w0 < p.group ? n_wit - w0 : p.group;
        if (!shared_b || w0 == 0) {
            const size_t rows = shared_b ? 1 : g;
            VMPC_CHECK(ntt_split(ctx, st.split, (const char *)b + 32 * w0 * b_stride, b_stride, nb, rows, p, rb));
            VMPC_CHECK(ntt_forward(ctx, st.fwd, rb, rows, p));
        }
        VMPC_CHECK(ntt_split(ctx, st.split, (const char *)a + 32 * w0 * a_stride, a_stride, na, g, p, ra));
        VMPC_CHECK(ntt_forward(ctx, st.fwd, ra, g, p));
        VMPC_CHECK(ntt_inverse(ctx, st.inv, ra, g, rb, shared_b ? 1 : g, p));
        {
            vmpc_stage_scope s(ctx, st.crt);
            k_ntt_crt<F><<<dim3((unsigned)((k_cnt + NTT_WG - 1) / NTT_WG), (unsigned)g), NTT_WG, 0, ctx->stream>>>(
                ra, (uint32_t)g, (uint32_t)p.L, (uint32_t)k_lo, (uint32_t)k_cnt, sc,
                (uint32_t *)out + 8 * w0 * out_stride, out_stride);
            VMPC_KERNEL_CHECK();
        }
    }
    return VMPC_OK;
}

// n_wit >= 1 products of a non-empty window, checked by the entries (csrc/bn256_koe.hip's koe_poly_mul hands over here)
int vmpc_ntt_poly_mul(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na, const void *b, size_t b_stride,
                      size_t nb, size_t k_lo, size_t k_cnt, void *out, size_t out_stride, size_t n_wit) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const ntt_plan p = ntt_plan_of(na, nb, b_stride == 0, n_wit, vmpc_ntt_arena_cap(ctx));
    VMPC_CHECK(vmpc_ws_reserve(ctx, p.bytes));      // before any launch
    uint32_t *rb = (uint32_t *)vmpc_ws_take(ctx, p.row_bytes * p.b_rows);
    uint32_t *ra = (uint32_t *)vmpc_ws_take(ctx, p.row_bytes * p.group);
    const vmpc_ntt_stages st = {"bn_fr_ntt_split", "bn_fr_ntt_fwd", "bn_fr_ntt_inv", "bn_fr_ntt_crt"};
    return ntt_poly_mul_in<frbn>(ctx, p, st, rb, ra, a, a_stride, na, b, b_stride, nb, k_lo, k_cnt, out, out_stride,
                                 n_wit);
}

// The window [k_lo, k_lo + k_cnt) of the cyclic products, of 2^p.log_l points, of `rows` rows of a with ONE b, over
// GF(l) of Ed25519, in the caller's residue buffers (p = vmpc_ntt_plan_at(log_l, true, rows, cap); rb one row, ra
// p.group rows): the correlation of Protocol 8's extension (cs_extend, csrc/circuit_sat.hip), which has reserved.
int vmpc_ntt_fr_rows_mul(vmpc_ctx *ctx, const vmpc_ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb, uint32_t *ra,
                         const void *a, size_t a_stride, size_t na, size_t rows, const void *b, size_t nb, size_t k_lo,
                         size_t k_cnt, void *out, size_t out_stride) {
    return ntt_poly_mul_in<fr>(ctx, p, st, rb, ra, a, a_stride, na, b, 0, nb, k_lo, k_cnt, out, out_stride, rows);
}

// the same window reduced mod n, the BN-256 order: the extension of Protocol 8 over GF(n) (cs_extend<frbn>)
int vmpc_ntt_frbn_rows_mul(vmpc_ctx *ctx, const vmpc_ntt_plan &p, const vmpc_ntt_stages &st, uint32_t *rb, uint32_t *ra,
                           const void *a, size_t a_stride, size_t na, size_t rows, const void *b, size_t nb, size_t k_lo,
                           size_t k_cnt, void *out, size_t out_stride) {
    return ntt_poly_mul_in<frbn>(ctx, p, st, rb, ra, a, a_stride, na, b, 0, nb, k_lo, k_cnt, out, out_stride, rows);
}

size_t vmpc_ntt_arena_cap(const vmpc_ctx *ctx) {
    return ctx ? (ctx->ntt_arena_cap ? ctx->ntt_arena_cap : NTT_ARENA_MAX) : NTT_ARENA_MAX;
}

size_t vmpc_ntt_poly_mul_bytes(size_t na, size_t nb, bool shared_b, size_t n_wit, size_t cap) {
    return ntt_plan_of(na, nb, shared_b, n_wit, cap).bytes;
}

static int ntt_tree_log_l(size_t m) {
    int log_l = 1;
    while (((size_t)1 << log_l) < 2 * m) log_l++;
    return log_l;
}

// the residues of the level's T (one set), of the rows' children and of their parents
size_t vmpc_ntt_tree_level_bytes(size_t m, size_t nodes, size_t rows) {
    const size_t t = (size_t)NTT31_NP * 4 * (nodes << ntt_tree_log_l(m));
    return vmpc_align(t) + vmpc_align(t * rows) + vmpc_align(t * rows / 2) + 768;
}

// One level of a subproduct tree (csrc/bn256_qap_mtree.hip), ONE launch sequence for all nodes and rows:
//     nout[row][p] = nin[row][2p] T[2p+1] + nin[row][2p+1] T[2p]     for the 2^(log_nodes - 1) parents p of every row
// T: 2^log_nodes nodes of m + 1 coefficients each, one after the other; nin: rows of 2^log_nodes children of m
// coefficients, a row nodes x m scalars from the next; nout: the parents of 2 m coefficients in the same rows.
// rows = rows_y x rows_z (two grid dimensions), at least 1; log_nodes >= 1; everything checked by the caller, who has
// also kept rows x nodes x L within vmpc_ntt_arena_cap (below 2^32 values per prime).
int vmpc_ntt_tree_level(vmpc_ctx *ctx, const void *T, size_t m, int log_nodes, const void *nin, void *nout,
                        size_t rows_y, size_t rows_z) {
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    const int log_l = ntt_tree_log_l(m), log_b = log_l < NTT_LDS_LOG ? log_l : NTT_LDS_LOG;
    const size_t nodes = (size_t)1 << log_nodes, rows = rows_y * rows_z, per_row = nodes << log_l;
    const size_t t_b = (size_t)NTT31_NP * 4 * per_row;
    VMPC_CHECK(vmpc_ws_reserve(ctx, vmpc_ntt_tree_level_bytes(m, nodes, rows)));      // before any launch
    uint32_t *rb = (uint32_t *)vmpc_ws_take(ctx, t_b);
    uint32_t *ra = (uint32_t *)vmpc_ws_take(ctx, t_b * rows);
    uint32_t *rp = (uint32_t *)vmpc_ws_take(ctx, t_b * rows / 2);
    VMPC_CHECK(ntt_tables(ctx));
    ntt_scale sc;
    const uint32_t P[NTT31_NP] = NTT31_PRIMES;
    for (int i = 0; i < NTT31_NP; i++) sc.linv[i] = ntt31_inv_pow2(log_l, P[i]);
    ntt_plan flat;      // the transforms one after the other: the stages of log_l, the grid of all values
    flat.log_l = log_l;
    const unsigned split_x = (unsigned)((per_row + NTT_WG - 1) / NTT_WG);
    vmpc_stage_scope s(ctx, "bn_qap_mtree_level");
    k_ntt_split_nodes<<<dim3(split_x, 1, 1), NTT_WG, 0, ctx->stream>>>((const uint32_t *)T, 0, m + 1, (uint32_t)(m + 1),
                                                                      log_l, (uint32_t)nodes, rb);
    VMPC_KERNEL_CHECK();
    flat.L = per_row;
    VMPC_CHECK(ntt_forward_launch(ctx, rb, 1, flat));
    k_ntt_split_nodes<<<dim3(split_x, (unsigned)rows_y, (unsigned)rows_z), NTT_WG, 0, ctx->stream>>>(
        (const uint32_t *)nin, nodes * m, m, (uint32_t)m, log_l, (uint32_t)nodes, ra);
    VMPC_KERNEL_CHECK();
    flat.L = rows * per_row;
    VMPC_CHECK(ntt_forward_launch(ctx, ra, 1, flat));
    k_ntt_lds_pair<<<dim3((unsigned)((rows * (nodes / 2)) << (log_l - log_b)), NTT31_NP), NTT_WG, 0, ctx->stream>>>(
        ra, rb, rp, (uint32_t)rows, log_nodes, log_l, log_b, (const uint32_t *)ctx->ntt_twiddles);
    VMPC_KERNEL_CHECK();
    flat.L = rows * per_row / 2;
    VMPC_CHECK(ntt_high_stages<true>(ctx, rp, 1, flat));
    const size_t outs = rows * nodes * m;
    k_ntt_crt_nodes<<<(unsigned)((outs + NTT_WG - 1) / NTT_WG), NTT_WG, 0, ctx->stream>>>(
        rp, rows * (nodes / 2), log_l, (uint32_t)(2 * m), sc, (uint32_t *)nout);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}

static bool ntt_batch_in_range(size_t na, size_t nb, size_t k_lo, size_t k_cnt, size_t n_wit) {
    return n_wit <= VMPC_BN256_QAP_MAX_WIT && na <= VMPC_BN256_FR_POLY_MAX && nb <= VMPC_BN256_FR_POLY_MAX &&
           k_lo <= 2 * VMPC_BN256_FR_POLY_MAX && k_cnt <= 2 * VMPC_BN256_FR_POLY_MAX &&
           (k_cnt == 0 || k_lo + k_cnt + 1 <= na + nb);
}

extern "C" size_t vmpc_bn256_fr_poly_mul_ntt_batch_bytes(size_t na, size_t nb, size_t k_lo, size_t k_cnt,
                                                         size_t n_wit) {
    if (!ntt_batch_in_range(na, nb, k_lo, k_cnt, n_wit) || na == 0 || nb == 0 || k_cnt == 0 || n_wit == 0) return 0;
    // (the larger of the two layouts: the entry does not know the stride of b here)
    const size_t s = ntt_plan_of(na, nb, true, n_wit, NTT_ARENA_MAX).bytes;
    const size_t d = ntt_plan_of(na, nb, false, n_wit, NTT_ARENA_MAX).bytes;
    return s > d ? s : d;
}

extern "C" int vmpc_bn256_fr_poly_mul_ntt_batch_dev(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na,
                                                    const void *b, size_t b_stride, size_t nb, size_t k_lo, size_t k_cnt,
                                                    void *out, size_t out_stride, size_t n_wit) {
    const size_t cap = (size_t)1 << 31;
    if (!ntt_batch_in_range(na, nb, k_lo, k_cnt, n_wit) || a_stride > cap || b_stride > cap || out_stride > cap ||
        (n_wit && (a_stride < na || (b_stride && b_stride < nb) || out_stride < k_cnt)))
        return VMPC_E_RANGE;
    if (!ctx || !a || !b || !out || na == 0 || nb == 0) return VMPC_E_INVAL;
    if (n_wit == 0 || k_cnt == 0) return VMPC_OK;
    return vmpc_ntt_poly_mul(ctx, a, a_stride, na, b, b_stride, nb, k_lo, k_cnt, out, out_stride, n_wit);
}

// the whole product: the window [0, na + nb - 1) of one pair
extern "C" int vmpc_bn256_fr_poly_mul_ntt_dev(vmpc_ctx *ctx, const void *a, size_t na, const void *b, size_t nb,
                                              void *out) {
    if (na > VMPC_BN256_FR_POLY_MAX || nb > VMPC_BN256_FR_POLY_MAX) return VMPC_E_RANGE;
    if (!ctx || !a || !b || !out || na == 0 || nb == 0) return VMPC_E_INVAL;
    return vmpc_ntt_poly_mul(ctx, a, na, na, b, nb, nb, 0, na + nb - 1, out, na + nb - 1, 1);
}

extern "C" int vmpc_ctx_set_poly_product(vmpc_ctx *ctx, int mode) {
    if (!ctx || mode < VMPC_POLY_PRODUCT_SCHOOLBOOK || mode > VMPC_POLY_PRODUCT_NTT) return VMPC_E_INVAL;
    ctx->poly_product = mode;
    return VMPC_OK;
}

extern "C" int vmpc_ctx_get_poly_product(vmpc_ctx *ctx, int *mode) {
    if (!ctx || !mode) return VMPC_E_INVAL;
    *mode = ctx->poly_product;
    return VMPC_OK;
}

extern "C" int vmpc_ctx_set_ntt_arena_cap(vmpc_ctx *ctx, size_t bytes) {
    if (!ctx) return VMPC_E_INVAL;
    ctx->ntt_arena_cap = bytes;
    return VMPC_OK;
}
