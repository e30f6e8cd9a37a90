// The recombination of Trinocchio's proof shares in the exponent (demos/demo_zkp_trinocchio.py:86-93:
// proof[key] = sum_p lambda_p * share_p[key]): for n elements and M parties
//     out[e] = sum_{p < M} weights[p] parts[p][e]
// with SHARED scalars (the M Lagrange weights) and per-element points - the transpose of k_bnp_lincomb's shape (shared
// bases, per-row scalars), and a sum the general MSM path is far too heavy for: M = 3 terms per element, 8 K elements
// per batch of K proofs.
//
//   k_rc_recombine   one lane per (party, element), party-major: a workgroup is RC_WAVES wavefronts over the SAME 64
//                    elements, wavefront v taking the parties v, v + RC_WAVES, ..  A wavefront therefore holds ONE weight
//                    at a time, and whether to add at a bit is a decision on a kernel argument, read through the scalar
//                    data path: no lane branches on a bit of its own.  Each lane runs double-and-add over its party's
//                    point, adds the result to its running Jacobian sum, and the wavefronts' sums meet in LDS, where
//                    wavefront 0 adds them in wavefront order and normalises (one inversion per element).
//
// The host folds the sign: a weight above n / 2 travels as n - weight with a flag that negates the party's points.  The
// Lagrange weights at 0 of the nodes 1..M are the signed binomials (-1)^p C(M, p + 1) - for M = 3: 3, -3, 1 - so the
// chains of a real recombination are a handful of bits long and the kernel's time is the inversion; a chain starts at
// the weight's top bit (uniform).  Arbitrary weights cost a full 256-bit chain per party.
//
// The special cases of the group law are jac_madd's and jac_add's (csrc/sw256.h: an infinite operand, equal points ->
// doubling, opposite points -> infinity); the output is canonical affine, so the bytes do not depend on how the sum is
// organised.  No arena, no atomics, asynchronous on the context's stream.
#include <string.h>

#include "common.h"
#include "bn256_curve.h"
#include "fr_bn.h"
#include "share_combine.h"

#define RC_LANES 64                      // elements per workgroup: one wavefront wide
#define RC_WAVES 4                       // wavefronts per workgroup (G2: 3 x 64 x 192 B = 36 KiB of LDS)
#define RC_MAX ((size_t)1 << 31)         // n and the stride at most

// the weights travel as a kernel argument (2 KiB + 8 bytes), as k_r1cs_share_finish's do: |weight| and its sign
struct rc_weights {
    uint32_t w[VMPC_SHARE_MAX_PARTIES][8];
    uint64_t neg;                        // bit p: party p's points are negated
};

template <class C, class F>
__global__ void __launch_bounds__(RC_LANES * RC_WAVES)
k_rc_recombine(const uint32_t *__restrict__ parts, uint32_t parties, size_t n, size_t part_stride, rc_weights wts,
               uint32_t *__restrict__ out) {
    __shared__ uint32_t lds[(RC_WAVES - 1) * RC_LANES * C::ACC_WORDS];
    const uint32_t lane = threadIdx.x & (RC_LANES - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / RC_LANES));   // uniform
    const size_t e = (size_t)blockIdx.x * RC_LANES + lane;
    jac<F> sum = jac_identity<F>();
    for (uint32_t p = wave; p < parties; p += RC_WAVES) {
        int top = -1;                    // the weight's highest set word (uniform)
        for (int k = 7; k >= 0; k--)
            if (wts.w[p][k]) {
                top = k;
                break;
            }
        if (top < 0) continue;           // weight 0 adds nothing
        aff<F> a;
        a.inf = true;
        a.x = F::zero();
        a.y = F::zero();
        if (e < n) a = aff_load<F>(parts + (size_t)C::AFF_WORDS * ((size_t)p * part_stride + e));
        a.y = F::select(a.y, F::neg(a.y), (wts.neg >> p) & 1u);
        jac<F> acc = jac_identity<F>();
        for (int k = top; k >= 0; k--) {
            const uint32_t word = wts.w[p][k];
            for (int bit = k == top ? 31 - __clz(word) : 31; bit >= 0; bit--) {
                acc = jac_dbl<F>(acc);
                if ((word >> bit) & 1u) acc = jac_madd<F>(acc, a);
            }
        }
        sum = jac_add<F>(sum, acc);
    }
    if (wave) C::acc_st(lds + (size_t)C::ACC_WORDS * ((wave - 1) * RC_LANES + lane), sum);
    __syncthreads();
    if (wave) return;
    const uint32_t n_waves = parties < RC_WAVES ? parties : RC_WAVES;
    for (uint32_t v = 1; v < n_waves; v++)
        sum = jac_add<F>(sum, C::acc_ld(lds + (size_t)C::ACC_WORDS * ((v - 1) * RC_LANES + lane)));
    if (e < n) aff_store<F>(out + (size_t)C::AFF_WORDS * e, jac_to_affine<F>(sum));
}

// canonical weight -> (|weight|, sign): n - w where that is the smaller
static bool rc_fold_sign(uint32_t w[8]) {
    const uint32_t N[8] = VMPC_FRBN_N;
    uint32_t m[8], any = 0;
    int64_t b = 0;
    for (int i = 0; i < 8; i++) {
        b += (int64_t)N[i] - (int64_t)w[i];
        m[i] = (uint32_t)b;
        b >>= 32;
        any |= w[i];
    }
    if (!any) return false;
    for (int i = 7; i >= 0; i--) {
        if (m[i] < w[i]) break;
        if (m[i] > w[i]) return false;
    }
    memcpy(w, m, 32);                    // (m == w cannot happen: n is odd)
    return true;
}

extern "C" int vmpc_bn256_recombine_dev(vmpc_ctx *ctx, int group, const void *parts, size_t parties, size_t n,
                                        size_t part_stride, const uint8_t *weights, void *out) {
    if (parties > VMPC_SHARE_MAX_PARTIES || n > RC_MAX || part_stride > RC_MAX) return VMPC_E_RANGE;
    if (!ctx || (group != 1 && group != 2) || part_stride < n || (n && parties == 0) || (parties && !weights))
        return VMPC_E_INVAL;
    rc_weights w;
    memset(&w, 0, sizeof w);
    for (size_t p = 0; p < parties; p++) {
        memcpy(w.w[p], weights + 32 * p, 32);
        if (f256_geq_m<frbn>(w.w[p])) return VMPC_E_NONCANON;
        if (rc_fold_sign(w.w[p])) w.neg |= (uint64_t)1 << p;
    }
    if (n == 0) return VMPC_OK;
    if (!parts || !out) return VMPC_E_INVAL;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_recombine");
    const unsigned blocks = (unsigned)((n + RC_LANES - 1) / RC_LANES);
    if (group == 1)
        k_rc_recombine<G1, BnF1><<<blocks, RC_LANES * RC_WAVES, 0, ctx->stream>>>(
            (const uint32_t *)parts, (uint32_t)parties, n, part_stride, w, (uint32_t *)out);
    else
        k_rc_recombine<G2, BnF2><<<blocks, RC_LANES * RC_WAVES, 0, ctx->stream>>>(
            (const uint32_t *)parts, (uint32_t)parties, n, part_stride, w, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
