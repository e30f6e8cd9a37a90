// Per-element scalar multiplication on BN-256: out[i] = scalars[i] * points[i] for i < n, every point with a scalar of
// its own.  One party's pass over a jointly made pp of the knowledge-of-exponent pivot is this shape
// (knowledge_of_exponent.update_setup): element i of both sides times the party's own
// g z^(i+1), 2N points in G1 and 2N on the twist.  The other per-element kernels do not fit: gk_fixed_base has ONE base,
// k_bnp_lincomb shared bases, and k_rc_recombine shared scalars that it reads as kernel arguments.
//
//   k_scale_points   one lane per element, SC_LANES = 64 lanes (one wavefront) per workgroup so that a pp of a few
//                    thousand points still reaches every CU.  The lane loads its point (all-zero bytes: infinity),
//                    runs the branch-free 256-bit chain of csrc/scale_chain.h on the scalar's words as they stand in
//                    memory - a lane's bits are its own, so the bit selects between the doubled and the added
//                    accumulator instead of branching - and normalises: one inversion per lane, about a tenth of the
//                    chain, and no exchange between lanes at all.
//
// The output is canonical affine, so its bytes do not depend on how the chain is organised.  Points are not validated
// (vmpc_bn256_validate_dev).  No arena, no atomics, no LDS, asynchronous on the context's stream.
#include "common.h"
#include "bn256_curve.h"
#include "scale_chain.h"

#define SC_LANES 64                      // lanes per workgroup: one wavefront
#define SC_MAX ((size_t)1 << 31)         // n at most

template <class C, class F>
__global__ void __launch_bounds__(SC_LANES)
k_scale_points(const uint32_t *__restrict__ points, const uint32_t *__restrict__ scalars, size_t n,
               uint32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * SC_LANES + threadIdx.x;
    if (i >= n) return;
    const aff<F> a = aff_load<F>(points + (size_t)C::AFF_WORDS * i);
    const jac<F> r = scale_chain<F>(a, scalars + 8 * i);
    aff_store<F>(out + (size_t)C::AFF_WORDS * i, jac_to_affine<F>(r));
}

extern "C" int vmpc_bn256_scale_points_dev(vmpc_ctx *ctx, int group, const void *points, const void *scalars, size_t n,
                                           void *out) {
    if (n > SC_MAX) return VMPC_E_RANGE;
    if (!ctx || (group != 1 && group != 2) || (n && (!points || !scalars || !out))) return VMPC_E_INVAL;
    if (n == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    vmpc_stage_scope sc(ctx, "bn_scale_points");
    const unsigned blocks = (unsigned)((n + SC_LANES - 1) / SC_LANES);
    if (group == 1)
        k_scale_points<G1, BnF1><<<blocks, SC_LANES, 0, ctx->stream>>>((const uint32_t *)points, (const uint32_t *)scalars,
                                                                      n, (uint32_t *)out);
    else
        k_scale_points<G2, BnF2><<<blocks, SC_LANES, 0, ctx->stream>>>((const uint32_t *)points, (const uint32_t *)scalars,
                                                                      n, (uint32_t *)out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
