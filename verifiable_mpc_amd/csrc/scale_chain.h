// The per-point chain of vmpc_bn256_scale_points_dev (csrc/bn256_scale.hip): k * P for ONE point and ONE 256-bit
// scalar, the scalar used as it is (no reduction mod the group order).
//
// Left-to-right double-and-add over all 256 bits, taken branch-free: every bit costs a doubling AND a mixed addition,
// and the bit only selects which of the two results goes on (jac_select).  In the kernel a lane's bits are its own, so
// a branch on the bit would make a wavefront run the addition whenever ANY of its 64 lanes has the bit set - for
// random scalars always - and the divergent form saves nothing over this one while adding the branch's bookkeeping.
// The loop is uniform: 8 words x 32 bits whatever the scalar, the words read one at a time through `sc` (global
// memory in the kernel: no array of the lane's own is indexed by a loop variable, so nothing goes to scratch).
// The special cases of the group law are jac_dbl's and jac_madd's (csrc/sw256.h): the accumulator at infinity (every
// leading zero bit), P + P and P - P; a point at infinity on input stays there (jac_madd returns its first operand).
// VMPC_HD: host-testable (tests/native/scale_chain_host_test.cpp).
#pragma once
#include "sw256.h"

// the 32 bits of one scalar word, most significant first
template <class F>
VMPC_HD jac<F> scale_chain_word(jac<F> acc, const aff<F> &a, uint32_t word) {
    for (int bit = 31; bit >= 0; bit--) {
        acc = jac_dbl<F>(acc);
        const jac<F> sum = jac_madd<F>(acc, a);
        acc = jac_select<F>(acc, sum, ((word >> bit) & 1u) != 0);
    }
    return acc;
}

// sc: the scalar's 8 little-endian words
template <class F>
VMPC_HD jac<F> scale_chain(const aff<F> &a, const uint32_t *sc) {
    jac<F> acc = jac_identity<F>();
    for (int w = 7; w >= 0; w--) acc = scale_chain_word<F>(acc, a, sc[w]);
    return acc;
}
