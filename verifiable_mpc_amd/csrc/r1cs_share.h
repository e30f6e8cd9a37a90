// The two per-element steps of a PRODUCT row of the R1CS solve on Shamir shares (csrc/bn256_r1cs_share.hip, DESIGN.md
// section 23) over a field of csrc/fr256.h.  c is ONE party's share vector of one witness: slot 0 holds 1 (every party's
// share of the constant), every other known slot this party's degree-t share of the wire.
//     deal     d = (V_i . c)(W_i . c), a degree-2t share of the product; a fresh degree-t sharing of d for parties
//              1..P goes out, out[q][e] = d + sum_{k=1..t} coeffs[k-1][e] (q + 1)^k.  d itself is stored nowhere.
//     finish   after the exchange: c[wire_i] = (sum_p weights[p] parts[p][e] - Y_i . c) inv_i, the weights the
//              M-point Lagrange weights at 0, which take the degree back to t.
// The dots are r1cs_row_dot of csrc/r1cs_solve.h (f256_acc, one reduction, its two shortcuts), the sum over the parts is
// share_combine_element of csrc/share_combine.h.  Entries whose column is above m and a new wire above m read / write
// nothing.  VMPC_HD: each kernel's per-lane step, host-testable (tests/native/r1cs_share_host_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fr256.h"
#include "r1cs_solve.h"
#include "share_combine.h"

// one matrix of the plan: a CSR over the plan's rows (vals: 32-byte canonical residues)
struct r1cs_csr {
    const uint32_t *row_ptr;
    const uint32_t *col;
    const uint32_t *vals;
};

// row r of the plan on the share vector c; e < n_e: the element's index in the round's tables (coeffs: t rows of n_e
// scalars, out: `parties` rows, out_stride scalars apart).  Horner in k at the small node q + 1.
template <class F>
VMPC_HD void r1cs_share_deal_element(const r1cs_csr &V, const r1cs_csr &W, uint32_t r, const uint32_t *c, uint32_t m,
                                     const uint32_t *coeffs, uint32_t t, uint32_t parties, size_t n_e, size_t e,
                                     uint32_t *out, size_t out_stride) {
    const F a = r1cs_row_dot<F>(V.row_ptr, V.col, V.vals, r, c, m);
    const F b = r1cs_row_dot<F>(W.row_ptr, W.col, W.vals, r, c, m);
    const F d = f256_mul(a, b);
    for (uint32_t q = 0; q < parties; q++) {
        F acc = d;
        if (t) {
            const F node = f256_small<F>(q + 1);
            acc = r1cs_ld<F>(coeffs, (long long)((size_t)(t - 1) * n_e + e));
            for (uint32_t k = t - 1; k >= 1; k--)
                acc = f256_add(f256_mul(acc, node), r1cs_ld<F>(coeffs, (long long)((size_t)(k - 1) * n_e + e)));
            acc = f256_add(f256_mul(acc, node), d);
        }
        r1cs_raw_st(out, (long long)((size_t)q * out_stride + e), acc.v);
    }
}

// false (and c untouched) where an element of parts is not a canonical residue; weights: canonical, checked by the caller
template <class F>
VMPC_HD bool r1cs_share_finish_element(const r1cs_csr &Y, const uint32_t *wire, const uint32_t *inv, uint32_t r,
                                       uint32_t *c, uint32_t m, const uint32_t *parts, uint32_t parties,
                                       size_t part_stride, size_t e, const uint32_t (*weights)[8]) {
    F v;
    if (!share_combine_element<F>(v, parts, parties, part_stride, e, weights, nullptr)) return false;
    v = f256_sub(v, r1cs_row_dot<F>(Y.row_ptr, Y.col, Y.vals, r, c, m));   // an empty dot is 0 and costs nothing
    const F f = r1cs_ld<F>(inv, r);
    if (!f256_equal(f, f256_one<F>())) v = f256_mul(v, f);   // coefficient 1: nothing to divide by
    const uint32_t s = wire[r];
    if (s <= m) r1cs_raw_st(c, s, v.v);
    return true;
}
