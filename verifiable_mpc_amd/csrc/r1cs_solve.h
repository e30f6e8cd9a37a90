// One row of the R1CS solve (csrc/bn256_r1cs_solve.hip) over a field of csrc/fr256.h: the three
// sparse dots a, b, y of the row over the KNOWN wires of one witness, then by the row's kind
//     check   nothing stored; failed where a b != y
//     Y       c_s = (a b - y) inv                 (inv = 1 / gamma, the new wire's coefficient in Y)
//     A       c_s = (y / b - a) inv               (inv = 1 / alpha, its coefficient in V; failed where b = 0)
//     B       c_s = (y / a - b) inv               (inv = 1 / beta, its coefficient in W; failed where a = 0)
// The new wire's own entry is not among the row's stored entries (the host plan removed it), so nothing here reads a
// slot that no earlier row wrote.  A zero divisor stores 0 and reports failed: f256_inv maps 0 to 0, nothing faults.
// Entries whose column is above m and a new wire above m read / write nothing (a plan made by pynocchio.SolvePlan has
// none).  VMPC_HD: every kernel's per-row step, host-testable (tests/native/r1cs_solve_host_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fr256.h"
#include "share_combine.h"   // f256_raw_ld

#define R1CS_KIND_CHECK 0u
#define R1CS_KIND_Y 1u
#define R1CS_KIND_A 2u
#define R1CS_KIND_B 3u

// the plan's rows in level order: one CSR per matrix (vals: 32-byte canonical residues), kind, new wire and inverse
// coefficient per row
struct r1cs_plan {
    const uint32_t *row_ptr[3];
    const uint32_t *col[3];
    const uint32_t *vals[3];
    const uint32_t *kind;
    const uint32_t *wire;
    const uint32_t *inv;
};

VMPC_HD void r1cs_raw_st(uint32_t *p, long long i, const uint32_t w[8]) {
#ifdef __HIPCC__
    uint4 *q = (uint4 *)(p + 8 * i);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
    for (int k = 0; k < 8; k++) p[8 * i + k] = w[k];
#endif
}

template <class F>
VMPC_HD F r1cs_ld(const uint32_t *p, long long i) {
    uint32_t w[8];
    f256_raw_ld(w, p, i);
    return f256_load<F>(w);
}

// sum over the row's entries of vals[e] c[col[e]]: unreduced products in f256_acc, ONE reduction.  The two shapes that
// the reference's flattener writes most need no arithmetic at all and take none: an empty dot is 0, and a single entry
// of coefficient 1 is the wire itself (the accumulator's reduction is three Barrett reductions, a product's is one:
// on a chain of x * t rows this is the difference between 17 and 3 us per level).  The same
// canonical residue either way.
template <class F>
VMPC_HD F r1cs_row_dot(const uint32_t *row_ptr, const uint32_t *col, const uint32_t *vals, uint32_t r, const uint32_t *c,
                       uint32_t m) {
    const uint32_t e0 = row_ptr[r], e1 = row_ptr[r + 1];
    if (e1 <= e0) return f256_zero<F>();
    if (e1 - e0 == 1 && col[e0] <= m && f256_equal(r1cs_ld<F>(vals, e0), f256_one<F>())) return r1cs_ld<F>(c, col[e0]);
    f256_acc acc = f256_acc_zero();
    for (uint32_t e = e0; e < e1; e++) {
        const uint32_t k = col[e];
        if (k > m) continue;
        const F x = r1cs_ld<F>(vals, e), v = r1cs_ld<F>(c, k);
        f256_acc_mac(acc, x.v, v.v);
    }
    return f256_acc_reduce<F>(acc);
}

// row r (level-order position) on the witness c (slots 0..m): stores the new wire, returns true where the row FAILED
template <class F>
VMPC_HD bool r1cs_solve_row(const r1cs_plan &p, uint32_t r, uint32_t *c, uint32_t m) {
    const uint32_t kind = p.kind[r], s = p.wire[r];
    const F a = r1cs_row_dot<F>(p.row_ptr[0], p.col[0], p.vals[0], r, c, m);
    const F b = r1cs_row_dot<F>(p.row_ptr[1], p.col[1], p.vals[1], r, c, m);
    const F y = r1cs_row_dot<F>(p.row_ptr[2], p.col[2], p.vals[2], r, c, m);
    if (kind == R1CS_KIND_CHECK) return !f256_equal(f256_mul(a, b), y);
    bool failed = false;
    F v;
    if (kind == R1CS_KIND_Y) {
        v = f256_sub(f256_mul(a, b), y);
    } else {
        const F &div = kind == R1CS_KIND_A ? b : a, &rest = kind == R1CS_KIND_A ? a : b;
        failed = f256_equal(div, f256_zero<F>());
        v = f256_sub(f256_mul(y, f256_inv(div)), rest);
    }
    const F inv = r1cs_ld<F>(p.inv, r);
    if (failed) v = f256_zero<F>();
    else if (!f256_equal(inv, f256_one<F>())) v = f256_mul(v, inv);   // coefficient 1: nothing to divide by
    if (s <= m) r1cs_raw_st(c, s, v.v);
    return failed;
}

// slot i <= n_in of a witness before the first level: slot 0 becomes 1, an input its canonical residue
template <class F>
VMPC_HD void r1cs_solve_prepare(uint32_t *c, uint32_t i) {
    const F v = i ? r1cs_ld<F>(c, i) : f256_one<F>();
    r1cs_raw_st(c, i, v.v);
}
