// Geometry of the moment transform's subproduct tree (csrc/bn256_qap_mtree.hip): plain C++, host
// and device (tests/native/qap_mtree_plan_host_test.cpp), as fold_jump_plan.h is for the fold jump.
//
// The tree stands over the points 1 .. d', d' = s 2^L >= d: L is the smallest number of levels with
// s = ceil(d / 2^L) <= QAP_MTREE_S_MAX.  Points beyond d carry u_j = 0 and change N and T by the same factor, so the
// series R / D is the one of d points; the waste d' - d is below 2^L, and s > S_MAX / 2 whenever L > 0 (one level
// fewer would have had ceil(d / 2^(L-1)) > S_MAX, and s >= that / 2).
//
//   level l (0 = leaves .. L = root)   2^(L-l) nodes T = prod (x - j) over s 2^l consecutive points, each with ALL its
//                                      s 2^l + 1 coefficients (the leading 1 included), one after the other:
//                                      d' + 2^(L-l) scalars from lvl_off[l]
//   dinv_off                           n_max scalars: D^-1 mod z^n_max, D(z) = z^d' T_root(1 / z)
//   tmp_off                            2 n_max scalars the build alone uses (D and the Newton step's 2 - D g)
//   total                              (L + 1) d' + 2^(L+1) - 1 + 3 n_max scalars
//
// Caps (include/vmpc.h): d + 1 <= 2^20 and n_max <= 2^20.  Then L <= 13 (ceil((2^20 - 1) / 2^13) = 128), and
// d' = s 2^L <= 128 x 2^13 = 2^20.  Every product the tree asks of the NTT (csrc/bn256_ntt.hip) stays within the
// transform's 2^21 points: a level's N_left T_right + N_right T_left has 2 s 2^l <= d' <= 2^20 coefficients, T_left
// T_right one more (<= 2^20 + 1), a Newton step and the final product at most 2 n_max - 1 < 2^21.
//
// The coefficient bound: the operands of every product are canonical residues (< n < 2^256).  An integer coefficient of
// a parent's N_left T_right + N_right T_left is a sum of at most 2 s 2^l <= d' products, below d' n^2 < 2^(512 +
// ceil(log2 d')) <= 2^532 - the bound csrc/ntt31.h states for ONE product at its cap, below the product of its 18 primes
// (551 bits).  So the two products of a parent are added in the residue domain, before the one inverse transform.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define QAP_MTREE_S_MAX 128       // points per leaf at most (= QH_LEAF: the leaf kernel of t's coefficients, shared)
#define QAP_MTREE_MAX_LEVELS 14   // levels 0 .. L, L <= 13 at the cap

struct qap_mtree_plan {
    uint32_t s, L;                           // points per leaf, levels above the leaves
    size_t dp;                               // d' = s 2^L
    size_t lvl_off[QAP_MTREE_MAX_LEVELS];    // scalars
    size_t dinv_off, tmp_off, total;         // scalars
};

// d >= 1, d <= 2^20
inline qap_mtree_plan qap_mtree_plan_of(size_t d, size_t n_max) {
    qap_mtree_plan p;
    p.L = 0;
    while ((d + ((size_t)1 << p.L) - 1) >> p.L > QAP_MTREE_S_MAX) p.L++;
    p.s = (uint32_t)((d + ((size_t)1 << p.L) - 1) >> p.L);
    p.dp = (size_t)p.s << p.L;
    size_t off = 0;
    for (uint32_t l = 0; l < QAP_MTREE_MAX_LEVELS; l++) {
        p.lvl_off[l] = off;
        if (l <= p.L) off += p.dp + ((size_t)1 << (p.L - l));
    }
    p.dinv_off = off;
    p.tmp_off = off + n_max;
    p.total = off + 3 * n_max;
    return p;
}

// the caller's scratch, in scalars: two buffers of d' per vector (always counted for two vectors) and witness
inline size_t qap_mtree_scratch_scalars(size_t d, size_t n_wit) { return 4 * qap_mtree_plan_of(d, 1).dp * n_wit; }

// an integer coefficient the tree asks the NTT to rebuild is below 2^(this): 512 + ceil(log2 d')
inline int qap_mtree_coeff_bits(size_t d) {
    const size_t dp = qap_mtree_plan_of(d, 1).dp;
    int lg = 0;
    while (((size_t)1 << lg) < dp) lg++;
    return 512 + lg;
}
