// prod (x - j) over a leaf's consecutive points, multiplied out in LDS: shared by the leaves of t's product tree
// (csrc/bn256_qap_h.hip, k_qh_tleaf) and of the moment transform's subproduct tree (csrc/bn256_qap_mtree.hip).
#pragma once
#include "fr_bn.h"

#define QH_LEAF 128                 // factors (x - j) per leaf at most

// The product over j = j0 .. j1 (at most QH_LEAF factors) by the threads t <= QH_LEAF of a workgroup: thread i owns
// coefficient i, new_i = old_(i-1) - j old_i.  -> the half of sP that holds the j1 - j0 + 2 coefficients (zeros above).
__device__ __forceinline__ int qh_tleaf_product(uint32_t t, uint32_t j0, uint32_t j1, frbn (*sP)[QH_LEAF + 1]) {
    int cur = 0;
    if (t <= QH_LEAF) sP[0][t] = t == 0 ? frbn_one() : frbn_zero();
    __syncthreads();
    for (uint32_t j = j0; j <= j1; j++) {
        if (t <= QH_LEAF) {
            const frbn left = t ? sP[cur][t - 1] : frbn_zero();
            sP[cur ^ 1][t] = frbn_sub(left, frbn_mul_small(sP[cur][t], j));
        }
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}
