// One output of the share combination over a field of csrc/fr256.h whose products do not fit a 16-limb sum:
//     out = addend + sum_p weights[p] parts[p][i]
// for GF(n) of fr_bn.h.  n fills all 256 bits, so FOUR products of n - 1 already need 513 bits (3 (n-1)^2 has 512,
// 4 (n-1)^2 has 513) and the plain 512-bit sum of csrc/mpc_share.hip's GF(l) kernel (l^2 < 2^506, 64 products below 2^512) would
// drop a carry.  The products go into f256_acc, whose carry counters hold 2^32 products, and are reduced once.
// VMPC_HD: the kernel's per-element step, host-testable (tests/native/share_combine_host_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fr256.h"

// a >= the modulus of F ?
template <class F>
VMPC_HD bool f256_geq_m(const uint32_t a[8]) {
    const typename F::P p{};
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        if (a[i] > p.m[i]) return true;
        if (a[i] < p.m[i]) return false;
    }
    return true;
}

// the eight limbs of element i as they lie in memory (no reduction: the caller decides what a value >= m means)
VMPC_HD void f256_raw_ld(uint32_t w[8], const uint32_t *p, long long i) {
#ifdef __HIPCC__
    const uint4 *q = (const uint4 *)(p + 8 * i);
    const uint4 x = q[0], y = q[1];
    w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w, w[4] = y.x, w[5] = y.y, w[6] = y.z, w[7] = y.w;
#else
    for (int k = 0; k < 8; k++) w[k] = p[8 * i + k];
#endif
}

// false (and out untouched) when an element of parts is not a canonical residue.  weights: canonical, checked by the
// caller; addend: NULL or values as f256_load takes them (any 32 bytes where m passes 2^255).  Part p's element i
// lies at parts + 8 (p part_stride + i).
template <class F>
VMPC_HD bool share_combine_element(F &out, const uint32_t *parts, uint32_t parties, size_t part_stride, size_t i,
                                   const uint32_t (*weights)[8], const uint32_t *addend) {
    f256_acc s = f256_acc_zero();
    for (uint32_t p = 0; p < parties; p++) {
        uint32_t v[8];
        f256_raw_ld(v, parts, (long long)((size_t)p * part_stride + i));
        if (f256_geq_m<F>(v)) return false;
        f256_acc_mac(s, v, weights[p]);
    }
    out = f256_acc_reduce<F>(s);
    if (addend) {
        uint32_t v[8];
        f256_raw_ld(v, addend, (long long)i);
        out = f256_add(out, f256_load<F>(v));
    }
    return true;
}
