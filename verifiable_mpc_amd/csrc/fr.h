// Scalar field GF(l), l = 2^252 + 27742317777372353535851937790883648493 (Ed25519 group
// order), 8 x 32-bit limbs, canonical residues in memory (32 bytes LE).  The arithmetic itself is csrc/fr256.h,
// shared with fr_bn.h.
//
// Replaces the MPyC GF(l) element arithmetic of the scalar side of Protocol 4/5:
//   z' = z_l + c*z_r, L' = c*L_l + L_r   verifiable_mpc/ac20/compressed_pivot.py:70-76
//   z  = c0*x + r, L~ = (L||0)*c1        compressed_pivot.py:134,141
//   L(z) = sum coeffs[i]*values[i]       verifiable_mpc/ac20/pivot.py:84-92
#pragma once
#include <stdint.h>
#include "fr256.h"

#define VMPC_FR_L                                                                              \
    { 0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0x00000000u, 0x00000000u,            \
      0x00000000u, 0x10000000u }
// mu = floor(2^512 / l), 9 limbs
#define VMPC_FR_MU                                                                             \
    { 0x0a2c131bu, 0xed9ce5a3u, 0x086329a7u, 0x2106215du, 0xffffffebu, 0xffffffffu,            \
      0xffffffffu, 0xffffffffu, 0x0000000fu }

// the arithmetic is csrc/fr256.h; l < 2^253, so sums stay within 256 bits and fr_load is a plain copy
struct fr_params {
    uint32_t m[8] = VMPC_FR_L;
    uint32_t mu[9] = VMPC_FR_MU;
    static constexpr int bits = 253;
};
typedef f256<fr_params> fr;

VMPC_HD fr fr_zero() { return f256_zero<fr>(); }
VMPC_HD fr fr_load(const uint32_t *p) { return f256_load<fr>(p); }
VMPC_HD void fr_store(uint32_t *p, const fr &a) { f256_store(p, a); }
VMPC_HD fr fr_cond_sub_l(const fr &a) { return f256_cond_sub(a, 0); }  // r = a - l if a >= l (a < 2l)
VMPC_HD fr fr_add(const fr &a, const fr &b) { return f256_add(a, b); }
VMPC_HD fr fr_sub(const fr &a, const fr &b) { return f256_sub(a, b); }
VMPC_HD fr fr_neg(const fr &a) { return f256_neg(a); }
VMPC_HD fr fr_reduce512(const uint32_t x[16]) { return f256_reduce512<fr>(x); }
VMPC_HD void fr_mul_wide(uint32_t t[16], const fr &a, const fr &b) { f256_mul_wide(t, a, b); }
VMPC_HD fr fr_mul(const fr &a, const fr &b) { return f256_mul(a, b); }
VMPC_HD bool fr_is_zero(const fr &a) { return f256_equal(a, f256_zero<fr>()); }

// a >= l ?
VMPC_HD bool fr_geq_l(const uint32_t a[8]) {
    const uint32_t L[8] = VMPC_FR_L;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        if (a[i] > L[i]) return true;
        if (a[i] < L[i]) return false;
    }
    return true;
}

VMPC_HD bool fr_is_canonical(const fr &a) { return !fr_geq_l(a.v); }

// ---- multiplication by a small integer: the Horner step of the multi-prime NTT's reconstruction (csrc/ntt31.h) -------
#define VMPC_FR_SMALL_BITS 31
#define VMPC_FR_M284 0xffffffffu   // floor(2^284 / l) = 2^32 - 1 (l = 2^252 + d, d < 2^125: 2^284 / l = 2^32 - d 2^-220 + ..)

// a * j mod l for a CANONICAL a (< l) and j < 2^31, canonical: the counterpart of frbn_mul_small (csrc/fr_bn.h).
// x = a j < 2^31 l < 2^284, so floor(x / l) < 2^31.  With X = floor(x / 2^192) < 2^92 and M = VMPC_FR_M284 the estimate
// q = floor(X M / 2^92) never exceeds x / l (both factors are rounded down) and
//     X M / 2^92 > (x / 2^192 - 1) (2^284 / l - 1) / 2^92 > x / l - x / 2^284 - 2^192 / l > x / l - (1/2 + 2^-128) - 2^-60,
// because x < 2^31 l = 2^284 (l / 2^253) and l / 2^253 < 1/2 + 2^-128.  The estimate loses less than 1: q is
// floor(x / l) or one less, x - q l < 2 l < 2^254 fits eight limbs and one conditional subtraction finishes.
// (X M < 2^124: the three partial products below carry into 64 bits without overflow; p2 = floor(X M / 2^64) < 2^60.)
VMPC_HD fr fr_mul_small(const fr &a, uint32_t j) {
    const uint32_t L[8] = VMPC_FR_L;
    uint32_t x[9];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] * j;
        x[i] = (uint32_t)c;
        c >>= 32;
    }
    x[8] = (uint32_t)c;
    const uint64_t p0 = (uint64_t)x[6] * VMPC_FR_M284;
    const uint64_t p1 = (uint64_t)x[7] * VMPC_FR_M284 + (p0 >> 32);
    const uint64_t p2 = (uint64_t)x[8] * VMPC_FR_M284 + (p1 >> 32);     // bits 64.. of (x >> 192) M284
    const uint32_t q = (uint32_t)(p2 >> 28);                            // < 2^31
    fr r;
    uint64_t m = 0;
    int64_t b = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        m += (uint64_t)q * L[i];
        b += (int64_t)x[i] - (int64_t)(uint32_t)m;
        r.v[i] = (uint32_t)b;
        b >>= 32;
        m >>= 32;
    }
    return fr_cond_sub_l(r);      // the ninth limb of x - q l is zero (< 2^254)
}

// reduce an arbitrary 256-bit value (e.g. a SHA-256 digest read as LE integer)
VMPC_HD fr fr_from_u256(const uint32_t a[8]) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        t[i] = a[i];
        t[i + 8] = 0;
    }
    return fr_reduce512(t);
}

// signed residue split used by the reference's `_int` (pivot.py:119-128) on a signed
// GF(l): returns true and |a| = l - a when a > l/2  [mpyc-recall: GF() is signed]
VMPC_HD bool fr_signed_abs(const fr &a, fr &mag) {
    // l/2 = (l-1)/2 ; a > (l-1)/2  <=>  2a > l - 1  <=> 2a >= l
    uint32_t d[8];
    uint32_t top = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        d[i] = (a.v[i] << 1) | top;
        top = a.v[i] >> 31;
    }
    bool neg = fr_geq_l(d);  // a < 2^253 so no overflow
    fr n = fr_neg(a);
    mag = neg ? n : a;
    return neg;
}
