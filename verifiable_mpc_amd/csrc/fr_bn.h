// Scalar field GF(n), n = 65000549695646603732796438742359905742570406053903786389881062969044166799969 (the order
// of the BN-256 groups, verifiable_mpc/ac20/pairing.py:44-51), 8 x 32-bit limbs, canonical residues in memory
// (32 bytes LE) - the conventions of fr.h.  The arithmetic itself is csrc/fr256.h, shared with fr.h.
//
// Replaces the MPyC GF(n) arithmetic of the knowledge-of-exponent pivot:
//   c_poly = c_poly_lhs * c_poly_rhs         verifiable_mpc/ac20/knowledge_of_exponent.py:121-123
//                                            (verifiable_mpc/tools/qap_creator.py Poly.__mul__, O(n^2))
//   g1_base ** z, g2_base ** z  (2n times)   knowledge_of_exponent.py:61-66: the exponents g_exp z^(i+1)
//
// n fills all 256 bits (2^255 < n < 2^256), which is where this differs from fr.h: a sum of two residues carries out
// of 256 bits and every 256-bit value is below 2n (ONE conditional subtraction canonicalises a load).
// VMPC_HD: host-testable (tests/native/frbn_host_test.cpp).
#pragma once
#include <stdint.h>
#include "fr256.h"

#define VMPC_FRBN_N                                                                            \
    { 0x57ac7261u, 0x1a2ef45bu, 0xf82b3924u, 0x2e8d8e12u, 0x6184dc21u, 0xaa6fecb8u,            \
      0x4aa387f9u, 0x8fb501e3u }
// mu = floor(2^512 / n), 9 limbs (257 bits)
#define VMPC_FRBN_MU                                                                           \
    { 0x9986fdabu, 0xd8c1a724u, 0xaf8baf78u, 0x13a80503u, 0x64874e35u, 0x1e2c1bc9u,            \
      0x10f7561fu, 0xc809f0fau, 0x00000001u }

struct frbn_params {
    uint32_t m[8] = VMPC_FRBN_N;
    uint32_t mu[9] = VMPC_FRBN_MU;
    static constexpr int bits = 256;
};
typedef f256<frbn_params> frbn;

VMPC_HD frbn frbn_zero() { return f256_zero<frbn>(); }
VMPC_HD frbn frbn_one() { return f256_one<frbn>(); }
VMPC_HD frbn frbn_cond_sub_n(const frbn &a, uint32_t a8) { return f256_cond_sub(a, a8); }
VMPC_HD frbn frbn_load(const uint32_t *p) { return f256_load<frbn>(p); }  // any 32-byte value -> its residue
VMPC_HD void frbn_store(uint32_t *p, const frbn &a) { f256_store(p, a); }
VMPC_HD frbn frbn_add(const frbn &a, const frbn &b) { return f256_add(a, b); }
VMPC_HD frbn frbn_sub(const frbn &a, const frbn &b) { return f256_sub(a, b); }
VMPC_HD frbn frbn_reduce512(const uint32_t x[16]) { return f256_reduce512<frbn>(x); }
VMPC_HD frbn frbn_mul(const frbn &a, const frbn &b) { return f256_mul(a, b); }
VMPC_HD frbn frbn_inv(const frbn &a) { return f256_inv(a); }

// the wide accumulator of the polynomial product
typedef f256_acc frbn_acc;
VMPC_HD frbn_acc frbn_acc_zero() { return f256_acc_zero(); }
VMPC_HD void frbn_acc_mac(frbn_acc &s, const uint32_t a[8], const uint32_t b[8]) { f256_acc_mac(s, a, b); }
VMPC_HD frbn frbn_acc_reduce(const frbn_acc &s) { return f256_acc_reduce<frbn>(s); }

// ---- multiplication by a small integer and the lazy sum of the moment transform (csrc/bn256_qap_h.hip) --------------
// The prover's h needs the power sums sum_j u_j j^k: the running value u_j j^k advances by a product with the integer
// j <= d < 2^21, eight limb products and a one-limb quotient instead of 64 and a Barrett reduction.
#define VMPC_FRBN_SMALL_BITS 21
#define VMPC_FRBN_M287 0xe404f87du   // floor(2^287 / n)

// a * j mod n for ANY 256-bit a and j < 2^21, canonical.  x = a j < 2^277; the quotient estimate
// q = floor((x >> 192) M287 / 2^95) is floor(x / n) or one less (the two truncations lose less than 2^-9), so
// x - q n < 2n and one conditional subtraction finishes.
VMPC_HD frbn frbn_mul_small(const frbn &a, uint32_t j) {
    const uint32_t N[8] = VMPC_FRBN_N;
    uint32_t x[9];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] * j;
        x[i] = (uint32_t)c;
        c >>= 32;
    }
    x[8] = (uint32_t)c;
    const uint64_t p0 = (uint64_t)x[6] * VMPC_FRBN_M287;
    const uint64_t p1 = (uint64_t)x[7] * VMPC_FRBN_M287 + (p0 >> 32);
    const uint64_t p2 = (uint64_t)x[8] * VMPC_FRBN_M287 + (p1 >> 32);   // bits 64.. of (x >> 192) M287
    const uint32_t q = (uint32_t)(p2 >> 31);                            // < 2^23
    frbn r;
    uint64_t m = 0;
    int64_t b = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        m += (uint64_t)q * N[i];
        b += (int64_t)x[i] - (int64_t)(uint32_t)m;
        r.v[i] = (uint32_t)b;
        b >>= 32;
        m >>= 32;
    }
    b += (int64_t)x[8] - (int64_t)(uint32_t)m;
    return frbn_cond_sub_n(r, (uint32_t)b);
}

// An unreduced sum of 256-bit values in nine limbs (< 2^288: 2^32 summands).  The moment transform adds a lane's few
// values with a carry chain, cuts the sum (< 2^260) into ten 26-bit pieces that a wave adds piece by piece in 32-bit
// registers (64 lanes: 6 more bits), joins the piece sums again and keeps adding in nine limbs; ONE reduction at the end.
struct frbn_wide {
    uint32_t v[9];
};

VMPC_HD frbn_wide frbn_wide_zero() {
    frbn_wide w;
#pragma unroll
    for (int i = 0; i < 9; i++) w.v[i] = 0;
    return w;
}

VMPC_HD void frbn_wide_add_fr(frbn_wide &w, const frbn &a) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)w.v[i] + a.v[i];
        w.v[i] = (uint32_t)c;
        c >>= 32;
    }
    w.v[8] += (uint32_t)c;
}

VMPC_HD void frbn_wide_add(frbn_wide &w, const frbn_wide &o) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c += (uint64_t)w.v[i] + o.v[i];
        w.v[i] = (uint32_t)c;
        c >>= 32;
    }
}

// p[i] = bits 26 i .. 26 i + 25 of w, for w < 2^260
VMPC_HD void frbn_wide_split26(const frbn_wide &w, uint32_t p[10]) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const int bit = 26 * i, l = bit >> 5, s = bit & 31;
        uint32_t x = w.v[l] >> s;
        if (s > 6 && l + 1 < 9) x |= w.v[l + 1] << (32 - s);
        p[i] = x & 0x3ffffffu;
    }
}

// sum_i p[i] 2^(26 i) for ANY 32-bit p[i] (< 2^266)
VMPC_HD frbn_wide frbn_wide_join26(const uint32_t p[10]) {
    uint64_t t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const int bit = 26 * i, l = bit >> 5, s = bit & 31;
        const uint64_t x = (uint64_t)p[i] << s;
        t[l] += (uint32_t)x;
        t[l + 1] += x >> 32;   // l + 1 <= 8: piece 9 starts at bit 234, limb 7
    }
    frbn_wide w;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c += t[i];
        w.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return w;
}

VMPC_HD frbn frbn_wide_reduce(const frbn_wide &w) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = i < 9 ? w.v[i] : 0u;
    return frbn_reduce512(t);
}
