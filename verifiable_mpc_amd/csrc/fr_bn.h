// Scalar field GF(n), n = 65000549695646603732796438742359905742570406053903786389881062969044166799969 (the order
// of the BN-256 groups, verifiable_mpc/ac20/pairing.py:44-51), 8 x 32-bit limbs, canonical residues in memory
// (32 bytes LE) - the conventions of fr.h.
//
// Replaces the MPyC GF(n) arithmetic of the knowledge-of-exponent pivot:
//   c_poly = c_poly_lhs * c_poly_rhs         verifiable_mpc/ac20/knowledge_of_exponent.py:121-123
//                                            (verifiable_mpc/tools/qap_creator.py Poly.__mul__, O(n^2))
//   g1_base ** z, g2_base ** z  (2n times)   knowledge_of_exponent.py:61-66: the exponents g_exp z^(i+1)
//
// n fills all 256 bits (2^255 < n < 2^256), which is where this differs from fr.h: a sum of two residues carries out
// of 256 bits, every 256-bit value is below 2n (ONE conditional subtraction canonicalises a load), and a sum of m
// 512-bit products needs 512 + log2(m) bits (frbn_acc: 16 limbs and eight 64-bit row carries, good for 2^32 products).
// VMPC_HD: host-testable (tests/native/frbn_host_test.cpp).
#pragma once
#include <stdint.h>
#include "fe25519.h"  // VMPC_HD

struct frbn {
    uint32_t v[8];
};

#define VMPC_FRBN_N                                                                            \
    { 0x57ac7261u, 0x1a2ef45bu, 0xf82b3924u, 0x2e8d8e12u, 0x6184dc21u, 0xaa6fecb8u,            \
      0x4aa387f9u, 0x8fb501e3u }
// mu = floor(2^512 / n), 9 limbs (257 bits)
#define VMPC_FRBN_MU                                                                           \
    { 0x9986fdabu, 0xd8c1a724u, 0xaf8baf78u, 0x13a80503u, 0x64874e35u, 0x1e2c1bc9u,            \
      0x10f7561fu, 0xc809f0fau, 0x00000001u }

VMPC_HD frbn frbn_zero() {
    frbn r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
}

VMPC_HD frbn frbn_one() {
    frbn r = frbn_zero();
    r.v[0] = 1;
    return r;
}

// r = a - n if a >= n, for a nine-limb a < 2n (a8: the ninth limb, 0 or 1)
VMPC_HD frbn frbn_cond_sub_n(const frbn &a, uint32_t a8) {
    const uint32_t N[8] = VMPC_FRBN_N;
    frbn s;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (int64_t)a.v[i] - (int64_t)N[i];
        s.v[i] = (uint32_t)c;
        c >>= 32;
    }
    c += (int64_t)a8;
    const uint32_t m = (uint32_t)c;  // all ones if borrow (a < n): keep a
    frbn r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (a.v[i] & m) | (s.v[i] & ~m);
    return r;
}

// any 32-byte value -> its canonical residue (2^256 < 2n: one subtraction)
VMPC_HD frbn frbn_load(const uint32_t *p) {
    frbn r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return frbn_cond_sub_n(r, 0);
}

VMPC_HD void frbn_store(uint32_t *p, const frbn &a) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}

VMPC_HD frbn frbn_add(const frbn &a, const frbn &b) {
    frbn r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] + b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return frbn_cond_sub_n(r, (uint32_t)c);  // a, b < n: the sum is below 2n but may pass 2^256
}

VMPC_HD frbn frbn_sub(const frbn &a, const frbn &b) {
    const uint32_t N[8] = VMPC_FRBN_N;
    frbn r;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (int64_t)a.v[i] - (int64_t)b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    const uint32_t m = (uint32_t)c;  // borrow: add n back
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        d += (uint64_t)r.v[i] + (N[i] & m);
        r.v[i] = (uint32_t)d;
        d >>= 32;
    }
    return r;
}

// Barrett reduction of a 512-bit value (HAC 14.42 with b = 2^32, k = 8); the quotient estimate is at most two short,
// so r < 3n < 2^258 lives in nine limbs
VMPC_HD frbn frbn_reduce512(const uint32_t x[16]) {
    const uint32_t N[8] = VMPC_FRBN_N;
    const uint32_t MU[9] = VMPC_FRBN_MU;
    // q1 = x >> 224 (x[7..15]); q2 = q1 * mu (18 limbs); q3 = q2 >> 288 (q2[9..17])
    uint32_t q2[18];
#pragma unroll
    for (int i = 0; i < 18; i++) q2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            c += (uint64_t)x[7 + i] * MU[j] + q2[i + j];
            q2[i + j] = (uint32_t)c;
            c >>= 32;
        }
        q2[i + 9] = (uint32_t)c;
    }
    // r2 = (q3 * n) mod 2^288
    uint32_t r2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) r2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (i + j < 9) {
                c += (uint64_t)q2[9 + i] * N[j] + r2[i + j];
                r2[i + j] = (uint32_t)c;
                c >>= 32;
            }
        }
        if (i + 8 < 9) r2[i + 8] = (uint32_t)c;
    }
    // r = (x mod 2^288) - r2 (mod 2^288)
    uint32_t r[9];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c += (int64_t)x[i] - (int64_t)r2[i];
        r[i] = (uint32_t)c;
        c >>= 32;
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        uint32_t s[9];
        int64_t b = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            b += (int64_t)r[i] - (int64_t)(i < 8 ? N[i] : 0u);
            s[i] = (uint32_t)b;
            b >>= 32;
        }
        const uint32_t m = (uint32_t)b;  // borrow: keep r
#pragma unroll
        for (int i = 0; i < 9; i++) r[i] = (r[i] & m) | (s[i] & ~m);
    }
    frbn out;
#pragma unroll
    for (int i = 0; i < 8; i++) out.v[i] = r[i];
    return out;
}

VMPC_HD frbn frbn_mul(const frbn &a, const frbn &b) {
    uint32_t t[16];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)a.v[0] * b.v[j];
        t[j] = (uint32_t)c;
        c >>= 32;
    }
    t[8] = (uint32_t)c;
#pragma unroll
    for (int i = 1; i < 8; i++) {
        c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a.v[i] * b.v[j] + t[i + j];
            t[i + j] = (uint32_t)c;
            c >>= 32;
        }
        t[i + 8] = (uint32_t)c;
    }
    return frbn_reduce512(t);
}

// a^(n-2) = 1/a for a != 0 (Fermat; 0 -> 0): 255 squarings and one product per set bit of n - 2, left to right
VMPC_HD frbn frbn_inv(const frbn &a) {
    uint32_t e[8] = VMPC_FRBN_N;
    e[0] -= 2;  // n is odd and its low limb exceeds 2: no borrow
    frbn r = frbn_one();
    for (int i = 255; i >= 0; i--) {
        r = frbn_mul(r, r);
        if ((e[i >> 5] >> (i & 31)) & 1u) r = frbn_mul(r, a);
    }
    return r;
}

// ---- the wide accumulator of the polynomial product ----------------------------------------------------------------
// value = sum_k lo[k] 2^(32 k) + sum_i hi[i] 2^(32 (i + 8)).  frbn_acc_mac adds one unreduced 8 x 8-limb product: row i
// of the schoolbook product runs its carry chain through lo[i .. i+7] and drops the carry that leaves the row into
// hi[i], a 64-bit counter, instead of rippling it to the top - so no limb above the row is touched and nothing is
// lost: after m products every hi[i] is below m 2^32, i.e. m < 2^32 products never overflow.
struct frbn_acc {
    uint32_t lo[16];
    uint64_t hi[8];
};

VMPC_HD frbn_acc frbn_acc_zero() {
    frbn_acc s;
#pragma unroll
    for (int i = 0; i < 16; i++) s.lo[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s.hi[i] = 0;
    return s;
}

VMPC_HD void frbn_acc_mac(frbn_acc &s, const uint32_t a[8], const uint32_t b[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a[i] * b[j] + s.lo[i + j];  // <= (2^32-1)^2 + 2 (2^32-1) = 2^64 - 1
            s.lo[i + j] = (uint32_t)c;
            c >>= 32;
        }
        s.hi[i] += c;
    }
}

// the accumulator's value mod n.  It is below 2^545 (hi[7] < 2^64 sits at bit 480): written as 18 limbs w, the top 16
// are reduced first and each lower limb is then shifted in (r 2^32 + limb < 2^288 is a valid Barrett input).
VMPC_HD frbn frbn_acc_reduce(const frbn_acc &s) {
    uint32_t w[18];
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < 18; k++) {
        // limb k receives lo[k], the low word of hi[k-8] and the high word of hi[k-9]
        if (k < 16) c += s.lo[k];
        if (k >= 8 && k < 16) c += (uint32_t)s.hi[k - 8];
        if (k >= 9 && k < 17) c += (uint32_t)(s.hi[k - 9] >> 32);
        w[k] = (uint32_t)c;
        c >>= 32;
    }
    frbn r = frbn_reduce512(w + 2);
#pragma unroll
    for (int k = 1; k >= 0; k--) {
        uint32_t t[16];
        t[0] = w[k];
#pragma unroll
        for (int i = 0; i < 8; i++) t[i + 1] = r.v[i];
#pragma unroll
        for (int i = 9; i < 16; i++) t[i] = 0;
        r = frbn_reduce512(t);
    }
    return r;
}

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
