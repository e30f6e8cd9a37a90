// Arithmetic of the multi-prime NTT over the INTEGERS (csrc/bn256_ntt.hip): GF(n) of BN-256 has no NTT of useful length
// (n - 1 = 2^5 * odd, csrc/bn256_koe.hip), the integers do.  A product of two coefficient vectors of ANY 32-byte values is
// convolved modulo NTT31_NP = 18 primes p = c 2^22 + 1 < 2^31 (csrc/ntt31_consts.h), the exact integer coefficient
// (at most 2^20 (2^256 - 1)^2 < 2^532 < M = prod p_i, 551 bits) is rebuilt by Garner's mixed-radix digits and reduced
// mod n by Horner over the digits: the canonical residue the schoolbook kernel writes, bit for bit.
//
//   per prime    Montgomery products with R = 2^32: one 32 x 32 -> 64 product, one low 32-bit product, one
//                multiply-add.  Values are LAZY, in [0, 2p) (p < 2^31: they fit 32 bits); ntt31_mul wants a b < p R,
//                which holds when one factor is canonical (< p) and the other lazy.
//   reduction    a 256-bit little-endian scalar mod p by Horner over its 8 limbs, result in Montgomery form.
//   butterflies  ntt31_dif (decimation in frequency, forward, output bit-reversed) and ntt31_dit (decimation in time,
//                inverse, from that order): no permutation pass.
//   rebuilding   ntt31_crt: the scale L^-1 of the inverse transform is folded in HERE (one product per prime, which also
//                takes the residue out of Montgomery form), then ntt31_garner and ntt31_horner.
//
// ntt31_horner multiplies by p_i < 2^31 with frbn_mul_small, whose header states j < 2^21: for a < 2^256 and j < 2^31,
// x = a j < 2^287, the quotient fits 32 bits and the estimate loses less than x / 2^287 + 2^-63 < 1, so it is still the
// quotient or one less and one conditional subtraction finishes (tests/native/ntt31_host_test.cpp holds it against
// unsigned __int128 limb arithmetic).
// Nothing above belongs to GF(n) but that last Horner reduction: ntt31_horner_in / ntt31_crt_in take the field as a
// template parameter, and GF(l) of Ed25519 (csrc/fr.h, fr_mul_small with its own bound; the Protocol 8 extension of
// csrc/circuit_sat.hip, coefficients at most 2^20 (l - 1)^2 < 2^526) is the second instantiation
// (tests/native/ntt31_fr_host_test.cpp).
// VMPC_HD, plain C++: host-testable (tests/native/ntt31_host_test.cpp).
#pragma once
#include <stdint.h>

#include "fr.h"
#include "fr_bn.h"
#include "ntt31_consts.h"

struct ntt31_prime {
    uint32_t p, ninv, r1, r2;      // the prime, -p^-1 mod 2^32, R mod p, R^2 mod p
};

// prime i (any index: the tables are constant data, a constant index folds to literals)
VMPC_HD ntt31_prime ntt31_prime_of(int i) {
    const uint32_t P[NTT31_NP] = NTT31_PRIMES, NI[NTT31_NP] = NTT31_NINV, R1[NTT31_NP] = NTT31_R1,
                   R2[NTT31_NP] = NTT31_R2;
    ntt31_prime q;
    q.p = P[i];
    q.ninv = NI[i];
    q.r1 = R1[i];
    q.r2 = R2[i];
    return q;
}

// a b / R mod p in [0, 2p), for a b < p R
VMPC_HD uint32_t ntt31_mul(uint32_t a, uint32_t b, const ntt31_prime &q) {
    const uint64_t t = (uint64_t)a * b;
    const uint32_t m = (uint32_t)t * q.ninv;
    return (uint32_t)((t + (uint64_t)m * q.p) >> 32);
}

// [0, 2p) -> [0, p)
VMPC_HD uint32_t ntt31_csub(uint32_t a, uint32_t p) { return a >= p ? a - p : a; }

// a + b and a - b for lazy a, b, lazy again (no 32-bit wrap: 2p - b is formed first)
VMPC_HD uint32_t ntt31_add(uint32_t a, uint32_t b, uint32_t p) {
    const uint32_t c = 2 * p - b;
    return a >= c ? a - c : a + b;
}
VMPC_HD uint32_t ntt31_sub(uint32_t a, uint32_t b, uint32_t p) { return a >= b ? a - b : a - b + 2 * p; }

// base^e for a Montgomery-form base, canonical Montgomery form
VMPC_HD uint32_t ntt31_pow(uint32_t base, uint32_t e, const ntt31_prime &q) {
    uint32_t r = q.r1, s = ntt31_csub(base, q.p);
    for (; e; e >>= 1) {
        if (e & 1) r = ntt31_csub(ntt31_mul(r, s, q), q.p);
        s = ntt31_csub(ntt31_mul(s, s, q), q.p);
    }
    return r;
}

// the 256-bit value x[0..7] (little endian, ANY value) mod p, canonical Montgomery form
VMPC_HD uint32_t ntt31_reduce256(const uint32_t x[8], const ntt31_prime &q) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        uint32_t l = x[i];                                  // < 2^32 < 4p (p > 2^30)
        if (l >= 2 * q.p) l -= 2 * q.p;
        l = ntt31_csub(l, q.p);
        s = ntt31_csub(ntt31_mul(s, q.r2, q), q.p) + l;     // s 2^32 + l, lazy
    }
    return ntt31_csub(ntt31_mul(s, q.r2, q), q.p);
}

// forward butterfly: (a, b) -> (a + b, (a - b) w); a, b lazy, w canonical
VMPC_HD void ntt31_dif(uint32_t &a, uint32_t &b, uint32_t w, const ntt31_prime &q) {
    const uint32_t s = ntt31_add(a, b, q.p), d = ntt31_sub(a, b, q.p);
    a = s;
    b = ntt31_mul(d, w, q);
}

// inverse butterfly: (a, b) -> (a + b w, a - b w); a, b lazy, w canonical (the inverse twiddle)
VMPC_HD void ntt31_dit(uint32_t &a, uint32_t &b, uint32_t w, const ntt31_prime &q) {
    const uint32_t t = ntt31_mul(b, w, q);
    b = ntt31_sub(a, t, q.p);
    a = ntt31_add(a, t, q.p);
}

// L^-1 mod p for L = 2^log_l <= 2^22, plain (not Montgomery): 2^k divides p - 1, so 2^-k = p - (p - 1) / 2^k
VMPC_HD uint32_t ntt31_inv_pow2(int log_l, uint32_t p) { return p - ((p - 1) >> log_l); }

// mixed-radix digits of the x in [0, M) with x = r[i] mod p_i (r canonical, plain): x = d0 + p0 (d1 + p1 (d2 + ...))
VMPC_HD void ntt31_garner(const uint32_t r[NTT31_NP], uint32_t d[NTT31_NP]) {
    const uint32_t G[NTT31_NP][NTT31_NP] = NTT31_GARNER;
#pragma unroll
    for (int i = 0; i < NTT31_NP; i++) {
        const ntt31_prime q = ntt31_prime_of(i);
        uint32_t t = r[i];
#pragma unroll
        for (int j = 0; j < i; j++) {
            const uint32_t dj = ntt31_csub(d[j], q.p);      // d_j < p_j < 2^31 < 2 p_i
            const uint32_t diff = t >= dj ? t - dj : t - dj + q.p;
            t = ntt31_csub(ntt31_mul(diff, G[i][j], q), q.p);
        }
        d[i] = t;
    }
}

// acc p mod the field's modulus, canonical, for a 31-bit p: frbn_mul_small (csrc/fr_bn.h) takes ANY 256-bit acc,
// fr_mul_small (csrc/fr.h) a canonical one - which acc is at every step of ntt31_horner_in: it starts as a digit < 2^31
// and every step ends in an f256_add of canonical values.
VMPC_HD frbn ntt31_mul_small(const frbn &a, uint32_t p) { return frbn_mul_small(a, p); }
VMPC_HD fr ntt31_mul_small(const fr &a, uint32_t p) { return fr_mul_small(a, p); }

// the value of the digits mod the modulus of F (frbn: n, fr: l), from the top digit: acc = acc p_i + d_i
template <class F>
VMPC_HD F ntt31_horner_in(const uint32_t d[NTT31_NP]) {
    const uint32_t P[NTT31_NP] = NTT31_PRIMES;
    F acc = f256_zero<F>();
    acc.v[0] = d[NTT31_NP - 1];
#pragma unroll
    for (int i = NTT31_NP - 2; i >= 0; i--) {
        F di = f256_zero<F>();
        di.v[0] = d[i];
        acc = f256_add(ntt31_mul_small(acc, P[i]), di);
    }
    return acc;
}

// res[i]: the inverse transform's output mod p_i (Montgomery form, lazy, still times L); linv[i] = ntt31_inv_pow2
template <class F>
VMPC_HD F ntt31_crt_in(const uint32_t res[NTT31_NP], const uint32_t linv[NTT31_NP]) {
    uint32_t r[NTT31_NP], d[NTT31_NP];
#pragma unroll
    for (int i = 0; i < NTT31_NP; i++) {
        const ntt31_prime q = ntt31_prime_of(i);
        r[i] = ntt31_csub(ntt31_mul(res[i], linv[i], q), q.p);
    }
    ntt31_garner(r, d);
    return ntt31_horner_in<F>(d);
}

// the GF(n) instantiations under the names they have always had
VMPC_HD frbn ntt31_horner(const uint32_t d[NTT31_NP]) { return ntt31_horner_in<frbn>(d); }
VMPC_HD frbn ntt31_crt(const uint32_t res[NTT31_NP], const uint32_t linv[NTT31_NP]) {
    return ntt31_crt_in<frbn>(res, linv);
}
