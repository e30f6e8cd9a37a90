// CPU check of the GF(l) half of csrc/ntt31.h (the reconstruction of the Protocol 8 extension's NTT route,
// csrc/circuit_sat.hip) against unsigned __int128 and a small limb-array big-number type of this file's own:
// fr_mul_small (csrc/fr.h) and ntt31_horner_in<fr> / ntt31_crt_in<fr>, and that the GF(n) instantiation still returns
// what long arithmetic mod n gives on the same tuples.  Built by tests/test_native_ntt31_fr_host.py with g++ under
// AddressSanitizer and UndefinedBehaviorSanitizer and run directly; prints one "<name> ok" line per group.
// l = 2^252 + 27742317777372353535851937790883648493, restated here limb by limb (not taken from csrc/fr.h).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../verifiable_mpc_amd/csrc/ntt31.h"

typedef unsigned __int128 u128;

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

// ---- big numbers: 24 limbs (768 bits), little endian ---------------------------------------------------------------
#define BL 24
struct big {
    uint32_t v[BL];
};
static big big_zero() {
    big r;
    memset(r.v, 0, sizeof r.v);
    return r;
}
static int big_cmp(const big &a, const big &b) {
    for (int i = BL - 1; i >= 0; i--)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i] ? -1 : 1;
    return 0;
}
static big big_sub(const big &a, const big &b) {
    CHECK(big_cmp(a, b) >= 0);
    big r;
    int64_t c = 0;
    for (int i = 0; i < BL; i++) {
        c += (int64_t)a.v[i] - (int64_t)b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
static big big_mul_small_add(const big &a, uint32_t m, uint32_t add) {
    big r;
    uint64_t c = add;
    for (int i = 0; i < BL; i++) {
        c += (uint64_t)a.v[i] * m;
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    CHECK(c == 0);
    return r;
}
// schoolbook product through unsigned __int128 column sums
static big big_mul(const big &a, const big &b) {
    big r = big_zero();
    u128 c = 0;
    for (int k = 0; k < BL; k++) {
        for (int i = 0; i <= k; i++) c += (u128)((uint64_t)a.v[i] * b.v[k - i]);
        r.v[k] = (uint32_t)c;
        c >>= 32;
    }
    CHECK(c == 0);
    for (int i = 0; i < BL; i++)
        for (int j = BL - i; j < BL; j++) CHECK(a.v[i] == 0 || b.v[j] == 0);      // nothing fell off the top
    return r;
}
static uint32_t big_mod_small(const big &a, uint32_t p) {
    uint64_t r = 0;
    for (int i = BL - 1; i >= 0; i--) r = ((r << 32) | a.v[i]) % p;
    return (uint32_t)r;
}
// a mod m by shift and subtract
static big big_mod(const big &a, const big &m) {
    big r = big_zero();
    for (int bit = 32 * BL - 1; bit >= 0; bit--) {
        uint32_t carry = (a.v[bit / 32] >> (bit % 32)) & 1;
        for (int i = 0; i < BL; i++) {
            const uint32_t nc = r.v[i] >> 31;
            r.v[i] = (r.v[i] << 1) | carry;
            carry = nc;
        }
        CHECK(carry == 0);
        if (big_cmp(r, m) >= 0) r = big_sub(r, m);
    }
    return r;
}
static big big_l() {
    // 27742317777372353535851937790883648493 = 0x14def9dea2f79cd65812631a5cf5d3ed
    const uint32_t L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u};
    big r = big_zero();
    memcpy(r.v, L, sizeof L);
    return r;
}
static big big_n() {
    // 65000549695646603732796438742359905742570406053903786389881062969044166799969, the BN-256 group order
    const uint32_t N[8] = {0x57ac7261u, 0x1a2ef45bu, 0xf82b3924u, 0x2e8d8e12u, 0x6184dc21u, 0xaa6fecb8u, 0x4aa387f9u,
                           0x8fb501e3u};
    big r = big_zero();
    memcpy(r.v, N, sizeof N);
    return r;
}
static big big_from256(const uint32_t x[8]) {
    big r = big_zero();
    memcpy(r.v, x, 32);
    return r;
}
template <class F>
static bool f_is(const F &a, const big &want) {
    for (int i = 0; i < BL; i++)
        if ((i < 8 ? a.v[i] : 0u) != want.v[i]) return false;
    return true;
}
static fr fr_of(const big &x) {
    fr a;
    for (int i = 8; i < BL; i++) CHECK(x.v[i] == 0);
    memcpy(a.v, x.v, 32);
    return a;
}
static big rnd_below_l() {
    big x = big_zero();
    for (int i = 0; i < 8; i++) x.v[i] = (uint32_t)rnd();
    x.v[7] &= 0x0fffffffu;      // < 2^252 < l
    return x;
}

static const uint32_t PR[NTT31_NP] = NTT31_PRIMES;

// ---- fr_mul_small ----------------------------------------------------------------------------------------------------
static void check_mul_small(const big &a, uint32_t j) {
    CHECK(big_cmp(a, big_l()) < 0 && j < (1u << 31));
    const fr got = fr_mul_small(fr_of(a), j);
    CHECK(f_is(got, big_mod(big_mul_small_add(a, j, 0), big_l())));
    // and limb by limb through unsigned __int128, without the shift-and-subtract reduction: got + q l = a j
    u128 c = 0;
    uint32_t x[9];
    for (int i = 0; i < 8; i++) {
        c += (u128)a.v[i] * j;
        x[i] = (uint32_t)c;
        c >>= 32;
    }
    x[8] = (uint32_t)c;
    // q = (a j - got) / l must be an integer below 2^31: divide the difference's top by l's top as a cross-check
    big diff = big_zero();
    memcpy(diff.v, x, sizeof x);
    big g = big_zero();
    memcpy(g.v, got.v, 32);
    diff = big_sub(diff, g);
    CHECK(big_cmp(big_mod(diff, big_l()), big_zero()) == 0);
    CHECK(big_cmp(g, big_l()) < 0);
}

static void test_mul_small() {
    const big l = big_l();
    big one = big_zero(), lm1 = l;
    one.v[0] = 1;
    lm1.v[0] -= 1;
    big as[8] = {big_zero(), one, lm1};
    for (int t = 3; t < 8; t++) as[t] = rnd_below_l();
    for (const big &a : as) {
        check_mul_small(a, 0);
        check_mul_small(a, 1);
        check_mul_small(a, 0x7fffffffu);
        for (int i = 0; i < NTT31_NP; i++) check_mul_small(a, PR[i]);
    }
    for (int t = 0; t < 4000; t++) {
        big a = rnd_below_l();
        if (t % 7 == 0) {      // close below l: l - 1 - (a small number)
            a = lm1;
            a.v[0] -= (uint32_t)(rnd() & 0xffff);
        }
        check_mul_small(a, (uint32_t)(rnd() & 0x7fffffffu));
    }
    printf("fr mul small ok\n");
}

// ---- Garner and Horner over both fields ------------------------------------------------------------------------------
static void check_value(const big &x, int log_l) {
    const big want_l = big_mod(x, big_l()), want_n = big_mod(x, big_n());
    uint32_t r[NTT31_NP], d[NTT31_NP], res[NTT31_NP], linv[NTT31_NP];
    for (int i = 0; i < NTT31_NP; i++) r[i] = big_mod_small(x, PR[i]);
    ntt31_garner(r, d);
    big back = big_zero();
    for (int i = NTT31_NP - 1; i >= 0; i--) {
        CHECK(d[i] < PR[i]);
        back = big_mul_small_add(back, PR[i], d[i]);
    }
    CHECK(big_cmp(back, x) == 0);
    CHECK(f_is(ntt31_horner_in<fr>(d), want_l));
    CHECK(f_is(ntt31_horner_in<frbn>(d), want_n) && f_is(ntt31_horner(d), want_n));
    // what the inverse transform leaves: x L R mod p, lazy
    for (int i = 0; i < NTT31_NP; i++) {
        const uint64_t l = (uint64_t)1 << log_l;
        res[i] = (uint32_t)((u128)r[i] * (l % PR[i]) % PR[i] * (((uint64_t)1 << 32) % PR[i]) % PR[i]);
        if (rnd() & 1) res[i] += PR[i];
        linv[i] = ntt31_inv_pow2(log_l, PR[i]);
    }
    CHECK(f_is(ntt31_crt_in<fr>(res, linv), want_l));
    CHECK(f_is(ntt31_crt(res, linv), want_n) && f_is(ntt31_crt_in<frbn>(res, linv), want_n));
}

static void test_crt() {
    const big l = big_l();
    big lm1 = l;
    lm1.v[0] -= 1;
    check_value(big_zero(), 1);
    check_value(l, 3);
    check_value(big_mul(l, l), 11);
    printf("crt fixed ok\n");
    // 2^20 (l - 1)^2: the largest coefficient the extension can meet (M <= 2^20 products of residues below l)
    big top = big_mul(lm1, lm1);
    top = big_mul_small_add(top, 1u << 20, 0);
    check_value(top, 21);
    {
        big m = big_zero();      // the primes' product exceeds it
        m.v[0] = 1;
        for (int i = 0; i < NTT31_NP; i++) m = big_mul_small_add(m, PR[i], 0);
        CHECK(big_cmp(m, top) > 0);
    }
    printf("crt largest ok\n");
    for (int t = 0; t < 300; t++) {
        uint32_t d[NTT31_NP];      // a random 18-tuple of digits: any value below the primes' product
        big x = big_zero();
        for (int i = NTT31_NP - 1; i >= 0; i--) {
            d[i] = (uint32_t)(rnd() % PR[i]);
            if (t < 4) d[i] = t & 1 ? PR[i] - 1 : (t & 2 ? 0 : d[i]);
            x = big_mul_small_add(x, PR[i], d[i]);
        }
        check_value(x, 1 + (int)(rnd() % 21));
    }
    printf("crt random ok\n");
}

int main() {
    test_mul_small();
    test_crt();
    return 0;
}
