// CPU check of csrc/ntt31.h (the arithmetic of csrc/bn256_ntt.hip's kernels) against unsigned __int128 and a small
// limb-array big-number type of this file's own.  Built by tests/test_native_ntt31_host.py with g++ under
// AddressSanitizer and UndefinedBehaviorSanitizer and run directly; prints one "<name> ok" line per group.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../verifiable_mpc_amd/csrc/ntt31.h"

typedef unsigned __int128 u128;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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
static big big_pow2(int bit) {
    big r = big_zero();
    r.v[bit / 32] = 1u << (bit % 32);
    return r;
}
static int big_cmp(const big &a, const big &b) {
    for (int i = BL - 1; i >= 0; i--)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i] ? -1 : 1;
    return 0;
}
static big big_add(const big &a, const big &b) {
    big r;
    uint64_t c = 0;
    for (int i = 0; i < BL; i++) {
        c += (uint64_t)a.v[i] + b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    CHECK(c == 0);
    return r;
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
static big big_n() {
    const uint32_t N[8] = VMPC_FRBN_N;
    big r = big_zero();
    memcpy(r.v, N, sizeof N);
    return r;
}
static big big_from256(const uint32_t x[8]) {
    big r = big_zero();
    memcpy(r.v, x, 32);
    return r;
}
static bool frbn_is(const frbn &a, const big &want) {
    for (int i = 0; i < BL; i++)
        if ((i < 8 ? a.v[i] : 0u) != want.v[i]) return false;
    return true;
}

static const uint32_t PR[NTT31_NP] = NTT31_PRIMES;

// ---- Montgomery products -------------------------------------------------------------------------------------------
static void check_mul(uint32_t a, uint32_t b, const ntt31_prime &q) {
    const uint32_t r = ntt31_mul(a, b, q);
    CHECK(r < 2 * (uint64_t)q.p);
    CHECK((uint64_t)(((u128)r << 32) % q.p) == (uint64_t)((u128)a * b % q.p));
}

static void test_montgomery() {
    for (int i = 0; i < NTT31_NP; i++) {
        const ntt31_prime q = ntt31_prime_of(i);
        CHECK(q.p == PR[i] && (q.p - 1) % (1u << NTT31_TWO_ADICITY) == 0 && q.p < (1u << 31) && q.p > (1u << 30));
        CHECK((uint32_t)(q.p * q.ninv) == 0xffffffffu);
        CHECK(q.r1 == (uint32_t)(((uint64_t)1 << 32) % q.p) && q.r2 == (uint32_t)((u128)q.r1 * q.r1 % q.p));
        const uint32_t lazy[4] = {0, 1, q.p - 1, 2 * q.p - 1}, canon[3] = {0, 1, q.p - 1};
        for (uint32_t a : lazy)
            for (uint32_t b : canon) {
                check_mul(a, b, q);
                check_mul(b, a, q);
            }
        for (int t = 0; t < 2000; t++) check_mul((uint32_t)(rnd() % (2 * (uint64_t)q.p)), (uint32_t)(rnd() % q.p), q);
        // lazy sums and differences
        for (int t = 0; t < 2000; t++) {
            const uint32_t a = t == 0 ? 2 * q.p - 1 : (uint32_t)(rnd() % (2 * (uint64_t)q.p));
            const uint32_t b = t < 2 ? 2 * q.p - 1 : t == 2 ? 0 : (uint32_t)(rnd() % (2 * (uint64_t)q.p));
            const uint32_t s = ntt31_add(a, b, q.p), d = ntt31_sub(a, b, q.p);
            CHECK(s < 2 * (uint64_t)q.p && d < 2 * (uint64_t)q.p);
            CHECK(s % q.p == ((uint64_t)a + b) % q.p && d % q.p == ((uint64_t)a + 2 * (uint64_t)q.p - b) % q.p);
        }
        // the roots: order exactly 2^22, inverse of each other
        const uint32_t W[NTT31_NP] = NTT31_ROOT, WI[NTT31_NP] = NTT31_ROOT_INV;
        CHECK(ntt31_pow(W[i], 1u << 22, q) == q.r1 && ntt31_pow(W[i], 1u << 21, q) == q.p - q.r1);
        CHECK(ntt31_csub(ntt31_mul(W[i], WI[i], q), q.p) == q.r1);
    }
    printf("montgomery ok\n");
}

// ---- 256-bit reduction ---------------------------------------------------------------------------------------------
static void check_reduce(const uint32_t x[8]) {
    const big bx = big_from256(x);
    for (int i = 0; i < NTT31_NP; i++) {
        const ntt31_prime q = ntt31_prime_of(i);
        const uint32_t r = ntt31_reduce256(x, q);
        CHECK(r < q.p);
        CHECK(r == (uint32_t)(((u128)big_mod_small(bx, q.p) << 32) % q.p));
    }
}

static void test_reduce() {
    const uint32_t N[8] = VMPC_FRBN_N;
    uint32_t x[8];
    memset(x, 0, sizeof x);
    check_reduce(x);
    memcpy(x, N, sizeof x);
    check_reduce(x);
    x[0] -= 1;
    check_reduce(x);
    memset(x, 0xff, sizeof x);
    check_reduce(x);
    for (int t = 0; t < 500; t++) {
        for (int i = 0; i < 8; i++) x[i] = (uint32_t)rnd();
        if (t % 5 == 0) x[t % 8] = 0xffffffffu;
        check_reduce(x);
    }
    printf("reduce256 ok\n");
}

// ---- transforms through the header's butterflies -------------------------------------------------------------------
static unsigned bitrev(unsigned v, int bits) {
    unsigned r = 0;
    for (int i = 0; i < bits; i++) r |= ((v >> i) & 1) << (bits - 1 - i);
    return r;
}

static void test_transform(int log_l) {
    const int L = 1 << log_l;
    const uint32_t W[NTT31_NP] = NTT31_ROOT, WI[NTT31_NP] = NTT31_ROOT_INV;
    for (int i = 0; i < NTT31_NP; i++) {
        const ntt31_prime q = ntt31_prime_of(i);
        uint32_t x[64], y[64];
        for (int k = 0; k < L; k++) x[k] = y[k] = (uint32_t)(rnd() % q.p);      // Montgomery-form values
        if (i == 0)
            for (int k = 0; k < L; k++) x[k] = y[k] = q.p - 1;
        const uint32_t w = ntt31_pow(W[i], 1u << (22 - log_l), q), wi = ntt31_pow(WI[i], 1u << (22 - log_l), q);
        for (int h = L / 2; h >= 1; h /= 2)             // forward: decimation in frequency
            for (int k = 0; k < L; k++)
                if (!(k & h)) ntt31_dif(y[k], y[k + h], ntt31_pow(w, (uint32_t)((k & (h - 1)) * (L / (2 * h))), q), q);
        for (int k = 0; k < L; k++) {                   // against the definition, at the bit-reversed index
            u128 s = 0;
            for (int j = 0; j < L; j++)
                s += (u128)ntt31_csub(ntt31_mul(x[j], ntt31_pow(w, (uint32_t)((j * k) % L), q), q), q.p);
            CHECK(y[bitrev((unsigned)k, log_l)] < 2 * (uint64_t)q.p);
            CHECK(y[bitrev((unsigned)k, log_l)] % q.p == (uint32_t)(s % q.p));
        }
        for (int h = 1; h < L; h *= 2)                  // inverse: decimation in time, from that order
            for (int k = 0; k < L; k++)
                if (!(k & h)) ntt31_dit(y[k], y[k + h], ntt31_pow(wi, (uint32_t)((k & (h - 1)) * (L / (2 * h))), q), q);
        const uint32_t linv = ntt31_inv_pow2(log_l, q.p);
        CHECK((uint64_t)linv * (uint64_t)L % q.p == 1);
        for (int k = 0; k < L; k++) {
            // times the plain L^-1: out of Montgomery form as well
            const uint32_t plain = ntt31_csub(ntt31_mul(y[k], linv, q), q.p);
            CHECK((uint32_t)(((u128)plain << 32) % q.p) == x[k]);
        }
    }
    printf("transform %d ok\n", L);
}

// ---- Garner and Horner ---------------------------------------------------------------------------------------------
static void check_value(const big &x, int log_l) {
    const big want = big_mod(x, big_n());
    uint32_t r[NTT31_NP], d[NTT31_NP], res[NTT31_NP], linv[NTT31_NP];
    for (int i = 0; i < NTT31_NP; i++) r[i] = big_mod_small(x, PR[i]);
    ntt31_garner(r, d);
    big back = big_zero();
    for (int i = NTT31_NP - 1; i >= 0; i--) {
        CHECK(d[i] < PR[i]);
        back = big_mul_small_add(back, PR[i], d[i]);
    }
    CHECK(big_cmp(back, x) == 0);
    CHECK(frbn_is(ntt31_horner(d), want));
    // what the inverse transform leaves: x L R mod p, lazy
    for (int i = 0; i < NTT31_NP; i++) {
        const uint64_t l = (uint64_t)1 << log_l;
        res[i] = (uint32_t)((u128)r[i] * (l % PR[i]) % PR[i] * (((uint64_t)1 << 32) % PR[i]) % PR[i]);
        if (rnd() & 1) res[i] += PR[i];
        linv[i] = ntt31_inv_pow2(log_l, PR[i]);
    }
    CHECK(frbn_is(ntt31_crt(res, linv), want));
}

static void test_crt() {
    check_value(big_zero(), 1);
    printf("crt zero ok\n");
    // 2^20 (2^256 - 1)^2 = 2^532 - 2^277 + 2^20: the largest coefficient a product at the cap can have
    check_value(big_add(big_sub(big_pow2(532), big_pow2(277)), big_pow2(20)), 21);
    printf("crt largest ok\n");
    // every digit p_i - 1: M - 1
    big m1 = big_zero();
    for (int i = NTT31_NP - 1; i >= 0; i--) m1 = big_mul_small_add(m1, PR[i], PR[i] - 1);
    {
        uint32_t d[NTT31_NP];
        for (int i = 0; i < NTT31_NP; i++) d[i] = PR[i] - 1;
        CHECK(frbn_is(ntt31_horner(d), big_mod(m1, big_n())));
        big m = big_add(m1, big_pow2(0)), lim = big_add(big_sub(big_pow2(532), big_pow2(277)), big_pow2(20));
        CHECK(big_cmp(m, lim) > 0);                                    // 18 primes suffice
        big m17 = big_zero();
        m17.v[0] = 1;
        for (int i = 0; i < NTT31_NP - 1; i++) m17 = big_mul_small_add(m17, PR[i], 0);
        CHECK(big_cmp(m17, lim) < 0);                                  // 17 do not
    }
    check_value(m1, 22);
    printf("crt all-top-digits ok\n");
    for (int t = 0; t < 300; t++) {
        big x = big_zero();
        const int limbs = 1 + (int)(rnd() % 17);                       // up to 544 bits, below M
        for (int i = 0; i < limbs; i++) x.v[i] = (uint32_t)rnd();
        if (limbs == 17) x.v[16] &= 0xffff;
        check_value(x, 1 + (int)(rnd() % 21));
    }
    printf("crt random ok\n");
    // the running products of the generated header
    const uint32_t PM[NTT31_NP][8] = NTT31_PREFIX_MOD_N;
    big run = big_pow2(0);
    for (int i = 0; i < NTT31_NP; i++) {
        frbn f;
        memcpy(f.v, PM[i], 32);
        CHECK(frbn_is(f, big_mod(run, big_n())));
        run = big_mul_small_add(run, PR[i], 0);
    }
    printf("prefix products ok\n");
}

// frbn_mul_small with a 31-bit word, as ntt31_horner uses it
static void test_mul_word() {
    const uint32_t N[8] = VMPC_FRBN_N;
    for (int t = 0; t < 2000; t++) {
        frbn a;
        for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)rnd();
        if (t == 0) memset(a.v, 0xff, 32);
        if (t == 1) {
            memcpy(a.v, N, 32);
            a.v[0] -= 1;
        }
        const uint32_t j = t < 2 ? 0x7fffffffu : PR[t % NTT31_NP];
        CHECK(frbn_is(frbn_mul_small(a, j), big_mod(big_mul_small_add(big_from256(a.v), j, 0), big_n())));
    }
    printf("mul word ok\n");
}

int main() {
    test_montgomery();
    test_reduce();
    test_transform(3);
    test_transform(6);
    test_crt();
    test_mul_word();
    return 0;
}
