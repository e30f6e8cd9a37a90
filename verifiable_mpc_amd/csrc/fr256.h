// One prime field of at most 256 bits, 8 x 32-bit limbs, canonical residues in memory (32 bytes LE), reduced by
// Barrett's method (HAC 14.42 with b = 2^32, k = 8).  fr.h (GF(l), the Ed25519 order) and fr_bn.h (GF(n), the BN-256
// order) instantiate it: each gives a parameter type
//     struct P { uint32_t m[8] = modulus; uint32_t mu[9] = floor(2^512 / modulus); static constexpr int bits; };
// and names f256<P> as its element type, so the two fields are distinct types and mixing them does not compile.
// bits = 256 (2^255 < modulus) is where the fields differ: a sum of two residues then carries into a ninth limb, and
// a 256-bit value is below twice the modulus, so that ONE conditional subtraction canonicalises a load.
// The parameters are read through a function-local `const P p{};`: after unrolling every limb is an immediate and no
// table is read from memory.  VMPC_HD throughout: host-testable (tests/native/frbn_host_test.cpp).
#pragma once
#include <stdint.h>
#include "fe25519.h"  // VMPC_HD

template <class Params>
struct f256 {
    typedef Params P;
    uint32_t v[8];
};

template <class F>
VMPC_HD F f256_zero() {
    F r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
}

template <class F>
VMPC_HD F f256_small(uint32_t k) {
    F r = f256_zero<F>();
    r.v[0] = k;
    return r;
}

template <class F>
VMPC_HD F f256_one() {
    return f256_small<F>(1);
}

template <class F>
VMPC_HD bool f256_equal(const F &a, const F &b) {
    uint32_t o = 0;
#pragma unroll
    for (int l = 0; l < 8; l++) o |= a.v[l] ^ b.v[l];
    return o == 0;
}

// a < modulus ?  (what an entry asks of a 32-byte scalar ARGUMENT before it answers VMPC_E_NONCANON)
template <class F>
VMPC_HD bool f256_is_canonical(const uint32_t a[8]) {
    const typename F::P p{};
    for (int i = 7; i >= 0; i--) {
        if (a[i] > p.m[i]) return false;
        if (a[i] < p.m[i]) return true;
    }
    return false;
}

// r = a - m if a >= m, for a nine-limb a < 2m (a8: the ninth limb, 0 or 1)
template <class F>
VMPC_HD F f256_cond_sub(const F &a, uint32_t a8) {
    const typename F::P p{};
    F s;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (int64_t)a.v[i] - (int64_t)p.m[i];
        s.v[i] = (uint32_t)c;
        c >>= 32;
    }
    c += (int64_t)a8;
    const uint32_t m = (uint32_t)c;  // all ones if borrow (a < m): keep a
    F r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (a.v[i] & m) | (s.v[i] & ~m);
    return r;
}

template <class F>
VMPC_HD F f256_copy(const uint32_t *p) {
    F r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
}

// any 32-byte value -> its canonical residue where one subtraction does it (bits = 256); a plain copy otherwise
template <class F>
VMPC_HD F f256_load(const uint32_t *p) {
    const F r = f256_copy<F>(p);
    return F::P::bits == 256 ? f256_cond_sub(r, 0) : r;
}

template <class F>
VMPC_HD void f256_store(uint32_t *p, const F &a) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}

template <class F>
VMPC_HD F f256_add(const F &a, const F &b) {
    F r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] + b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    // a, b < m: the sum is below 2m; it passes 2^256 only where m passes 2^255
    return f256_cond_sub(r, F::P::bits == 256 ? (uint32_t)c : 0u);
}

template <class F>
VMPC_HD F f256_sub(const F &a, const F &b) {
    const typename F::P p{};
    F r;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (int64_t)a.v[i] - (int64_t)b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    const uint32_t m = (uint32_t)c;  // borrow: add the modulus back
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        d += (uint64_t)r.v[i] + (p.m[i] & m);
        r.v[i] = (uint32_t)d;
        d >>= 32;
    }
    return r;
}

template <class F>
VMPC_HD F f256_neg(const F &a) {
    return f256_sub(f256_zero<F>(), a);
}

// Barrett reduction of a 512-bit value; the quotient estimate is at most two short, so r < 3m < 2^258 lives in nine
// limbs
template <class F>
VMPC_HD F f256_reduce512(const uint32_t x[16]) {
    const typename F::P p{};
    // q1 = x >> 224 (x[7..15]); q2 = q1 * mu (18 limbs); q3 = q2 >> 288 (q2[9..17])
    uint32_t q2[18];
#pragma unroll
    for (int i = 0; i < 18; i++) q2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            c += (uint64_t)x[7 + i] * p.mu[j] + q2[i + j];
            q2[i + j] = (uint32_t)c;
            c >>= 32;
        }
        q2[i + 9] = (uint32_t)c;
    }
    // r2 = (q3 * m) mod 2^288
    uint32_t r2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) r2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (i + j < 9) {
                c += (uint64_t)q2[9 + i] * p.m[j] + r2[i + j];
                r2[i + j] = (uint32_t)c;
                c >>= 32;
            }
        }
        if (i + 8 < 9) r2[i + 8] = (uint32_t)c;
    }
    // r = (x mod 2^288) - r2 (mod 2^288); 0 <= r < 3m
    uint32_t r[9];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c += (int64_t)x[i] - (int64_t)r2[i];
        r[i] = (uint32_t)c;
        c >>= 32;
    }
    // at most two subtractions of m (nine-limb compare)
#pragma unroll
    for (int k = 0; k < 2; k++) {
        uint32_t s[9];
        int64_t b = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            b += (int64_t)r[i] - (int64_t)(i < 8 ? p.m[i] : 0u);
            s[i] = (uint32_t)b;
            b >>= 32;
        }
        const uint32_t m = (uint32_t)b;  // borrow: keep r
#pragma unroll
        for (int i = 0; i < 9; i++) r[i] = (r[i] & m) | (s[i] & ~m);
    }
    F out;
#pragma unroll
    for (int i = 0; i < 8; i++) out.v[i] = r[i];
    return out;
}

template <class F>
VMPC_HD void f256_mul_wide(uint32_t t[16], const F &a, const F &b) {
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
}

template <class F>
VMPC_HD F f256_mul(const F &a, const F &b) {
    uint32_t t[16];
    f256_mul_wide(t, a, b);
    return f256_reduce512<F>(t);
}

// a^(m-2) = 1/a for a != 0 (Fermat; 0 -> 0): a squaring per bit of m - 2 and one product per set bit, left to right
template <class F>
VMPC_HD F f256_inv(const F &a) {
    const typename F::P p{};
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = p.m[i];
    e[0] -= 2;  // the modulus is odd and its low limb exceeds 2: no borrow
    F r = f256_one<F>();
    for (int i = F::P::bits - 1; i >= 0; i--) {
        r = f256_mul(r, r);
        if ((e[i >> 5] >> (i & 31)) & 1u) r = f256_mul(r, a);
    }
    return r;
}

// ---- the wide accumulator of sums of products ------------------------------------------------------------------------
// value = sum_k lo[k] 2^(32 k) + sum_i hi[i] 2^(32 (i + 8)).  f256_acc_mac adds one unreduced 8 x 8-limb product: row i
// of the schoolbook product runs its carry chain through lo[i .. i+7] and drops the carry that leaves the row into
// hi[i], a 64-bit counter, instead of rippling it to the top - so no limb above the row is touched and nothing is
// lost: after m products every hi[i] is below m 2^32, i.e. m < 2^32 products never overflow, whatever the field.
// F256_ACC_MAX_PRODUCTS states that interval for the kernels that accumulate without reducing: a product adds at most
// 2^32 - 1 (a row's outgoing carry) to a 64-bit counter, and 2^32 (2^32 - 1) < 2^64.
#define F256_ACC_MAX_PRODUCTS ((uint64_t)1 << 32)
static_assert(F256_ACC_MAX_PRODUCTS <= UINT64_MAX / 0xFFFFFFFFull, "f256_acc: a carry counter could wrap");
struct f256_acc {
    uint32_t lo[16];
    uint64_t hi[8];
};

VMPC_HD f256_acc f256_acc_zero() {
    f256_acc s;
#pragma unroll
    for (int i = 0; i < 16; i++) s.lo[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s.hi[i] = 0;
    return s;
}

VMPC_HD void f256_acc_mac(f256_acc &s, const uint32_t a[8], const uint32_t b[8]) {
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

// the accumulator's value mod m.  It is below 2^545 (hi[7] < 2^64 sits at bit 480): written as 18 limbs w, the top 16
// are reduced first and each lower limb is then shifted in (r 2^32 + limb < 2^288 is a valid Barrett input).
template <class F>
VMPC_HD F f256_acc_reduce(const f256_acc &s) {
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
    F r = f256_reduce512<F>(w + 2);
#pragma unroll
    for (int k = 1; k >= 0; k--) {
        uint32_t t[16];
        t[0] = w[k];
#pragma unroll
        for (int i = 0; i < 8; i++) t[i + 1] = r.v[i];
#pragma unroll
        for (int i = 9; i < 16; i++) t[i] = 0;
        r = f256_reduce512<F>(t);
    }
    return r;
}

// ---- element i of a vector in device memory: two 16-byte accesses, through f256_load -----------------------------------
#ifdef __HIPCC__
template <class F>
__device__ __forceinline__ F f256_ld(const void *p, long long i) {
    const uint4 *q = (const uint4 *)((const uint32_t *)p + 8 * i);
    const uint4 x = q[0], y = q[1];
    const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    return f256_load<F>(w);
}

template <class F>
__device__ __forceinline__ void f256_st(void *p, long long i, const F &a) {
    uint4 *q = (uint4 *)((uint32_t *)p + 8 * i);
    q[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    q[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}

// zero where i leaves [0, n)
template <class F>
__device__ __forceinline__ F f256_ld_or_zero(const void *p, long long i, long long n) {
    if (i < 0 || i >= n) return f256_zero<F>();
    return f256_ld<F>(p, i);
}
#endif
