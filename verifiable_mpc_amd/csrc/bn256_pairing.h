// BN-256 optimal-ate pairing over fp29.h: the tower, the Miller loop and the final exponentiation.
//
// What it computes: the reference's optimal_ate (verifiable_mpc/ac20/pairing.py:614-643) - coefficient for
// coefficient - for a point P of G1 and a point Q of the sextic twist y^2 = x^3 + 3/xi:
//     Fp2  = Fp[i]/(i^2 + 1)                  (fp29x2)
//     Fp6  = Fp2[tau]/(tau^3 - xi), xi = i + 3  element x tau^2 + y tau + z   (pairing.py:100-265)
//     Fp12 = Fp6[w]/(w^2 - tau)                 element x w + y               (pairing.py:268-370)
//     f    = f_{6u+2,Q}(P) l_{T,pi(Q)}(P) l_{T',-pi^2(Q)}(P)   over the NAF of 6u+2   (pairing.py:503-554)
//     e    = f^((p^12 - 1) / N)  (easy part, then the hard part of eprint 2010/354 Alg. 31, pairing.py:557-611)
// The lines are the reference's in value up to a factor in Fp2, which the final exponentiation removes: Q is
// untwisted into E(Fp12) by (x, y) -> (x w^2, y w^3), so the affine line through T with slope lambda' w evaluated
// at P is  y_P - lambda' x_P w + (lambda' x_T - y_T) w^3  (w^3 = tau w).  With T Jacobian (X : Y : Z) and the
// denominator of lambda' cleared (an Fp2 factor):
//     doubling:       y_P * Z3 Z^2,   tau w: 3 X^3 - 2 Y^2,         w: -3 X^2 Z^2 x_P        (Z3 = 2 Y Z)
//     adding (x2,y2): y_P * Z3,       tau w: R x2 - y2 Z3,          w: -R x_P    (R = y2 Z^3 - Y, Z3 = Z H)
// tests/bn256_pairing_ref.py states the same map with affine lines and the plain power; the host harness
// (tests/native/pairing_host_test.cpp) and the GPU tests compare the two.
//
// Values: every Fp element is an fp29 (Montgomery 2^261, < 2p).  VMPC_HD: host-testable.
#pragma once
#include "fp29.h"

// The Fp6 / Fp12 products and the line steps stay out-of-line on the device: fully inlined, one Miller loop plus a
// final exponentiation is several hundred thousand instructions and the compiler takes the better part of an hour
// over it.  (The host harness builds them inline.)
#if defined(__HIP_DEVICE_COMPILE__)
#define BNP_NOINLINE __attribute__((noinline))
#else
#define BNP_NOINLINE
#endif

// ---- constants (Montgomery form, 9 x 29-bit limbs) ---------------------------------------------------------------
// gamma_k = xi^(k(p-1)/6) in Fp2 (the p-power Frobenius: w^p = gamma_1 w)
#define BNP_G1A { 0x1b8c9499u, 0x047dea76u, 0x0f0bcc1au, 0x18497c7du, 0x14324ec5u, 0x1c728cc5u, 0x1013af21u, 0x085868a4u, 0x00459a0bu }
#define BNP_G1B { 0x0ef9b6e0u, 0x0f529884u, 0x16c3512du, 0x09157773u, 0x08627b03u, 0x12e872c2u, 0x02913e80u, 0x14fa9974u, 0x002f2331u }
#define BNP_G2A { 0x073d723cu, 0x0f523801u, 0x1c9ca518u, 0x1d708a8fu, 0x0f80db97u, 0x073182cdu, 0x0ba39202u, 0x1b2491a6u, 0x0056d90fu }
#define BNP_G2B { 0x040feadau, 0x1ced9a24u, 0x17b9173du, 0x12365a20u, 0x1c5c27deu, 0x1c1cafb8u, 0x086d85d3u, 0x07d3b71au, 0x0075e742u }
#define BNP_G3A { 0x09df7f2eu, 0x050c5e63u, 0x0f4c1710u, 0x0c587d07u, 0x06d69e00u, 0x09bf245au, 0x15270a8cu, 0x16c03156u, 0x00043565u }
#define BNP_G3B { 0x1d9e7d8au, 0x0f251b29u, 0x0de44530u, 0x05097716u, 0x1483da01u, 0x1d3d6d0eu, 0x1f751fa4u, 0x04409403u, 0x000ca031u }
#define BNP_G4A { 0x094d1242u, 0x1a811b92u, 0x022a02fbu, 0x0ac1aa16u, 0x060c336fu, 0x00757ae1u, 0x0cb19f51u, 0x089aacfau, 0x005afde7u }
#define BNP_G4B { 0x02451ed6u, 0x162e2018u, 0x1c6ddd66u, 0x1978f743u, 0x0c5de610u, 0x0eb21a8fu, 0x19acde94u, 0x0c174e18u, 0x00224b1bu }
#define BNP_G5A { 0x0eb6237du, 0x12f7c7a1u, 0x07ed2dcau, 0x105b8864u, 0x1ea9b1dbu, 0x0078d631u, 0x1ccdb71fu, 0x032335bcu, 0x003d64d0u }
#define BNP_G5B { 0x16ee7da7u, 0x065bfc12u, 0x1a194dd9u, 0x1b503cc8u, 0x17e756f7u, 0x09992c5du, 0x1496a605u, 0x0cf90559u, 0x007e8b3bu }
// delta_k = xi^(k(p^2-1)/6) = gamma_k conj(gamma_k), in Fp (the p^2-power Frobenius)
#define BNP_D1 { 0x09309f73u, 0x1a9ad7e5u, 0x0ec8844du, 0x062704aau, 0x06c2b88cu, 0x170b93d9u, 0x0d7296e5u, 0x0532a266u, 0x00885f53u }
#define BNP_D2 { 0x191a1c62u, 0x1fadf8ecu, 0x0c249128u, 0x0914253bu, 0x16fb99b2u, 0x11926f23u, 0x07ce6294u, 0x18a66f8fu, 0x0087acbeu }
#define BNP_D3 { 0x0df21356u, 0x07f8846au, 0x0ac97461u, 0x19fec2d2u, 0x1dfb000bu, 0x10e30c0cu, 0x1a42756eu, 0x0fdd2199u, 0x008f026du }
#define BNP_D4 { 0x14d7f6f4u, 0x084a8b7du, 0x1ea4e338u, 0x10ea9d96u, 0x06ff6659u, 0x1f509ce9u, 0x127412d9u, 0x1736b20au, 0x000755aeu }
#define BNP_D5 { 0x04ee7a05u, 0x03376a76u, 0x0148d65du, 0x0dfd7d06u, 0x16c68533u, 0x04c9c19eu, 0x1818472bu, 0x03c2e4e1u, 0x00080843u }
// 6u + 2 in non-adjacent form: 66 digits, the top one (bit 65) is +1, bit 64 is 0; +1 / -1 digits of bits 0..63
#define BNP_NAF_POS 0x200820220a141208ull
#define BNP_NAF_NEG 0x0140088080010000ull
// u = 1868033^3 (pairing.py:44-47)
#define BNP_U 0x5a76ae9aec588301ull

// ---- Fp2 helpers -------------------------------------------------------------------------------------------------
VMPC_HD fp29x2 f2_zero() { return Fp29x2Ops::zero(); }
VMPC_HD fp29x2 f2_one() { return Fp29x2Ops::one(); }
VMPC_HD fp29x2 f2_add(const fp29x2 &x, const fp29x2 &y) { return Fp29x2Ops::add(x, y); }
VMPC_HD fp29x2 f2_sub(const fp29x2 &x, const fp29x2 &y) { return Fp29x2Ops::sub(x, y); }
VMPC_HD fp29x2 f2_neg(const fp29x2 &x) { return Fp29x2Ops::neg(x); }
VMPC_HD fp29x2 f2_dbl(const fp29x2 &x) { return Fp29x2Ops::add(x, x); }
VMPC_HD fp29x2 f2_mul(const fp29x2 &x, const fp29x2 &y) { return fp29x2_mul(x, y); }
VMPC_HD fp29x2 f2_sqr(const fp29x2 &x) { return fp29x2_sqr(x); }
VMPC_HD fp29x2 f2_inv(const fp29x2 &x) { return Fp29x2Ops::inv(x); }
VMPC_HD bool f2_is_zero(const fp29x2 &x) { return Fp29x2Ops::is_zero(x); }
VMPC_HD fp29x2 f2_conj(const fp29x2 &x) {
    fp29x2 r;
    r.a = x.a;
    r.b = fp29_neg(x.b);
    return r;
}
VMPC_HD fp29x2 f2_mul_fp(const fp29x2 &x, const fp29 &s) {
    fp29x2 r;
    r.a = fp29_mul(x.a, s);
    r.b = fp29_mul(x.b, s);
    return r;
}
// x xi = (a + b i)(3 + i) = (3a - b) + (a + 3b) i
VMPC_HD fp29x2 f2_mul_xi(const fp29x2 &x) {
    fp29x2 r;
    const fp29 a3 = fp29_add(fp29_dbl(x.a), x.a), b3 = fp29_add(fp29_dbl(x.b), x.b);
    r.a = fp29_sub(a3, x.b);
    r.b = fp29_add(x.a, b3);
    return r;
}
VMPC_HD fp29x2 f2_const(const uint32_t (&a)[FP29_LIMBS], const uint32_t (&b)[FP29_LIMBS]) {
    fp29x2 r;
#pragma unroll
    for (int k = 0; k < FP29_LIMBS; k++) {
        r.a.v[k] = a[k];
        r.b.v[k] = b[k];
    }
    return r;
}
VMPC_HD fp29 fp_const(const uint32_t (&a)[FP29_LIMBS]) {
    fp29 r;
#pragma unroll
    for (int k = 0; k < FP29_LIMBS; k++) r.v[k] = a[k];
    return r;
}

// ---- Fp6 = Fp2[tau]/(tau^3 - xi): x tau^2 + y tau + z ------------------------------------------------------------
struct fp6 {
    fp29x2 x, y, z;
};
VMPC_HD fp6 f6_zero() {
    fp6 r;
    r.x = f2_zero();
    r.y = f2_zero();
    r.z = f2_zero();
    return r;
}
VMPC_HD fp6 f6_one() {
    fp6 r = f6_zero();
    r.z = f2_one();
    return r;
}
VMPC_HD fp6 f6_add(const fp6 &a, const fp6 &b) {
    fp6 r;
    r.x = f2_add(a.x, b.x);
    r.y = f2_add(a.y, b.y);
    r.z = f2_add(a.z, b.z);
    return r;
}
VMPC_HD fp6 f6_sub(const fp6 &a, const fp6 &b) {
    fp6 r;
    r.x = f2_sub(a.x, b.x);
    r.y = f2_sub(a.y, b.y);
    r.z = f2_sub(a.z, b.z);
    return r;
}
VMPC_HD fp6 f6_neg(const fp6 &a) {
    fp6 r;
    r.x = f2_neg(a.x);
    r.y = f2_neg(a.y);
    r.z = f2_neg(a.z);
    return r;
}
// a tau: (x, y, z) -> (y, z, xi x)
VMPC_HD fp6 f6_mul_tau(const fp6 &a) {
    fp6 r;
    r.x = a.y;
    r.y = a.z;
    r.z = f2_mul_xi(a.x);
    return r;
}
// Karatsuba over the three coefficients (a0 = z, a1 = y, a2 = x): 6 Fp2 products
BNP_NOINLINE VMPC_HD fp6 f6_mul(const fp6 &a, const fp6 &b) {
    const fp29x2 v0 = f2_mul(a.z, b.z), v1 = f2_mul(a.y, b.y), v2 = f2_mul(a.x, b.x);
    fp6 r;
    // r0 = v0 + xi ((a1 + a2)(b1 + b2) - v1 - v2)
    r.z = f2_add(v0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(a.y, a.x), f2_add(b.y, b.x)), v1), v2)));
    // r1 = (a0 + a1)(b0 + b1) - v0 - v1 + xi v2
    r.y = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.z, a.y), f2_add(b.z, b.y)), v0), v1), f2_mul_xi(v2));
    // r2 = (a0 + a2)(b0 + b2) - v0 - v2 + v1
    r.x = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.z, a.x), f2_add(b.z, b.x)), v0), v2), v1);
    return r;
}
// r0 = a0^2 + 2 xi a1 a2, r1 = 2 a0 a1 + xi a2^2, r2 = a1^2 + 2 a0 a2
BNP_NOINLINE VMPC_HD fp6 f6_sqr(const fp6 &a) {
    const fp29x2 s0 = f2_sqr(a.z), s1 = f2_sqr(a.y), s2 = f2_sqr(a.x);
    const fp29x2 m12 = f2_dbl(f2_mul(a.y, a.x)), m01 = f2_dbl(f2_mul(a.z, a.y)), m02 = f2_dbl(f2_mul(a.z, a.x));
    fp6 r;
    r.z = f2_add(s0, f2_mul_xi(m12));
    r.y = f2_add(m01, f2_mul_xi(s2));
    r.x = f2_add(s1, m02);
    return r;
}
VMPC_HD fp6 f6_mul_f2(const fp6 &a, const fp29x2 &k) {
    fp6 r;
    r.x = f2_mul(a.x, k);
    r.y = f2_mul(a.y, k);
    r.z = f2_mul(a.z, k);
    return r;
}
// a (b1 tau + b0): 5 Fp2 products
BNP_NOINLINE VMPC_HD fp6 f6_mul_01(const fp6 &a, const fp29x2 &b0, const fp29x2 &b1) {
    const fp29x2 v0 = f2_mul(a.z, b0), v1 = f2_mul(a.y, b1);
    fp6 r;
    r.z = f2_add(v0, f2_mul_xi(f2_mul(a.x, b1)));
    r.y = f2_sub(f2_sub(f2_mul(f2_add(a.z, a.y), f2_add(b0, b1)), v0), v1);
    r.x = f2_add(v1, f2_mul(a.x, b0));
    return r;
}
// the adjugate of the multiplication matrix over its determinant
BNP_NOINLINE VMPC_HD fp6 f6_inv(const fp6 &a) {
    const fp29x2 A = f2_sub(f2_sqr(a.z), f2_mul_xi(f2_mul(a.y, a.x)));
    const fp29x2 B = f2_sub(f2_mul_xi(f2_sqr(a.x)), f2_mul(a.z, a.y));
    const fp29x2 C = f2_sub(f2_sqr(a.y), f2_mul(a.z, a.x));
    const fp29x2 det = f2_add(f2_mul(a.z, A), f2_mul_xi(f2_add(f2_mul(a.x, B), f2_mul(a.y, C))));
    const fp29x2 di = f2_inv(det);
    fp6 r;
    r.z = f2_mul(A, di);
    r.y = f2_mul(B, di);
    r.x = f2_mul(C, di);
    return r;
}

// ---- Fp12 = Fp6[w]/(w^2 - tau): x w + y -------------------------------------------------------------------------
struct fp12 {
    fp6 x, y;
};
VMPC_HD fp12 f12_one() {
    fp12 r;
    r.x = f6_zero();
    r.y = f6_one();
    return r;
}
BNP_NOINLINE VMPC_HD fp12 f12_mul(const fp12 &a, const fp12 &b) {
    const fp6 t0 = f6_mul(a.y, b.y), t1 = f6_mul(a.x, b.x);
    fp12 r;
    r.x = f6_sub(f6_sub(f6_mul(f6_add(a.x, a.y), f6_add(b.x, b.y)), t0), t1);
    r.y = f6_add(t0, f6_mul_tau(t1));
    return r;
}
// (x w + y)^2 = 2xy w + (y^2 + x^2 tau);  y^2 + x^2 tau = (x + y)(x tau + y) - xy - xy tau
BNP_NOINLINE VMPC_HD fp12 f12_sqr(const fp12 &a) {
    const fp6 v0 = f6_mul(a.x, a.y);
    fp12 r;
    r.y = f6_sub(f6_sub(f6_mul(f6_add(a.x, a.y), f6_add(f6_mul_tau(a.x), a.y)), v0), f6_mul_tau(v0));
    r.x = f6_add(v0, v0);
    return r;
}
// the p^6-power map: w -> -w
VMPC_HD fp12 f12_conj(const fp12 &a) {
    fp12 r;
    r.x = f6_neg(a.x);
    r.y = a.y;
    return r;
}
// (x w + y)^-1 = (y - x w) / (y^2 - x^2 tau)
BNP_NOINLINE VMPC_HD fp12 f12_inv(const fp12 &a) {
    const fp6 d = f6_inv(f6_sub(f6_sqr(a.y), f6_mul_tau(f6_sqr(a.x))));
    fp12 r;
    r.x = f6_neg(f6_mul(a.x, d));
    r.y = f6_mul(a.y, d);
    return r;
}
// p-power map: in the w basis sum c_k w^k -> sum conj(c_k) gamma_k w^k; tower slots: x.z w, y.y w^2, x.y w^3,
// y.x w^4, x.x w^5
BNP_NOINLINE VMPC_HD fp12 f12_frob(const fp12 &a) {
    const uint32_t g1a[FP29_LIMBS] = BNP_G1A, g1b[FP29_LIMBS] = BNP_G1B, g2a[FP29_LIMBS] = BNP_G2A,
                   g2b[FP29_LIMBS] = BNP_G2B, g3a[FP29_LIMBS] = BNP_G3A, g3b[FP29_LIMBS] = BNP_G3B,
                   g4a[FP29_LIMBS] = BNP_G4A, g4b[FP29_LIMBS] = BNP_G4B, g5a[FP29_LIMBS] = BNP_G5A,
                   g5b[FP29_LIMBS] = BNP_G5B;
    fp12 r;
    r.y.z = f2_conj(a.y.z);
    r.x.z = f2_mul(f2_conj(a.x.z), f2_const(g1a, g1b));
    r.y.y = f2_mul(f2_conj(a.y.y), f2_const(g2a, g2b));
    r.x.y = f2_mul(f2_conj(a.x.y), f2_const(g3a, g3b));
    r.y.x = f2_mul(f2_conj(a.y.x), f2_const(g4a, g4b));
    r.x.x = f2_mul(f2_conj(a.x.x), f2_const(g5a, g5b));
    return r;
}
// p^2-power map: c_k -> c_k delta_k (delta_k in Fp)
BNP_NOINLINE VMPC_HD fp12 f12_frob2(const fp12 &a) {
    const uint32_t d1[FP29_LIMBS] = BNP_D1, d2[FP29_LIMBS] = BNP_D2, d3[FP29_LIMBS] = BNP_D3,
                   d4[FP29_LIMBS] = BNP_D4, d5[FP29_LIMBS] = BNP_D5;
    fp12 r;
    r.y.z = a.y.z;
    r.x.z = f2_mul_fp(a.x.z, fp_const(d1));
    r.y.y = f2_mul_fp(a.y.y, fp_const(d2));
    r.x.y = f2_mul_fp(a.x.y, fp_const(d3));
    r.y.x = f2_mul_fp(a.y.x, fp_const(d4));
    r.x.x = f2_mul_fp(a.x.x, fp_const(d5));
    return r;
}
VMPC_HD bool f12_is_one(const fp12 &a) {
    return fp29_is_zero(fp29_sub(a.y.z.a, fp29_one())) && fp29_is_zero(a.y.z.b) && f2_is_zero(a.y.y) &&
           f2_is_zero(a.y.x) && f2_is_zero(a.x.x) && f2_is_zero(a.x.y) && f2_is_zero(a.x.z);
}
// a^u, u = 1868033^3 (63 bits), left to right
BNP_NOINLINE VMPC_HD fp12 f12_pow_u(const fp12 &a) {
    fp12 r = a;
    for (int b = 61; b >= 0; b--) {
        r = f12_sqr(r);
        if ((BNP_U >> b) & 1ull) r = f12_mul(r, a);
    }
    return r;
}

// ---- line functions and the sparse product ----------------------------------------------------------------------
// a line value l = (0, b1, b0) w + (0, 0, c0): b1 at tau w, b0 at w, c0 at 1
struct bnp_line {
    fp29x2 b0, b1, c0;
};
struct bnp_g2 {                  // Jacobian point of the twist
    fp29x2 X, Y, Z;
};

// f l, 13 Fp2 products
BNP_NOINLINE VMPC_HD fp12 f12_mul_line(const fp12 &f, const bnp_line &l) {
    const fp6 yc = f6_mul_f2(f.y, l.c0);                 // f.y * (c0)
    const fp6 xb = f6_mul_01(f.x, l.b0, l.b1);           // f.x * (b1 tau + b0)
    fp12 r;
    // x' = (f.x + f.y)(b1 tau + b0 + c0) - f.x(b1 tau + b0) - f.y c0
    r.x = f6_sub(f6_sub(f6_mul_01(f6_add(f.x, f.y), f2_add(l.b0, l.c0), l.b1), xb), yc);
    // y' = f.y c0 + f.x (b1 tau + b0) tau
    r.y = f6_add(yc, f6_mul_tau(xb));
    return r;
}

// T <- 2T and the tangent line at T evaluated at P = (xp, yp)
BNP_NOINLINE VMPC_HD bnp_line bnp_dbl(bnp_g2 &t, const fp29 &xp, const fp29 &yp) {
    const fp29x2 XX = f2_sqr(t.X), YY = f2_sqr(t.Y), ZZ = f2_sqr(t.Z);
    const fp29x2 M = f2_add(f2_dbl(XX), XX);                          // 3 X^2
    const fp29x2 S = f2_dbl(f2_dbl(f2_mul(t.X, YY)));                 // 4 X Y^2
    const fp29x2 YYYY8 = f2_dbl(f2_dbl(f2_dbl(f2_sqr(YY))));          // 8 Y^4
    bnp_line l;
    l.b1 = f2_sub(f2_mul(M, t.X), f2_dbl(YY));                        // 3 X^3 - 2 Y^2
    l.b0 = f2_neg(f2_mul_fp(f2_mul(M, ZZ), xp));                      // -3 X^2 Z^2 x_P
    const fp29x2 Z3 = f2_dbl(f2_mul(t.Y, t.Z));                       // 2 Y Z
    l.c0 = f2_mul_fp(f2_mul(Z3, ZZ), yp);                             // 2 Y Z^3 y_P
    const fp29x2 X3 = f2_sub(f2_sqr(M), f2_dbl(S));
    t.Y = f2_sub(f2_mul(M, f2_sub(S, X3)), YYYY8);
    t.X = X3;
    t.Z = Z3;
    return l;
}

// T <- T + (x2, y2) (affine, T != +-(x2, y2)) and the line through them evaluated at P
BNP_NOINLINE VMPC_HD bnp_line bnp_add(bnp_g2 &t, const fp29x2 &x2, const fp29x2 &y2, const fp29 &xp, const fp29 &yp) {
    const fp29x2 ZZ = f2_sqr(t.Z);
    const fp29x2 H = f2_sub(f2_mul(x2, ZZ), t.X);
    const fp29x2 R = f2_sub(f2_mul(y2, f2_mul(ZZ, t.Z)), t.Y);
    const fp29x2 HH = f2_sqr(H), HHH = f2_mul(H, HH), V = f2_mul(t.X, HH);
    const fp29x2 Z3 = f2_mul(t.Z, H);
    bnp_line l;
    l.b1 = f2_sub(f2_mul(R, x2), f2_mul(y2, Z3));
    l.b0 = f2_neg(f2_mul_fp(R, xp));
    l.c0 = f2_mul_fp(Z3, yp);
    const fp29x2 X3 = f2_sub(f2_sub(f2_sqr(R), HHH), f2_dbl(V));
    t.Y = f2_sub(f2_mul(R, f2_sub(V, X3)), f2_mul(t.Y, HHH));
    t.X = X3;
    t.Z = Z3;
    return l;
}

// ---- Miller loop and final exponentiation ------------------------------------------------------------------------
// P = (xp, yp) in G1, Q = (xq, yq) on the twist, both affine, finite
VMPC_HD fp12 bnp_miller(const fp29 &xp, const fp29 &yp, const fp29x2 &xq, const fp29x2 &yq) {
    bnp_g2 t;
    t.X = xq;
    t.Y = yq;
    t.Z = f2_one();
    const fp29x2 myq = f2_neg(yq);
    fp12 f = f12_one();
    for (int i = 64; i >= 0; i--) {          // digits below the leading one (bit 64 is a zero digit)
        f = f12_sqr(f);
        f = f12_mul_line(f, bnp_dbl(t, xp, yp));
        const bool pos = i < 64 && ((BNP_NAF_POS >> i) & 1ull), neg = i < 64 && ((BNP_NAF_NEG >> i) & 1ull);
        if (pos || neg) f = f12_mul_line(f, bnp_add(t, xq, pos ? yq : myq, xp, yp));
    }
    // Q1 = pi(Q): (conj(x) gamma_2, conj(y) gamma_3);  Q2 = -pi^2(Q): (x delta_2, y)
    const uint32_t g2a[FP29_LIMBS] = BNP_G2A, g2b[FP29_LIMBS] = BNP_G2B, g3a[FP29_LIMBS] = BNP_G3A,
                   g3b[FP29_LIMBS] = BNP_G3B, d2[FP29_LIMBS] = BNP_D2;
    const fp29x2 x1 = f2_mul(f2_conj(xq), f2_const(g2a, g2b)), y1 = f2_mul(f2_conj(yq), f2_const(g3a, g3b));
    f = f12_mul_line(f, bnp_add(t, x1, y1, xp, yp));
    const fp29x2 x2 = f2_mul_fp(xq, fp_const(d2));
    f = f12_mul_line(f, bnp_add(t, x2, yq, xp, yp));
    return f;
}

// f^((p^12 - 1) / N): easy part f^((p^6 - 1)(p^2 + 1)), then the hard part (p^4 - p^2 + 1) / N as the addition chain
// of eprint 2010/354 Algorithm 31 over t^u, t^(u^2), t^(u^3) and Frobenius images
VMPC_HD fp12 bnp_final_exp(const fp12 &in) {
    fp12 t1 = f12_mul(f12_conj(in), f12_inv(in));
    t1 = f12_mul(t1, f12_frob2(t1));

    const fp12 fp1 = f12_frob(t1), fp2 = f12_frob2(t1), fp3 = f12_frob(fp2);
    const fp12 fu1 = f12_pow_u(t1);
    const fp12 fu2 = f12_pow_u(fu1);
    const fp12 fu3 = f12_pow_u(fu2);

    const fp12 y0 = f12_mul(f12_mul(fp1, fp2), fp3);
    const fp12 y1 = f12_conj(t1);
    const fp12 y2 = f12_frob2(fu2);
    const fp12 y3 = f12_conj(f12_frob(fu1));
    const fp12 y4 = f12_conj(f12_mul(fu1, f12_frob(fu2)));
    const fp12 y5 = f12_conj(fu2);
    const fp12 y6 = f12_conj(f12_mul(fu3, f12_frob(fu3)));

    fp12 t0 = f12_mul(f12_mul(f12_sqr(y6), y4), y5);
    fp12 t = f12_mul(f12_mul(y3, y5), t0);
    t0 = f12_mul(t0, y2);
    t = f12_mul(f12_sqr(t), t0);
    t = f12_sqr(t);
    t0 = f12_mul(t, y1);
    t = f12_mul(t, y0);
    t0 = f12_sqr(t0);
    return f12_mul(t0, t);
}

// ---- exchange format: 12 canonical 32-byte LE residues, order x.x, x.y, x.z, y.x, y.y, y.z, each (re, im) --------
VMPC_HD void f12_store(uint32_t *dst, const fp12 &a) {
    Fp29x2Ops::store(dst + 0, a.x.x);
    Fp29x2Ops::store(dst + 16, a.x.y);
    Fp29x2Ops::store(dst + 32, a.x.z);
    Fp29x2Ops::store(dst + 48, a.y.x);
    Fp29x2Ops::store(dst + 64, a.y.y);
    Fp29x2Ops::store(dst + 80, a.y.z);
}
VMPC_HD fp12 f12_load(const uint32_t *src) {
    fp12 a;
    a.x.x = Fp29x2Ops::load(src + 0);
    a.x.y = Fp29x2Ops::load(src + 16);
    a.x.z = Fp29x2Ops::load(src + 32);
    a.y.x = Fp29x2Ops::load(src + 48);
    a.y.y = Fp29x2Ops::load(src + 64);
    a.y.z = Fp29x2Ops::load(src + 80);
    return a;
}
// workspace format (Montgomery residues, shifts only)
VMPC_HD void f12_store_raw(uint32_t *dst, const fp12 &a) {
    Fp29x2Ops::store_raw(dst + 0, a.x.x);
    Fp29x2Ops::store_raw(dst + 16, a.x.y);
    Fp29x2Ops::store_raw(dst + 32, a.x.z);
    Fp29x2Ops::store_raw(dst + 48, a.y.x);
    Fp29x2Ops::store_raw(dst + 64, a.y.y);
    Fp29x2Ops::store_raw(dst + 80, a.y.z);
}
VMPC_HD fp12 f12_load_raw(const uint32_t *src) {
    fp12 a;
    a.x.x = Fp29x2Ops::load_raw(src + 0);
    a.x.y = Fp29x2Ops::load_raw(src + 16);
    a.x.z = Fp29x2Ops::load_raw(src + 32);
    a.y.x = Fp29x2Ops::load_raw(src + 48);
    a.y.y = Fp29x2Ops::load_raw(src + 64);
    a.y.z = Fp29x2Ops::load_raw(src + 80);
    return a;
}

// e(P, Q) from the 64-byte G1 and 128-byte twist affine encodings (canonical LE; all zero = infinity -> 1): the
// Miller value only (final exponentiation separately)
VMPC_HD fp12 bnp_miller_enc(const uint32_t *g1, const uint32_t *g2) {
    uint32_t o1 = 0, o2 = 0;
    for (int k = 0; k < 16; k++) o1 |= g1[k];
    for (int k = 0; k < 32; k++) o2 |= g2[k];
    if (o1 == 0 || o2 == 0) return f12_one();
    return bnp_miller(Fp29Ops::load(g1), Fp29Ops::load(g1 + 8), Fp29x2Ops::load(g2), Fp29x2Ops::load(g2 + 16));
}
