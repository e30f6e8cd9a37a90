"""Test helper: the BN-256 optimal-ate pairing restated with Python big ints (NOT the product).

What the reference computes (verifiable_mpc/ac20/pairing.py):
    :55-62     xi = i + 3 and the Frobenius constants xi^(k(p-1)/6)
    :100-370   the tower Fp6 = Fp2[tau]/(tau^3 - xi), Fp12 = Fp6[w]/(w^2 - tau)
    :503-554   the Miller loop over the NAF of 6u+2, then the lines through pi(Q) and -pi^2(Q)
    :557-611   the final exponentiation (easy part, then the hard part of Algorithm 31 of eprint 2010/354)
    :614-643   optimal_ate(Q, P): either point at infinity gives 1
and trinocchio/pynocchio.py:67-72: pairing(a, b) = optimal_ate(b, a), G1 argument first.

This file states the same map from its definition, in a different shape on purpose, so that it does not
share formulas with the reference or with csrc/bn256_pairing.h:
  * Fp12 is held as a polynomial c_0 + c_1 w + ... + c_5 w^5 over Fp2 with w^6 = xi (the tower is the same
    field: tau = w^2);
  * the twist point Q is untwisted into E(Fp12) by (x, y) -> (x w^2, y w^3), and the Miller loop runs in
    AFFINE coordinates there, every line evaluated as (y_P - y_T) - lambda (x_P - x_T) with lambda in Fp12;
  * pi is the p-power map on coordinates, computed by exponentiation;
  * the final exponentiation is the plain power f^((p^12 - 1) / N).
A Miller-loop value here and one made with projective lines differ by a factor in Fp6, which the final
exponentiation removes; the reduced pairing values are equal coefficient for coefficient.

GT values are exchanged as 12 ints in the order of include/vmpc.h (the reference's own nesting):
    [x.x, x.y, x.z, y.x, y.y, y.z] of f = x w + y, x = x.x tau^2 + x.y tau + x.z, each Fp2 as (re, im).
"""
from oracle.bn256_ref import E1, E2, Fp2, G1, G2, N, P, U, XI

# ---- Fp12 = Fp2[w]/(w^6 - xi) -------------------------------------------------------------------------------

ZERO12 = (Fp2.zero,) * 6
ONE12 = (Fp2.one,) + (Fp2.zero,) * 5


def f12_add(a, b):
    return tuple(Fp2.add(x, y) for x, y in zip(a, b))


def f12_sub(a, b):
    return tuple(Fp2.sub(x, y) for x, y in zip(a, b))


def f12_mul(a, b):
    acc = [(0, 0)] * 11
    for i, x in enumerate(a):
        if x == (0, 0):
            continue
        for j, y in enumerate(b):
            if y == (0, 0):
                continue
            acc[i + j] = Fp2.add(acc[i + j], Fp2.mul(x, y))
    return tuple(Fp2.add(acc[k], Fp2.mul(XI, acc[k + 6])) if k < 5 else acc[k] for k in range(6))


def f12_pow(a, e):
    r = ONE12
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def _f6_inv(d0, d1, d2):
    """(d0 + d1 tau + d2 tau^2)^-1 in Fp2[tau]/(tau^3 - xi), by the adjugate of the multiplication matrix"""
    m = Fp2.mul
    a = Fp2.sub(m(d0, d0), m(XI, m(d1, d2)))
    b = Fp2.sub(m(XI, m(d2, d2)), m(d0, d1))
    c = Fp2.sub(m(d1, d1), m(d0, d2))
    det = Fp2.add(m(d0, a), m(XI, Fp2.add(m(d2, b), m(d1, c))))
    di = Fp2.inv(det)
    return m(a, di), m(b, di), m(c, di)


def f12_inv(a):
    """a(w)^-1 = a(-w) / (a(w) a(-w)); the norm a(w) a(-w) is even in w, i.e. lies in Fp6 = Fp2[w^2]"""
    conj = tuple(x if k % 2 == 0 else Fp2.neg(x) for k, x in enumerate(a))
    n = f12_mul(a, conj)
    assert n[1] == n[3] == n[5] == Fp2.zero
    i0, i1, i2 = _f6_inv(n[0], n[2], n[4])
    return f12_mul(conj, (i0, Fp2.zero, i1, Fp2.zero, i2, Fp2.zero))


def f12_frob(a, k=1):
    return f12_pow(a, P ** k)


def f12_from_fp2(x, k=0):
    """x w^k"""
    out = [Fp2.zero] * 6
    out[k] = x
    return tuple(out)


# ---- exchange order of include/vmpc.h ------------------------------------------------------------------------
# f = x w + y; x = x.x tau^2 + x.y tau + x.z; y = y.x tau^2 + y.y tau + y.z; tau = w^2
#   -> w-powers: x.x w^5, x.y w^3, x.z w, y.x w^4, y.y w^2, y.z w^0
_ORDER = (5, 3, 1, 4, 2, 0)


def to_gt(a):
    out = []
    for k in _ORDER:
        out += [a[k][0] % P, a[k][1] % P]
    return tuple(out)


def from_gt(v):
    c = [None] * 6
    for slot, k in enumerate(_ORDER):
        c[k] = (v[2 * slot] % P, v[2 * slot + 1] % P)
    return tuple(c)


GT_ONE = to_gt(ONE12)

# ---- the Miller loop in E(Fp12) --------------------------------------------------------------------------------


def _untwist(q):
    (x, y) = q
    return (f12_from_fp2(x, 2), f12_from_fp2(y, 3))


def _line(t, r, p12):
    """line through t and r (tangent if t == r) evaluated at p12, and t + r; all in E(Fp12), affine"""
    (xt, yt), (xr, yr) = t, r
    if t == r:
        num = f12_mul(f12_from_fp2((3, 0)), f12_mul(xt, xt))
        den = f12_add(yt, yt)
    else:
        num, den = f12_sub(yr, yt), f12_sub(xr, xt)
    lam = f12_mul(num, f12_inv(den))
    xp, yp = p12
    line = f12_sub(f12_sub(yp, yt), f12_mul(lam, f12_sub(xp, xt)))
    x3 = f12_sub(f12_sub(f12_mul(lam, lam), xt), xr)
    y3 = f12_sub(f12_mul(lam, f12_sub(xt, x3)), yt)
    return line, (x3, y3)


def naf(k):
    """non-adjacent form, least significant digit first"""
    out = []
    while k > 0:
        if k & 1:
            d = 2 - (k & 3)
            k -= d
        else:
            d = 0
        out.append(d)
        k >>= 1
    return out


NAF_6U2 = naf(6 * U + 2)


def miller(p, q):
    """f_{6u+2,Q}(P) l_{[6u+2]Q, pi(Q)}(P) l_{.., -pi^2(Q)}(P), P in G1, Q on the twist (affine, finite)"""
    p12 = (f12_from_fp2((p[0], 0)), f12_from_fp2((p[1], 0)))
    q12 = _untwist(q)
    mq12 = (q12[0], f12_sub(ZERO12, q12[1]))
    f, t = ONE12, q12
    for d in reversed(NAF_6U2[:-1]):
        line, t = _line(t, t, p12)
        f = f12_mul(f12_mul(f, f), line)
        if d:
            line, t = _line(t, q12 if d == 1 else mq12, p12)
            f = f12_mul(f, line)
    q1 = (f12_frob(q12[0]), f12_frob(q12[1]))
    q2 = (f12_frob(q12[0], 2), f12_sub(ZERO12, f12_frob(q12[1], 2)))
    line, t = _line(t, q1, p12)
    f = f12_mul(f, line)
    line, t = _line(t, q2, p12)
    return f12_mul(f, line)


FINAL_EXP = (P ** 12 - 1) // N


def final_exp(f):
    return f12_pow(f, FINAL_EXP)


def pairing(p, q):
    """e(P, Q) for P in G1 (affine (x, y) ints, None = infinity) and Q on the twist (((x.re, x.im), (y.re, y.im)),
    None = infinity), in the argument order of pynocchio.pairing; -> 12 ints (to_gt order)"""
    if p is None or q is None:
        return GT_ONE
    return to_gt(final_exp(miller(p, q)))


def gt_mul(a, b):
    return to_gt(f12_mul(from_gt(a), from_gt(b)))


def gt_pow(a, e):
    return to_gt(f12_pow(from_gt(a), e))


__all__ = ["E1", "E2", "G1", "G2", "N", "P", "GT_ONE", "pairing", "miller", "final_exp", "gt_mul", "gt_pow",
           "to_gt", "from_gt", "f12_mul", "f12_inv", "f12_frob", "NAF_6U2"]
