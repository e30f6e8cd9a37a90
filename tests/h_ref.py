"""A big-int restatement of the Pinocchio prover's h (verifiable_mpc/trinocchio/pynocchio.py:203-225), deliberately by
the NAIVE route - interpolate V, W, Y, multiply, divide by t with remainder, add the zero-knowledge terms - so that it
shares nothing with the moment formula of csrc/bn256_qap_h.hip; that formula restated (moment_h); an O(d) test of a
claimed h at one random point, for degrees at which the restatements are too slow (h_identity_holds); and a builder of
random satisfiable sparse R1CS with their witnesses.  The independent side of tests/test_h_ref.py and
tests/test_gpu_pinocchio_h.py."""
import math
import random

import numpy as np

from tests import keygen_ref as K

N = K.N


def row_values(M, c):
    """dense rows or (row, col, value) entries -> the row values M c"""
    return [sum(int(x) * ci for x, ci in zip(r, c)) % N for r in M]


def entry_row_values(entries, d, c):
    out = [0] * d
    for r, col, x in entries:
        out[r] = (out[r] + x * c[col]) % N
    return out


def t_coeffs(d):
    t = [1]
    for j in range(1, d + 1):
        t = [((t[i - 1] if i else 0) - j * (t[i] if i < len(t) else 0)) % N for i in range(len(t) + 1)]
    return t


def interpolate_values(vals):
    """the coefficients (length d) of the polynomial of degree < d with P(j) = vals[j-1]: plain Lagrange, through
    keygen_ref.interpolate_columns (one column whose entry in row j is the value)"""
    d = len(vals)
    return K.interpolate_columns([(r, 0, int(v) % N) for r, v in enumerate(vals)], 1, d)[0]


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % N
    return out


def poly_divmod(p, t):
    """(quotient of len(p) - len(t) + 1 coefficients as the reference's div_polys keeps them, remainder) by monic t"""
    p = list(p)
    n = len(p) - len(t) + 1
    q = [0] * max(n, 0)
    for i in range(n - 1, -1, -1):
        f = p[i + len(t) - 1]
        q[i] = f
        if f:
            for k, x in enumerate(t):
                p[i + k] = (p[i + k] - f * x) % N
    return q, p[:len(t) - 1]


def naive_h(a, b, y, deltas=None):
    """(h, remainder): p = V W - Y from the interpolated row values (length 2d - 1, as compute_p_poly's), h = p / t of
    length d - 1; with deltas = (dv, dw, dy) the reference's zero-knowledge h of length d + 1:
    h + dv W + dw V + dv dw t - dy"""
    d = len(a)
    V, W, Y = interpolate_values(a), interpolate_values(b), interpolate_values(y)
    p = poly_mul(V, W)
    for i, x in enumerate(Y):
        p[i] = (p[i] - x) % N
    t = t_coeffs(d)
    h, rem = poly_divmod(p, t)
    if deltas is None:
        return h, rem
    dv, dw, dy = deltas
    out = [0] * (d + 1)
    for i, x in enumerate(h):
        out[i] = x
    for i in range(d):
        out[i] = (out[i] + dv * W[i] + dw * V[i]) % N
    for i in range(d + 1):
        out[i] = (out[i] + dv * dw % N * t[i]) % N
    out[0] = (out[0] - dy) % N
    return out, rem


def moment_h(a, b, deltas=None):
    """the formula the device uses, in big ints: length d + 1 with deltas, d - 1 without"""
    d = len(a)
    dv, dw, dy = deltas if deltas is not None else (0, 0, 0)
    t = t_coeffs(d)
    w = lambda j: (-1) ** (d - j) * math.factorial(j - 1) * math.factorial(d - j) % N
    u = [ai * pow(w(j), -1, N) % N for j, ai in enumerate(a, 1)]
    v = [bi * pow(w(j), -1, N) % N for j, bi in enumerate(b, 1)]
    A = [0] + [sum(x * pow(j, k - 1, N) for j, x in enumerate(u, 1)) % N for k in range(1, d + 1)]
    B = [0] + [sum(x * pow(j, k - 1, N) for j, x in enumerate(v, 1)) % N for k in range(1, d + 1)]
    C = [(sum(A[i] * B[k - i] for i in range(1, k)) + dv * B[k] + dw * A[k]) % N for k in range(d + 1)]
    h = [(sum(t[i] * C[i - e] for i in range(e + 1, d + 1)) + dv * dw * t[e] - (dy if e == 0 else 0)) % N
         for e in range(d + 1)]
    return h if deltas is not None else h[:max(d - 1, 0)]


def h_identity_holds(a, b, y, h, deltas=None, seed=0):
    """An O(d) test of a claimed h (ints, lowest coefficient first, any length) against the row values, for degrees at
    which moment_h is too slow: at one seeded random point r outside the nodes,
        h(r) t(r) == (V(r) + dv t(r)) (W(r) + dw t(r)) - (Y(r) + dy t(r)),     t(r) = prod_j (r - j),
    with V(r), W(r), Y(r) by barycentric evaluation of a, b, y at the nodes 1 .. d: P(r) = t(r) sum_j P(j) / (w_j (r - j)),
    w_j = prod_{k != j} (j - k) = (-1)^(d-j) (j-1)! (d-j)!.  Without deltas dv = dw = dy = 0.  Both sides are polynomials
    in r of degree at most 2 d, so a wrong h passes with probability at most 2 d / N.  The length of h is not tested."""
    d = len(a)
    dv, dw, dy = deltas if deltas is not None else (0, 0, 0)
    r = random.Random(seed).randrange(d + 1, N)
    fact = [1] * (d + 1)
    for j in range(1, d + 1):
        fact[j] = fact[j - 1] * j % N
    t = 1
    for j in range(1, d + 1):
        t = t * (r - j) % N
    inv = [pow((-1) ** (d - j) * fact[j - 1] * fact[d - j] * (r - j) % N, -1, N) for j in range(1, d + 1)]
    V, W, Y = (t * sum(int(v) * i for v, i in zip(vals, inv)) % N for vals in (a, b, y))
    hr = 0
    for x in reversed(h):
        hr = (hr * r + int(x)) % N
    return hr * t % N == ((V + dv * t) * (W + dw * t) - (Y + dy * t)) % N


def satisfiable_r1cs(d, seed, n_io=2, extra=3, zero_a=False, zero_b=False):
    """a random sparse R1CS of d constraints WITH a witness that satisfies it: rows of V and W with 1 to 3 random
    entries (values small, negative, or full size), a random witness, and row j of Y a single entry on a wire of
    non-zero value, set to a_j b_j / c_k.  zero_a / zero_b: V / W without entries (a = 0 / b = 0 everywhere).
    -> (V, W, Y as CSR tuples (row_ptr, col, list of ints), out_ix, m, witness as ints with c[0] = 1)"""
    rng = random.Random(seed)
    m = n_io + d + extra
    c = [1] + [rng.randrange(1, N) for _ in range(m)]

    def matrix(empty):
        ptr, col, vals = [0], [], []
        for _ in range(d):
            for _ in range(0 if empty else rng.randint(1, 3)):
                col.append(rng.randrange(0, m + 1))
                vals.append(rng.choice([rng.randint(-3, 3), rng.randrange(N), -rng.randrange(1 << 64)]))
            ptr.append(len(col))
        return ptr, col, vals
    V, W = matrix(zero_a), matrix(zero_b)

    def rows(M):
        ptr, col, vals = M
        return [sum(vals[e] * c[col[e]] for e in range(ptr[r], ptr[r + 1])) % N for r in range(d)]
    a, b = rows(V), rows(W)
    ycol = [rng.randrange(0, m + 1) for _ in range(d)]
    yval = [a[r] * b[r] % N * pow(c[ycol[r]], -1, N) % N for r in range(d)]
    Y = (list(range(d + 1)), ycol, yval)
    return V, W, Y, n_io, m, c


def csr_arrays(M):
    """a CSR tuple of Python lists -> the numpy form R1CSQAP takes (values as (nnz, 32) uint8 residues)"""
    ptr, col, vals = M
    v = K.to_array([x % N for x in vals]) if vals else np.zeros((0, 32), np.uint8)
    return np.asarray(ptr, np.int64), np.asarray(col, np.int64), v


def csr_row_values(M, c):
    ptr, col, vals = M
    return [sum(int(vals[e]) * c[col[e]] for e in range(ptr[r], ptr[r + 1])) % N for r in range(len(ptr) - 1)]
