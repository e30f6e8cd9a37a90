"""Shamir sharing mod n (the BN-256 group order) on Python ints: the CPU restatement that
tests/test_gpu_bn256_share_kernels.py and tests/test_gpu_trinocchio.py hold csrc/mpc_share.hip's GF(n) entries,
vmpc_bn256_qap_residual_dev and verifiable_mpc_amd/trinocchio.py against.  tests/share_ref.py is the same over GF(l).

Party q < M holds the value of a polynomial at node q + 1; a secret is the value at 0.
    deal            degree-t shares of a value for M parties, from given higher coefficients
    weights         Lagrange coefficients at 0 of the nodes 1..M (or of given nodes)
    recombine       the secret of M shares
    mul_deal        what vmpc_bn256_fr_share_mul_deal_dev writes: out[q][i] = a_i b_i + sum_k coeffs[k-1][i] (q + 1)^k
    combine         what vmpc_bn256_fr_share_combine_dev writes: out[dst[i]] = addend[i] + sum_p weights[p] parts[p][i]
    residual        what vmpc_bn256_qap_residual_dev writes: sum_j rho^j (a_j b_j - y_j), j from 0
    share_vector    degree-t shares of a list of values -> M lists
"""
from tests import h_ref as H

N = H.N


def deal(value, coeffs, parties):
    return [(value + sum(c * pow(q + 1, k + 1, N) for k, c in enumerate(coeffs))) % N for q in range(parties)]


def weights(nodes, at=0):
    out = []
    for i, x_i in enumerate(nodes):
        num = den = 1
        for j, x_j in enumerate(nodes):
            if i != j:
                num = num * (at - x_j) % N
                den = den * (x_i - x_j) % N
        out.append(num * pow(den, -1, N) % N)
    return out


def recombine(shares, nodes=None):
    nodes = nodes or list(range(1, len(shares) + 1))
    return sum(w * s for w, s in zip(weights(nodes), shares)) % N


def mul_deal(a, b, coeffs, parties):
    """a, b (None: ones): n values; coeffs: t rows of n -> parties rows of n"""
    d = [(u * (b[i] if b is not None else 1)) % N for i, u in enumerate(a)]
    cols = [deal(d[i], [row[i] for row in coeffs], parties) for i in range(len(a))]
    return [[cols[i][q] for i in range(len(a))] for q in range(parties)]


def combine(parts, wts, dst=None, out=None, addend=None):
    """out (a copy; default zeros of len n) with out[dst[i]] = addend[i] + sum_p wts[p] parts[p][i]"""
    n = len(parts[0])
    out = list(out) if out is not None else [0] * n
    for i in range(n):
        out[dst[i] if dst is not None else i] = ((addend[i] if addend is not None else 0)
                                                 + sum(w * row[i] for w, row in zip(wts, parts))) % N
    return out


def residual(a, b, y, rho):
    acc, pw = 0, 1
    for ai, bi, yi in zip(a, b, y):
        acc = (acc + pw * (ai * bi - yi)) % N
        pw = pw * rho % N
    return acc


def share_vector(values, t, parties, rng):
    """-> shares[p][i] of values[i], fresh degree-t polynomials from rng"""
    cols = [deal(v % N, [rng.randrange(N) for _ in range(t)], parties) for v in values]
    return [[col[p] for col in cols] for p in range(parties)]


def interpolate(vals):
    """the d coefficients of the polynomial of degree < d with P(j) = vals[j-1], in O(d^2): sum_j (vals_j / t'(j))
    t(x) / (x - j), each quotient by synthetic division (tests/h_ref.py's interpolate_values is cubic; tests/
    test_trinocchio_ref.py holds the two against each other)"""
    d = len(vals)
    t = H.t_coeffs(d)
    out = [0] * d
    for j, v in enumerate(vals, 1):
        if v % N == 0:
            continue
        q = [0] * d                          # t / (x - j): q_(d-1) = 1, q_(k-1) = t_k + j q_k
        acc = 0
        for k in range(d, 0, -1):
            acc = (t[k] + j * acc) % N
            q[k - 1] = acc
        w = 1                                # t'(j) = q(j)
        for i in range(1, d + 1):
            if i != j:
                w = w * (j - i) % N
        f = v * pow(w, -1, N) % N
        for k in range(d):
            out[k] = (out[k] + f * q[k]) % N
    return out


def quotient_parts(a, b, y):
    """(h, remainder, V, W, t): V W - Y divided by t for ANY row values, through h_ref's poly_mul and poly_divmod, with
    the quadratic interpolation above; h has d - 1 coefficients"""
    d = len(a)
    V, W, Y = interpolate(a), interpolate(b), interpolate(y)
    p = H.poly_mul(V, W)
    for i, x in enumerate(Y):
        p[i] = (p[i] - x) % N
    t = H.t_coeffs(d)
    h, rem = H.poly_divmod(p, t)
    return h, rem, V, W, t


def add_zk(h, V, W, t, deltas):
    """the zero-knowledge h of length d + 1: h + dv W + dw V + dv dw t - dy (h_ref.naive_h's second half)"""
    d = len(V)
    dv, dw, dy = deltas
    out = [0] * (d + 1)
    for i, x in enumerate(h):
        out[i] = x
    for i in range(d):
        out[i] = (out[i] + dv * W[i] + dw * V[i]) % N
    for i in range(d + 1):
        out[i] = (out[i] + dv * dw % N * t[i]) % N
    out[0] = (out[0] - dy) % N
    return out


def quotient(a, b, y, deltas=None):
    """(h, remainder) as h_ref.naive_h gives them"""
    h, rem, V, W, t = quotient_parts(a, b, y)
    return (h if deltas is None else add_zk(h, V, W, t, deltas)), rem
