"""Shamir sharing mod l on Python ints: the CPU restatement that tests/test_gpu_share_kernels.py and
tests/test_gpu_mpc_circuit_sat.py hold csrc/mpc_share.hip and verifiable_mpc_amd/mpc_circuit_sat.py against.

Party q < M holds the value of a polynomial at node q + 1; a secret is the value at 0.
    deal            degree-t shares of a value for M parties, from given higher coefficients
    weights         Lagrange coefficients at 0 of the nodes of some parties (ac20/recombine.py's double loop)
    mul_deal        what vmpc_fr_share_mul_deal_dev writes: out[q][i] = a_i b_i + sum_k coeffs[k-1][i] (q + 1)^k
    combine         what vmpc_fr_share_combine_dev writes: out[dst[i]] = sum_p weights[p] parts[p][i]
    extend_fg       f and g at 0 and m+2..2m, from tests/p8_ref.py's interpolation
"""
from tests import p8_ref as ref

ELL = ref.ELL


def deal(value, coeffs, parties):
    """[value + sum_k coeffs[k-1] (q + 1)^k for q < parties]"""
    return [(value + sum(c * pow(q + 1, k + 1, ELL) for k, c in enumerate(coeffs))) % ELL for q in range(parties)]


def weights(nodes, at=0):
    out = []
    for i, x_i in enumerate(nodes):
        num = den = 1
        for j, x_j in enumerate(nodes):
            if i != j:
                num = num * (at - x_j) % ELL
                den = den * (x_i - x_j) % ELL
        out.append(num * ref.inv(den) % ELL)
    return out


def recombine(shares, nodes=None, at=0):
    nodes = nodes or list(range(1, len(shares) + 1))
    return sum(w * s for w, s in zip(weights(nodes, at), shares)) % ELL


def mul_deal(a, b, coeffs, parties):
    """a, b (None: ones): n values; coeffs: t rows of n -> parties rows of n"""
    d = [(u * (b[i] if b is not None else 1)) % ELL for i, u in enumerate(a)]
    cols = [deal(d[i], [row[i] for row in coeffs], parties) for i in range(len(a))]
    return [[cols[i][q] for i in range(len(a))] for q in range(parties)]


def combine(parts, wts, dst=None, out=None):
    """out (a copy; default zeros of len n) with out[dst[i]] = sum_p wts[p] parts[p][i]"""
    n = len(parts[0])
    out = list(out) if out is not None else [0] * n
    for i in range(n):
        out[dst[i] if dst is not None else i] = sum(w * row[i] for w, row in zip(wts, parts)) % ELL
    return out


def extend_fg(a, b):
    """a, b: m + 1 values at the nodes 1..m+1 (the last: r_a, r_b) -> (f_out, g_out), each [v(0), v(m+2), .., v(2m)].
    Barycentric over tests/p8_ref.py's factorial tables: v(x) = l(x) sum_j v_j w_j / (x - j), with l(x) = prod_j (x - j)
    and w_j = (-1)^(M-j) / ((j-1)! (M-j)!); tests/test_share_ref.py holds it against p8_ref's coefficient route."""
    M = len(a)
    m = M - 1
    fact, ifact = ref.tables(2 * m + 1)
    T = [0] + [fact[k - 1] * ifact[k] % ELL for k in range(1, 2 * m + 2)]       # T[k] = 1 / k
    w = [(-1) ** (M - j) * ifact[j - 1] * ifact[M - j] % ELL for j in range(1, M + 1)]
    out = []
    for v in (a, b):
        u = [x * wj % ELL for x, wj in zip(v, w)]
        vals = []
        for x in [0] + list(range(m + 2, 2 * m + 1)):
            lx = 1
            for j in range(1, M + 1):
                lx = lx * (x - j) % ELL
            # 1 / (x - j) = T[x - j] for x > M >= j, and -T[j] at x = 0
            vals.append(lx * sum(uj * (T[x - j] if x else -T[j]) for j, uj in enumerate(u, 1)) % ELL)
        out.append(vals)
    return out[0], out[1]
