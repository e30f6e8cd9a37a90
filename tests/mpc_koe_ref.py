"""Pure-Python restatement of what verifiable_mpc_amd/mpc_koe.py does to scalars: Shamir shares
mod n, the BN-256 group order, the jointly made pp as its trapdoor, and the M-party opening of a public form as the
product of each party's share vector with the reversed form.  Python ints only; the points of a test are these exponents
times the generators (oracle/bn256_ref.py)."""
from tests import p8_field_ref as fref

N = fref.BN_N


def weights(M):
    """the Lagrange coefficients of the nodes 1..M at 0, mod n"""
    out = []
    for i in range(1, M + 1):
        num = den = 1
        for j in range(1, M + 1):
            if j != i:
                num = num * (-j) % N
                den = den * (i - j) % N
        out.append(num * pow(den, N - 2, N) % N)
    return out


def deal(values, t, M, rng):
    """degree-t Shamir shares of every value for the parties at the nodes 1..M: shares[p][i]"""
    polys = [[v % N] + [rng.randrange(N) for _ in range(t)] for v in values]
    return [[sum(c * pow(p + 1, k, N) for k, c in enumerate(poly)) % N for poly in polys] for p in range(M)]


def recombine(shares):
    """shares[p][i] of M parties -> the values"""
    w = weights(len(shares))
    return [sum(w[p] * shares[p][i] for p in range(len(shares))) % N for i in range(len(shares[0]))]


def joint_trapdoor(draws):
    """draws: every party's (g_exp, alpha, z), party 0 first -> the trapdoor of the pp after all the passes.  A pass
    multiplies element i by g_p z_p^(i+1) (alpha_p more on the twist), so the three components multiply."""
    g = a = z = 1
    for g_p, a_p, z_p in draws:
        g, a, z = g * g_p % N, a * a_p % N, z * z_p % N
    return fref.KoeTrapdoor(g, a, z)


def updated_exps(trap, g_exp, alpha, z, n_points):
    """(lhs, rhs) exponents of update_setup(pp under trap, g_exp, alpha, z), element by element as the pass makes them"""
    lhs = [trap.lhs_exp(i) * g_exp % N * pow(z, i + 1, N) % N for i in range(n_points)]
    rhs = [trap.rhs_exp(i) * g_exp % N * alpha % N * pow(z, i + 1, N) % N for i in range(n_points)]
    return lhs, rhs


def party_products(L, z_shares, gamma_shares):
    """every party's c^(p) = (gamma_p, z^(p)) * reversed(L), 2 len(L) coefficients each"""
    one = fref.KoeTrapdoor(1, 1, 1)
    return [one.product(L, z_p, g_p) for z_p, g_p in zip(z_shares, gamma_shares)]


def party_opening(trap, L, z_p, gamma_p):
    """(exponent of this party's Q_p over g1, its share of <L, z>)"""
    return trap.opening(L, z_p, gamma_p)


def joint_opening(trap, L, z_shares, gamma_shares):
    """(exponent of the recombined Q, the opened <L, z>) from the parties' local results"""
    w = weights(len(z_shares))
    parts = [party_opening(trap, L, z_p, g_p) for z_p, g_p in zip(z_shares, gamma_shares)]
    return sum(w[p] * q for p, (q, _) in enumerate(parts)) % N, sum(w[p] * u for p, (_, u) in enumerate(parts)) % N


def extend_fg(v):
    """the share form of Protocol 8's extension for ONE polynomial: v = (v_1, .., v_m, r) are the values at the nodes
    1..M, M = m + 1 -> [f(0), f(m+2), .., f(2m)] (max(m, 1) values), by the barycentric formula
    f(x) = l(x) sum_j w_j v_j / (x - j), w_j = (-1)^(M-j) / ((j-1)! (M-j)!), l(x) = prod_j (x - j).  O(m^2) products and
    O(m) inversions, so that the shapes of the arena tests (m = 600) have a reference."""
    M = len(v)
    m = M - 1
    fact = [1] * (M + 1)
    for k in range(1, M + 1):
        fact[k] = fact[k - 1] * k % N
    inv = [0] + [pow(k, N - 2, N) for k in range(1, 2 * M + 1)]          # 1 / k for every difference that occurs
    u = [v[j - 1] * pow((-1) ** (M - j) * fact[j - 1] * fact[M - j], N - 2, N) % N for j in range(1, M + 1)]
    out = []
    for x in [0] + list(range(m + 2, 2 * m + 1)):
        ell, acc = 1, 0
        for j in range(1, M + 1):
            ell = ell * (x - j) % N
            acc += u[j - 1] * (inv[x - j] if x else -inv[j])
        out.append(ell * acc % N)
    return out
