"""Big-integer restatement of the moment transform's subproduct-tree route (csrc/bn256_qap_mtree.hip, DESIGN.md section
26), independent of the library: leaves, tree, padding, Newton inverse, n_out on either side of d.

    A_k = sum_{j=1..d} u_j j^(k-1),   sum_{k>=0} A_(k+1) z^k = sum_j u_j / (1 - j z) = R(z) / D(z)

with N(x) = sum_j u_j prod_{i != j} (x - i), T(x) = prod_j (x - j), R and D their coefficients reversed."""
N = 65000549695646603732796438742359905742570406053903786389881062969044166799969      # BN-256's group order
S_MAX = 128


def moments(u, n_out):
    """the definition, by running powers: out[k] = sum_j u[j-1] j^k"""
    out, run = [], [x % N for x in u]
    for _ in range(n_out):
        out.append(sum(run) % N)
        run = [x * j % N for j, x in enumerate(run, 1)]
    return out


def geometry(d, s_max=S_MAX):
    """(s, L, d'): the smallest L with s = ceil(d / 2^L) <= s_max, d' = s 2^L"""
    L = 0
    while -(-d // (1 << L)) > s_max:
        L += 1
    s = -(-d // (1 << L))
    return s, L, s << L


def plan_scalars(d, n_max, s_max=S_MAX):
    """({level: scalar offset}, offset of D^-1, offset of the build's 2 n_max scalars, total) of the plan buffer: level l
    holds 2^(L-l) nodes of s 2^l + 1 coefficients"""
    s, L, dp = geometry(d, s_max)
    off, levels = 0, {}
    for l in range(L + 1):
        levels[l] = off
        off += dp + (1 << (L - l))
    return levels, off, off + n_max, off + 3 * n_max


def scratch_scalars(d, n_wit, s_max=S_MAX):
    return 4 * geometry(d, s_max)[2] * n_wit


def mul(a, b):
    o = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                o[i + j] = (o[i + j] + x * y) % N
    return o


def add(a, b):
    n = max(len(a), len(b))
    a, b = a + [0] * (n - len(a)), b + [0] * (n - len(b))
    return [(x + y) % N for x, y in zip(a, b)]


def inv_series(D, n):
    """D^-1 mod z^n for D(0) = 1 by Newton doubling: g <- g (2 - D g)"""
    g, k = [1], 1
    while k < n:
        k = min(2 * k, n)
        e = [(-x) % N for x in mul(D[:k], g)[:k]]
        e[0] = (e[0] + 2) % N
        g = mul(g, e)[:k]
    return g[:n]


def leaf(u, pts):
    """(T, N) of a leaf: synthetic division of T by (x - j), q_(i-1) = T_i + j q_i from the top"""
    T = [1]
    for j in pts:
        T = mul(T, [(-j) % N, 1])
    s = len(pts)
    acc = [0] * s
    for j in pts:
        q = [0] * s
        q[s - 1] = 1
        for i in range(s - 1, 0, -1):
            q[i - 1] = (T[i] + j * q[i]) % N
        acc = [(a + u[j - 1] * x) % N for a, x in zip(acc, q)]
    return T, acc


def tree_moments(u, n_out, s_max=S_MAX):
    """moments(u, n_out) by the tree -> (out, (s, L, d'))"""
    d = len(u)
    s, L, dp = geometry(d, s_max)
    u = [x % N for x in u] + [0] * (dp - d)
    Ts, Ns = zip(*(leaf(u, range(l * s + 1, l * s + s + 1)) for l in range(1 << L)))
    Ts, Ns = list(Ts), list(Ns)
    while len(Ts) > 1:
        Ns = [add(mul(Ns[i], Ts[i + 1]), mul(Ns[i + 1], Ts[i])) for i in range(0, len(Ts), 2)]
        Ts = [mul(Ts[i], Ts[i + 1]) for i in range(0, len(Ts), 2)]
    D = (Ts[0][::-1] + [0] * n_out)[:n_out]           # z^d' T(1 / z): constant term 1
    R = (Ns[0] + [0] * dp)[:dp][::-1][:n_out]         # z^(d'-1) N(1 / z), its low min(d', n_out) coefficients
    return mul(R, inv_series(D, n_out))[:n_out], (s, L, dp)
