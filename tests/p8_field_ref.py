"""Protocol 8 (AC20 circuit satisfiability) over ANY prime field, on Python ints: tests/p8_ref.py with the modulus as a
parameter, and the knowledge-of-exponent pivot (AC20 section 9) as scalar algebra under a known trapdoor.  The CPU
restatement that tests/test_gpu_p8_bn256_primitives.py and tests/test_gpu_circuit_sat_koe.py hold the GF(n) path
against; tests/test_p8_field_ref.py holds it against tests/p8_ref.py at p = l.

Circuits, z and the two routes (NAIVE: coefficient lists and double loops; BARYCENTRIC: factorial tables, correlation
with 1/k, prefix / suffix products, column sums) are those of tests/p8_ref.py.  `P8(p)` carries the modulus; the
knowledge-of-exponent part is at the end.
"""
import hashlib

ELL = 2**252 + 27742317777372353535851937790883648493
BN_N = 65000549695646603732796438742359905742570406053903786389881062969044166799969

CIRCUIT_TAG = {ELL: b"vmpc-ac20/p8/circuit/v1"}        # any other order: the tag of the BN-256 variant
CIRCUIT_TAG_BN = b"vmpc-ac20/p8/circuit/bn256/v1"
KOE_FIRST_TAG = b"vmpc-ac20/p8-koe/first/v1"
KOE_SECOND_TAG = b"vmpc-ac20/p8-koe/second/v1"


def _items(entries):
    return entries.items() if isinstance(entries, dict) else entries


class P8:
    def __init__(self, p):
        self.p = p

    def inv(self, a):
        return pow(a % self.p, self.p - 2, self.p)

    # ---- the circuit as data ---------------------------------------------------------------------------------------
    def canonical_rows(self, rows):
        p, out = self.p, []
        for entries, const in rows:
            acc = {}
            for c, v in _items(entries):
                acc[c] = (acc.get(c, 0) + v) % p
            out.append((sorted((c, v) for c, v in acc.items() if v), const % p))
        return out

    def circuit_digest(self, n_x, A, B, O):
        """tests/p8_ref.circuit_digest, the tag chosen by the order"""
        h = hashlib.sha256(CIRCUIT_TAG.get(self.p, CIRCUIT_TAG_BN))
        for v in (n_x, len(A), len(O)):
            h.update(v.to_bytes(8, "little"))
        for M in (A, B, O):
            rows = self.canonical_rows(M)
            ptr = [0]
            for e, _ in rows:
                ptr.append(ptr[-1] + len(e))
            h.update(len(rows).to_bytes(8, "little") + ptr[-1].to_bytes(8, "little"))
            h.update(b"".join(q.to_bytes(8, "little") for q in ptr))
            h.update(b"".join(c.to_bytes(8, "little") for e, _ in rows for c, _ in e))
            h.update(b"".join(v.to_bytes(32, "little") for e, _ in rows for _, v in e))
            h.update(b"".join(k.to_bytes(32, "little") for _, k in rows))
        return h.digest()

    def row_eval(self, row, n_x, x, gamma):
        entries, const = row
        s = const
        for c, v in _items(entries):
            s += v * (x[c] if c < n_x else gamma[c - n_x])
        return s % self.p

    def triples(self, n_x, A, B, x):
        m = len(A)
        a, b, gamma = [0] * m, [0] * m, [0] * m
        for i in range(m):
            a[i] = self.row_eval(A[i], n_x, x, gamma)
            b[i] = self.row_eval(B[i], n_x, x, gamma)
            gamma[i] = a[i] * b[i] % self.p
        return a, b, gamma

    # ---- naive route -----------------------------------------------------------------------------------------------
    def poly_mul(self, f, g):
        out = [0] * (len(f) + len(g) - 1)
        for i, a in enumerate(f):
            for j, b in enumerate(g):
                out[i + j] = (out[i + j] + a * b) % self.p
        return out

    def poly_eval(self, f, x):
        acc = 0
        for c in reversed(f):
            acc = (acc * x + c) % self.p
        return acc

    def interpolate(self, vals):
        """coefficients of the polynomial through (1, vals[0]), (2, vals[1]), .."""
        p, n = self.p, len(vals)
        out = [0] * n
        for i in range(1, n + 1):
            num, den = [1], 1
            for j in range(1, n + 1):
                if j != i:
                    num = self.poly_mul(num, [-j % p, 1])
                    den = den * (i - j) % p
            s = vals[i - 1] * self.inv(den) % p
            for k, c in enumerate(num):
                out[k] = (out[k] + c * s) % p
        return out

    def z_tail_naive(self, a, b, r_a, r_b):
        """[f(0), g(0), h(0), h(1), .., h(2m)]"""
        m = len(a)
        f, g = self.interpolate(a + [r_a]), self.interpolate(b + [r_b])
        h = self.poly_mul(f, g)
        return [self.poly_eval(f, 0), self.poly_eval(g, 0)] + [self.poly_eval(h, i) for i in range(2 * m + 1)]

    def lagrange_naive(self, K, c):
        p = self.p
        xs = list(range(K + 1))
        if c % p in xs:
            raise ZeroDivisionError("challenge on an interpolation node")
        out, prod = [], 1
        for j in xs:
            prod = prod * (c - j) % p
        for i in xs:
            d = 1
            for j in xs:
                if i != j:
                    d = d * (i - j) % p
            out.append(prod * self.inv((c - i) * d) % p)
        return out

    def forms_naive(self, n_x, n_in, A, B, O, c):
        """(F, G, H, [O_k]) as (dense coefficient list over z, constant)"""
        p, m = self.p, len(A)
        N = n_in + 3 + 2 * m

        def dense(row):
            entries, const = row
            v = [0] * N
            for col, val in _items(entries):
                pos = col if col < n_x else n_in + 3 + (col - n_x)
                v[pos] = (v[pos] + val) % p
            return v, const % p

        lam, lam2 = self.lagrange_naive(m, c), self.lagrange_naive(2 * m, c)
        out = []
        for wire, M in ((0, A), (1, B)):
            co, k = [0] * N, 0
            co[n_in + wire] = lam[0]
            for j in range(m):
                d, dc = dense(M[j])
                co = [(u + lam[j + 1] * w) % p for u, w in zip(co, d)]
                k = (k + lam[j + 1] * dc) % p
            out.append((co, k))
        out.append(([0] * (n_in + 2) + lam2, 0))
        return out[0], out[1], out[2], [dense(r) for r in O]

    # ---- barycentric / correlation route (what the kernels do) -------------------------------------------------------
    def tables(self, K):
        p = self.p
        fact = [1] * (K + 1)
        for k in range(1, K + 1):
            fact[k] = fact[k - 1] * k % p
        ifact = [0] * (K + 1)
        ifact[K] = self.inv(fact[K])
        for k in range(K, 0, -1):
            ifact[k - 1] = ifact[k] * k % p
        return fact, ifact

    def z_tail_bary(self, a, b, r_a, r_b):
        p, m = self.p, len(a)
        M = m + 1
        fact, ifact = self.tables(2 * m + 1)
        T = [0] + [fact[k - 1] * ifact[k] % p for k in range(1, 2 * m + 2)]
        w = [(-1) ** (M - j) * ifact[j - 1] * ifact[M - j] % p for j in range(1, M + 1)]
        uf = [v * wj % p for v, wj in zip(a + [r_a], w)]
        ug = [v * wj % p for v, wj in zip(b + [r_b], w)]
        l0 = (-1) ** (M + 1) * fact[M] % p
        f0 = l0 * sum(u * T[i + 1] for i, u in enumerate(uf)) % p
        g0 = l0 * sum(u * T[i + 1] for i, u in enumerate(ug)) % p
        h = [f0 * g0 % p] + [x * y % p for x, y in zip(a, b)]
        if m:
            h.append(r_a * r_b % p)
        for x in range(m + 2, 2 * m + 1):
            lx = fact[x - 1] * ifact[x - M - 1] % p
            sf = sum(uf[j - 1] * T[x - j] for j in range(1, M + 1))
            sg = sum(ug[j - 1] * T[x - j] for j in range(1, M + 1))
            h.append((lx * sf % p) * (lx * sg % p) % p)
        return [f0, g0] + h

    def lagrange_bary(self, K, c):
        p = self.p
        _, ifact = self.tables(max(K, 1))
        d = [(c - j) % p for j in range(K + 1)]
        pre, suf = [1] * (K + 2), [1] * (K + 2)
        for j in range(K + 1):
            pre[j + 1] = pre[j] * d[j] % p
        for j in range(K, -1, -1):
            suf[j] = suf[j + 1] * d[j] % p
        return [(-1) ** (K - j) * pre[j] * suf[j + 1] * ifact[j] * ifact[K - j] % p for j in range(K + 1)]

    def colsum(self, n_x, n_in, N, M, weights):
        """(coefficients over z, constant) of sum_i weights[i] * row i of M"""
        p = self.p
        co, k = [0] * N, 0
        for (entries, const), w in zip(M, weights):
            for col, val in _items(entries):
                pos = col if col < n_x else n_in + 3 + (col - n_x)
                co[pos] = (co[pos] + val * w) % p
            k = (k + const * w) % p
        return co, k

    def forms_bary(self, n_x, n_in, A, B, c):
        p, m = self.p, len(A)
        N = n_in + 3 + 2 * m
        lam, lam2 = self.lagrange_bary(m, c), self.lagrange_bary(2 * m, c)
        F, kf = self.colsum(n_x, n_in, N, A, lam[1:])
        G, kg = self.colsum(n_x, n_in, N, B, lam[1:])
        F[n_in] = (F[n_in] + lam[0]) % p
        G[n_in + 1] = (G[n_in + 1] + lam[0]) % p
        return (F, kf), (G, kg), ([0] * (n_in + 2) + lam2, 0)

    def dot(self, co, z):
        return sum(u * v for u, v in zip(co, z)) % self.p

    def combine(self, n_x, n_in, A, B, O, c, rho, y, outputs, route="bary"):
        """L = sum_k rho^k (O_k - out_k) + rho^n_out (F - y1) + rho^(n_out+1) (G - y2) + rho^(n_out+2) (H - y3)
        -> (coefficients, constant, (F, G, H))"""
        p, m, n_out = self.p, len(A), len(O)
        N = n_in + 3 + 2 * m
        if route == "bary":
            F, G, H = self.forms_bary(n_x, n_in, A, B, c)
            Oc, Ok = self.colsum(n_x, n_in, N, O, [pow(rho, k, p) for k in range(n_out)])
        else:
            F, G, H, Os = self.forms_naive(n_x, n_in, A, B, O, c)
            Oc, Ok = [0] * N, 0
            for k, (co, const) in enumerate(Os):
                Oc = [(u + pow(rho, k, p) * w) % p for u, w in zip(Oc, co)]
                Ok = (Ok + pow(rho, k, p) * const) % p
        const = (Ok - sum(pow(rho, k, p) * o for k, o in enumerate(outputs))) % p
        co = Oc
        for i, ((fc, fk), yi) in enumerate(zip((F, G, H), y)):
            pw = pow(rho, n_out + i, p)
            co = [(u + pw * w) % p for u, w in zip(co, fc)]
            const = (const + pw * (fk - yi)) % p
        return co, const, (F, G, H)

    # ---- the KoE variant's compact transcript ----------------------------------------------------------------------
    def koe_first_challenge(self, P_bytes, pi_bytes, digest, n_in):
        """(c, first digest): SHA-256(tag | P (64 B) | pi (128 B) | circuit digest | n_in u64 LE), c = digest LE mod p"""
        d = hashlib.sha256(KOE_FIRST_TAG + P_bytes + pi_bytes + digest + n_in.to_bytes(8, "little")).digest()
        return int.from_bytes(d, "little") % self.p, d

    def koe_second_challenge(self, first_digest, y, outputs):
        """rho: SHA-256(tag | first digest | y1, y2, y3 | n_out u32 LE | outputs), 32-byte LE residues"""
        d = hashlib.sha256(KOE_SECOND_TAG + first_digest + b"".join(v.to_bytes(32, "little") for v in y) +
                           len(outputs).to_bytes(4, "little") + b"".join(v.to_bytes(32, "little") for v in outputs)).digest()
        return int.from_bytes(d, "little") % self.p

    def witness(self, n_x, A, B, x, r_a, r_b, route="bary"):
        """(z, gamma): z = x + [f(0), g(0), h(0), h(1), .., h(2m)]"""
        a, b, gamma = self.triples(n_x, A, B, x)
        tail = (self.z_tail_bary if route == "bary" else self.z_tail_naive)(a, b, r_a, r_b)
        return [v % self.p for v in x] + tail, gamma

    def prove_koe(self, n_x, A, B, O, x, r_a, r_b, commit):
        """Protocol 8 of the KoE variant without the pivot.  commit(z) -> (P bytes, pi bytes)."""
        p, n_in = self.p, len(x)
        z, gamma = self.witness(n_x, A, B, x, r_a, r_b)
        c, d1 = self.koe_first_challenge(*commit(z), self.circuit_digest(n_x, A, B, O), n_in)
        outputs = [self.row_eval(r, n_x, x, gamma) for r in O]
        F, G, H = self.forms_bary(n_x, n_in, A, B, c)
        y = [(self.dot(co, z) + k) % p for co, k in (F, G, H)]
        assert y[0] * y[1] % p == y[2]
        rho = self.koe_second_challenge(d1, y, outputs)
        co, const, _ = self.combine(n_x, n_in, A, B, O, c, rho, y, outputs)
        assert (self.dot(co, z) + const) % p == 0
        return {"z": z, "gamma": gamma, "c": c, "y": y, "outputs": outputs, "rho": rho, "L": co, "L_const": const}

    # ---- random circuits (tests/p8_ref.random_circuit over this field) ----------------------------------------------
    def random_circuit(self, rng, n_x, m, n_out, width=3):
        p = self.p

        def coeff():
            r = rng.random()
            if r < 0.15:
                return -rng.randrange(1, 1 << 20)
            if r < 0.25:
                return rng.randrange(p, 1 << 300)
            return rng.randrange(1, p) if r < 0.6 else rng.randrange(1, 5)

        def row(i):
            if rng.random() < 0.1:
                return ({}, rng.randrange(p))
            e = {}
            for _ in range(rng.randrange(1, width + 1)):
                if n_x + i == 0:
                    break
                e[rng.randrange(n_x + i)] = coeff()
            return (e, rng.randrange(p) if rng.random() < 0.5 else 0)

        return [row(i) for i in range(m)], [row(i) for i in range(m)], [row(m) for _ in range(n_out)]


# ---- the knowledge-of-exponent pivot as scalars (knowledge_of_exponent.py:50-153) -----------------------------------
# Trapdoor (g_exp, alpha, s): pp_lhs[i] = g_exp s^(i+1) g1, pp_rhs[i] = g_exp alpha s^(i+1) g2, i < 2N.  Every proof
# element is a known multiple of g1 or g2, and a pairing equation is an identity between products of exponents mod n.
class KoeTrapdoor:
    def __init__(self, g_exp, alpha, s, p=BN_N):
        self.g_exp, self.alpha, self.s, self.p = g_exp % p, alpha % p, s % p, p

    def lhs_exp(self, i):
        return self.g_exp * pow(self.s, i + 1, self.p) % self.p

    def rhs_exp(self, i):
        return self.alpha * self.lhs_exp(i) % self.p

    def commitment(self, z, gamma):
        """(exponent of P over g1, exponent of pi over g2): gamma pp[0] + sum_i z_i pp[i + 1]"""
        e = sum(v * self.lhs_exp(i) for i, v in enumerate([gamma] + list(z))) % self.p
        return e, self.alpha * e % self.p

    def product(self, L, z, gamma):
        """c = (gamma, z_0, .., z_{N-1}) * (L_{N-1}, .., L_0): 2N coefficients; c[N] = <L, z>"""
        p = self.p
        lhs, rhs = [gamma] + list(z), list(reversed(L))
        c = [0] * (len(lhs) + len(rhs) - 1)
        for i, a in enumerate(lhs):
            for j, b in enumerate(rhs):
                c[i + j] = (c[i + j] + a * b) % p
        return c

    def opening(self, L, z, gamma):
        """(exponent of Q over g1, u_linear = <L, z>): Q = -sum_{i != N} c[i] pp_lhs[i]"""
        N, c = len(z), self.product(L, z, gamma)
        return -sum(v * self.lhs_exp(i) for i, v in enumerate(c) if i != N) % self.p, c[N]

    def opening_by_evaluation(self, L, z, gamma):
        """the same two values in O(N): with a(t) = gamma + sum z_i t^(i+1) and b(t) = sum_j L[N-1-j] t^j,
        sum_{i != N} c[i] s^i = a(s) b(s) - u s^N (what the O(N^2) product above states coefficient by coefficient)"""
        p, s, N = self.p, self.s, len(z)
        u = sum(a * b for a, b in zip(L, z)) % p
        a_s = (gamma + sum(v * pow(s, i + 1, p) for i, v in enumerate(z))) % p
        b_s = sum(v * pow(s, j, p) for j, v in enumerate(reversed(L))) % p
        return -self.g_exp * s * (a_s * b_s - u * pow(s, N, p)) % p, u

    def R_exp(self, L):
        """exponent over g2 of R = sum_j L[N-1-j] pp_rhs[j]"""
        return sum(v * self.rhs_exp(j) for j, v in enumerate(reversed(L))) % self.p

    def restriction_check(self, P_exp, pi_exp):
        """e(P, pp_rhs[0]) == e(pp_lhs[0], pi)"""
        return P_exp * self.rhs_exp(0) % self.p == self.lhs_exp(0) * pi_exp % self.p

    def prq_check(self, L, P_exp, Q_exp, u_linear):
        """e(P, R) e(Q, pp_rhs[0]) == e(pp_lhs[0], u pp_rhs[N])"""
        N = len(L)
        return (P_exp * self.R_exp(L) + Q_exp * self.rhs_exp(0) - self.lhs_exp(0) * u_linear * self.rhs_exp(N)) % self.p == 0


def to_csr(rows):
    ptr, col, vals, consts = [0], [], [], []
    for e, k in rows:
        for c, v in e.items():
            col.append(c)
            vals.append(v)
        ptr.append(len(col))
        consts.append(k)
    return ptr, col, vals, consts
