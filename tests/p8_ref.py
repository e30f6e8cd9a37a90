"""Protocol 8 (AC20 circuit satisfiability, excluding the pivot) for a sparse circuit on Python ints: the CPU
restatement that tests/test_gpu_circuit_sat.py holds verifiable_mpc_amd.circuit_sat_gpu against.

A circuit is three row lists over the columns (x_0..x_{n_x-1}, gamma_0..gamma_{m-1}):
    A[i], B[i]  = ({col: coefficient}, constant)   left / right wire of multiplication gate i (reads gamma_j, j < i only)
    O[k]        = ({col: coefficient}, constant)   output k
z = x (n_in >= n_x values: trailing ones are padding no form reads) + [f(0), g(0), h(0)] + [h(1), .., h(2m)], where f
runs through (j, a_j), j = 1..m, and (m + 1, r_a), g alike, h = f g.  m = 0: f and g are the constants r_a, r_b and
z = x + [r_a, r_b, r_a r_b].

Where it matters there are two routes: the NAIVE one (coefficient lists, the double loop of ac20/recombine.py, forms
row by row) and the BARYCENTRIC one the kernels use (factorial tables, correlation with 1/k, prefix / suffix products,
column sums).  tests/test_p8_ref.py holds them together.
"""
import hashlib

ELL = 2**252 + 27742317777372353535851937790883648493


def inv(a):
    return pow(a % ELL, ELL - 2, ELL)


# ---- the circuit as data ------------------------------------------------------------------------------------------------
def canonical_rows(rows):
    """[(sorted [(col, value mod l)] without zeros, duplicates added, constant mod l)]"""
    out = []
    for entries, const in rows:
        acc = {}
        for c, v in (entries.items() if isinstance(entries, dict) else entries):
            acc[c] = (acc.get(c, 0) + v) % ELL
        out.append((sorted((c, v) for c, v in acc.items() if v), const % ELL))
    return out


def circuit_digest(n_x, A, B, O):
    """SHA-256 over the canonical CSR bytes:  b"vmpc-ac20/p8/circuit/v1" | n_x, m, n_out (u64 LE each) | for A, B, O:
    rows u64, nnz u64, row_ptr (rows + 1 u64), cols (u64 each), values (32 B LE each), constants (32 B LE each)"""
    h = hashlib.sha256(b"vmpc-ac20/p8/circuit/v1")
    for v in (n_x, len(A), len(O)):
        h.update(v.to_bytes(8, "little"))
    for M in (A, B, O):
        rows = canonical_rows(M)
        ptr = [0]
        for e, _ in rows:
            ptr.append(ptr[-1] + len(e))
        h.update(len(rows).to_bytes(8, "little") + ptr[-1].to_bytes(8, "little"))
        h.update(b"".join(p.to_bytes(8, "little") for p in ptr))
        h.update(b"".join(c.to_bytes(8, "little") for e, _ in rows for c, _ in e))
        h.update(b"".join(v.to_bytes(32, "little") for e, _ in rows for _, v in e))
        h.update(b"".join(k.to_bytes(32, "little") for _, k in rows))
    return h.digest()


def row_eval(row, n_x, x, gamma):
    entries, const = row
    s = const
    for c, v in (entries.items() if isinstance(entries, dict) else entries):
        s += v * (x[c] if c < n_x else gamma[c - n_x])
    return s % ELL


def triples(n_x, A, B, x):
    m = len(A)
    a, b, gamma = [0] * m, [0] * m, [0] * m
    for i in range(m):
        a[i] = row_eval(A[i], n_x, x, gamma)
        b[i] = row_eval(B[i], n_x, x, gamma)
        gamma[i] = a[i] * b[i] % ELL
    return a, b, gamma


# ---- naive route ----------------------------------------------------------------------------------------------------------
def poly_mul(p, q):
    out = [0] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] = (out[i + j] + a * b) % ELL
    return out


def poly_eval(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % ELL
    return acc


def interpolate(vals):
    """coefficients of the polynomial through (1, vals[0]), (2, vals[1]), .. (qap_creator.lagrange_interp_ff)"""
    n = len(vals)
    out = [0] * n
    for i in range(1, n + 1):
        num, den = [1], 1
        for j in range(1, n + 1):
            if j != i:
                num = poly_mul(num, [-j % ELL, 1])
                den = den * (i - j) % ELL
        s = vals[i - 1] * inv(den) % ELL
        for k, c in enumerate(num):
            out[k] = (out[k] + c * s) % ELL
    return out


def z_tail_naive(a, b, r_a, r_b):
    """[f(0), g(0), h(0), h(1), .., h(2m)]"""
    m = len(a)
    f, g = interpolate(a + [r_a]), interpolate(b + [r_b])
    h = poly_mul(f, g)
    return [poly_eval(f, 0), poly_eval(g, 0)] + [poly_eval(h, i) for i in range(2 * m + 1)]


def lagrange_naive(K, c):
    """recombination vector of the nodes 0..K at c (ac20/recombine.py:5-32); c on a node divides by zero there"""
    xs = list(range(K + 1))
    if c % ELL in xs:
        raise ZeroDivisionError("challenge on an interpolation node")
    out = []
    p = 1
    for j in xs:
        p = p * (c - j) % ELL
    for i in xs:
        d = 1
        for j in xs:
            if i != j:
                d = d * (i - j) % ELL
        out.append(p * inv((c - i) * d) % ELL)
    return out


def forms_naive(n_x, n_in, A, B, O, c):
    """(F, G, H, [O_k]) as (dense coefficient list over z, constant)"""
    m = len(A)
    N = n_in + 3 + 2 * m

    def dense(row):
        entries, const = row
        v = [0] * N
        for col, val in (entries.items() if isinstance(entries, dict) else entries):
            pos = col if col < n_x else n_in + 3 + (col - n_x)
            v[pos] = (v[pos] + val) % ELL
        return v, const % ELL

    lam, lam2 = lagrange_naive(m, c), lagrange_naive(2 * m, c)
    out = []
    for wire, M in ((0, A), (1, B)):
        co, k = [0] * N, 0
        co[n_in + wire] = lam[0]
        for j in range(m):
            d, dc = dense(M[j])
            co = [(u + lam[j + 1] * w) % ELL for u, w in zip(co, d)]
            k = (k + lam[j + 1] * dc) % ELL
        out.append((co, k))
    out.append(([0] * (n_in + 2) + lam2, 0))
    return out[0], out[1], out[2], [dense(r) for r in O]


# ---- barycentric / correlation route (what the kernels do) -------------------------------------------------------------
def tables(K):
    fact = [1] * (K + 1)
    for k in range(1, K + 1):
        fact[k] = fact[k - 1] * k % ELL
    ifact = [0] * (K + 1)
    ifact[K] = inv(fact[K])
    for k in range(K, 0, -1):
        ifact[k - 1] = ifact[k] * k % ELL
    return fact, ifact


def convolve(u, t):
    """the exact integer product of two coefficient lists by Kronecker substitution (66-byte slots: up to 2^22 terms
    of 506 bits): what makes the correlation affordable on the host at m = 32000"""
    SL = 66
    U = int.from_bytes(b"".join(v.to_bytes(SL, "little") for v in u), "little")
    V = int.from_bytes(b"".join(v.to_bytes(SL, "little") for v in t), "little")
    raw = (U * V).to_bytes(SL * (len(u) + len(t)), "little")
    return [int.from_bytes(raw[i * SL:(i + 1) * SL], "little") for i in range(len(u) + len(t) - 1)]


def z_tail_bary(a, b, r_a, r_b, kronecker=None):
    m = len(a)
    M = m + 1
    fact, ifact = tables(2 * m + 1)
    T = [0] + [fact[k - 1] * ifact[k] % ELL for k in range(1, 2 * m + 2)]
    w = [(-1) ** (M - j) * ifact[j - 1] * ifact[M - j] % ELL for j in range(1, M + 1)]
    uf = [v * wj % ELL for v, wj in zip(a + [r_a], w)]
    ug = [v * wj % ELL for v, wj in zip(b + [r_b], w)]
    l0 = (-1) ** (M + 1) * fact[M] % ELL
    f0 = l0 * sum(u * T[i + 1] for i, u in enumerate(uf)) % ELL
    g0 = l0 * sum(u * T[i + 1] for i, u in enumerate(ug)) % ELL
    h = [f0 * g0 % ELL] + [x * y % ELL for x, y in zip(a, b)]
    if m:
        h.append(r_a * r_b % ELL)
    if kronecker is None:
        kronecker = m >= 512
    if kronecker:       # sum_j u_j T[x - j] is coefficient x - 1 of (sum_i u_(i+1) t^i) (sum_k T[k] t^k)
        cf, cg = convolve(uf, T), convolve(ug, T)
    for x in range(m + 2, 2 * m + 1):
        lx = fact[x - 1] * ifact[x - M - 1] % ELL
        if kronecker:
            sf, sg = cf[x - 1], cg[x - 1]
        else:
            sf = sum(uf[j - 1] * T[x - j] for j in range(1, M + 1))
            sg = sum(ug[j - 1] * T[x - j] for j in range(1, M + 1))
        h.append((lx * sf % ELL) * (lx * sg % ELL) % ELL)
    return [f0, g0] + h


def lagrange_bary(K, c):
    _, ifact = tables(max(K, 1))
    d = [(c - j) % ELL for j in range(K + 1)]
    pre, suf = [1] * (K + 2), [1] * (K + 2)
    for j in range(K + 1):
        pre[j + 1] = pre[j] * d[j] % ELL
    for j in range(K, -1, -1):
        suf[j] = suf[j + 1] * d[j] % ELL
    return [(-1) ** (K - j) * pre[j] * suf[j + 1] * ifact[j] * ifact[K - j] % ELL for j in range(K + 1)]


def colsum(n_x, n_in, N, M, weights):
    """(coefficients over z, constant) of sum_i weights[i] * row i of M"""
    co, k = [0] * N, 0
    for (entries, const), w in zip(M, weights):
        for col, val in (entries.items() if isinstance(entries, dict) else entries):
            pos = col if col < n_x else n_in + 3 + (col - n_x)
            co[pos] = (co[pos] + val * w) % ELL
        k = (k + const * w) % ELL
    return co, k


def forms_bary(n_x, n_in, A, B, c):
    m = len(A)
    N = n_in + 3 + 2 * m
    lam, lam2 = lagrange_bary(m, c), lagrange_bary(2 * m, c)
    F, kf = colsum(n_x, n_in, N, A, lam[1:])
    G, kg = colsum(n_x, n_in, N, B, lam[1:])
    F[n_in] = (F[n_in] + lam[0]) % ELL
    G[n_in + 1] = (G[n_in + 1] + lam[0]) % ELL
    return (F, kf), (G, kg), ([0] * (n_in + 2) + lam2, 0)


# ---- compact transcript -------------------------------------------------------------------------------------------------
def first_challenge(commitment_wire, digest, n_in):
    """(c, first digest): SHA-256(b"vmpc-ac20/p8/first/v1" | [z] as 32 bytes (RFC 8032) | circuit digest | n_in u64)"""
    d = hashlib.sha256(b"vmpc-ac20/p8/first/v1" + commitment_wire + digest + n_in.to_bytes(8, "little")).digest()
    return int.from_bytes(d, "little") % ELL, d


def second_challenge(first_digest, y1, y2, y3, outputs):
    """rho: SHA-256(b"vmpc-ac20/p8/second/v1" | first digest | y1, y2, y3 | n_out u32 | outputs), 32-byte LE residues"""
    d = hashlib.sha256(b"vmpc-ac20/p8/second/v1" + first_digest + b"".join(v.to_bytes(32, "little") for v in (y1, y2, y3)) +
                       len(outputs).to_bytes(4, "little") + b"".join(v.to_bytes(32, "little") for v in outputs)).digest()
    return int.from_bytes(d, "little") % ELL


def dot(co, z):
    return sum(u * v for u, v in zip(co, z)) % ELL


def combine(n_x, n_in, A, B, O, c, rho, y, outputs, route="bary"):
    """L = sum_k rho^k (O_k - out_k) + rho^n_out (F - y1) + rho^(n_out+1) (G - y2) + rho^(n_out+2) (H - y3)
    -> (coefficients, constant, (F, G, H))"""
    m, n_out = len(A), len(O)
    N = n_in + 3 + 2 * m
    if route == "bary":
        F, G, H = forms_bary(n_x, n_in, A, B, c)
        Oc, Ok = colsum(n_x, n_in, N, O, [pow(rho, k, ELL) for k in range(n_out)])
    else:
        F, G, H, Os = forms_naive(n_x, n_in, A, B, O, c)
        Oc, Ok = [0] * N, 0
        for k, (co, const) in enumerate(Os):
            Oc = [(u + pow(rho, k, ELL) * w) % ELL for u, w in zip(Oc, co)]
            Ok = (Ok + pow(rho, k, ELL) * const) % ELL
    const = (Ok - sum(pow(rho, k, ELL) * o for k, o in enumerate(outputs))) % ELL
    co = Oc
    for i, ((fc, fk), yi) in enumerate(zip((F, G, H), y)):
        p = pow(rho, n_out + i, ELL)
        co = [(u + p * w) % ELL for u, w in zip(co, fc)]
        const = (const + p * (fk - yi)) % ELL
    return co, const, (F, G, H)


def prove(n_x, A, B, O, x, r_a, r_b, commit, route="bary", c_override=None):
    """Protocol 8 without the pivot.  commit(z) -> the 32-byte wire form of [z].  Returns a dict of everything."""
    n_in = len(x)
    a, b, gamma = triples(n_x, A, B, x)
    tail = (z_tail_bary if route == "bary" else z_tail_naive)(a, b, r_a, r_b)
    z = [v % ELL for v in x] + tail
    cw = commit(z)
    c, d1 = first_challenge(cw, circuit_digest(n_x, A, B, O), n_in)
    if c_override is not None:
        c = c_override
    outputs = [row_eval(r, n_x, x, gamma) for r in O]
    F, G, H = forms_bary(n_x, n_in, A, B, c) if route == "bary" else forms_naive(n_x, n_in, A, B, O, c)[:3]
    y = [(dot(co, z) + k) % ELL for co, k in (F, G, H)]
    assert y[0] * y[1] % ELL == y[2]
    rho = second_challenge(d1, y[0], y[1], y[2], outputs)
    co, const, _ = combine(n_x, n_in, A, B, O, c, rho, y, outputs, route)
    assert (dot(co, z) + const) % ELL == 0
    lam = (lagrange_bary if route == "bary" else lagrange_naive)
    return {"a": a, "b": b, "gamma": gamma, "z": z, "c": c, "y": y, "outputs": outputs, "rho": rho, "L": co,
            "L_const": const, "F": F, "G": G, "H": H, "lambda_m": lam(len(A), c), "lambda_2m": lam(2 * len(A), c)}


# ---- random circuits the reference convention accepts --------------------------------------------------------------------
def random_circuit(rng, n_x, m, n_out, width=3, long_col=None, empty_rows=True, wild=True):
    """forms over the inputs and EARLIER gammas only.  long_col: a column that more than 64 rows read.  wild: some
    negative and some oversized coefficients.  empty_rows: some rows with no entries (constant wires)."""
    def coeff():
        r = rng.random()
        if wild and r < 0.15:
            return -rng.randrange(1, 1 << 20)
        if wild and r < 0.25:
            return rng.randrange(ELL, 1 << 300)
        return rng.randrange(1, ELL) if r < 0.6 else rng.randrange(1, 5)

    def row(i, limit):
        if empty_rows and rng.random() < 0.1:
            return ({}, rng.randrange(ELL))
        e = {}
        for _ in range(rng.randrange(1, width + 1)):
            hi = n_x + min(i, limit)
            if hi == 0:
                break
            e[rng.randrange(hi)] = coeff()
        if long_col is not None and long_col < n_x + min(i, limit) and rng.random() < 0.7:
            e[long_col] = coeff()
        return (e, rng.randrange(ELL) if rng.random() < 0.5 else 0)

    A = [row(i, i) for i in range(m)]
    B = [row(i, i) for i in range(m)]
    O = [row(m, m) for _ in range(n_out)]
    return A, B, O


# ---- shared by tests/test_p8_ref.py and tests/test_gpu_circuit_sat.py ----------------------------------------------------
# (seed, n_x, m, n_out) of every random circuit the GPU test proves
GPU_CASES = [(100 + m, 5, m, 2) for m in (1, 2, 3, 63, 64, 65, 1000, 4096)] + [(7, 4, 0, 1), (8, 6, 9, 0), (9, 1532, 32000, 1)]


def to_csr(rows):
    ptr, col, vals, consts = [0], [], [], []
    for e, k in rows:
        for c, v in e.items():
            col.append(c)
            vals.append(v)
        ptr.append(len(col))
        consts.append(k)
    return ptr, col, vals, consts


def sparse(n_x, A, B, O):
    from verifiable_mpc_amd.circuit_sat_gpu import SparseCircuit
    return SparseCircuit(n_x, to_csr(A), to_csr(B), to_csr(O))


def untyped(s, field=None):
    """a fixture's "i:<decimal>" / "f:<hex>" -> int, or field(residue) when a field is given"""
    if s.startswith("i:"):
        return int(s[2:])
    v = int(s[2:], 16)
    return field(v) if field else v


def fixture_rows(forms, field=None):
    """recorded dense forms -> [({col: coefficient}, constant)] (zero ints are no entries)"""
    out = []
    for f in forms:
        co = [untyped(v, field) for v in f["coeffs"]]
        out.append(({i: v for i, v in enumerate(co) if not (isinstance(v, int) and v == 0)}, untyped(f["constant"], field)))
    return out


def circuit_from_fixture(case, field=None):
    """a data stand-in for the circuit_builder.Circuit a fixture was recorded from: gates, mul_gates(), output_gates,
    input_ct, mul_ct, gate .op.name / .inputs / .output / .mul_index, str()"""
    from types import SimpleNamespace
    variables = {}

    def var(name, input_index=None):
        if name not in variables:
            variables[name] = SimpleNamespace(name=name, input_index=input_index, output_index=None)
        return variables[name]

    gates = []
    for g in case["gates"]:
        ins = [var(v["var"], v["input_index"]) if "var" in v else untyped(v["const"], field) for v in g["inputs"]]
        out = var(g["output"])
        out.output_index = g["output_index"]
        gates.append(SimpleNamespace(op=SimpleNamespace(name=g["op"]), inputs=ins, output=out, mul_index=g["mul_index"]))

    class Circuit:
        def mul_gates(self):
            return [g for g in self.gates if g.op.name == "mul"]

        def __str__(self):
            return case["circuit_str"]
    c = Circuit()
    c.gates, c.output_gates, c.input_ct, c.mul_ct = gates, list(case["output_gates"]), case["input_ct"], case["mul_ct"]
    return c
