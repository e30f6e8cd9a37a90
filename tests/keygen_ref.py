"""A Python restatement of Pinocchio key generation (verifiable_mpc/trinocchio/pynocchio.py:101-200) over a QAP given
by its R1CS, with big ints: the independent side of tests/test_keygen_ref.py and tests/test_gpu_pinocchio_keygen.py.

The reference interpolates constraint j at x = j (j = 1..d, qap_creator.r1cs_to_qap_ff) and t(x) = prod (x - j), so
    v_i(s) = sum_j V[j][i] l_j(s),   l_j(s) = t(s) / ((s - j) w_j),   w_j = prod_{k != j} (j - k) = (-1)^(d-j) (j-1)! (d-j)!
(barycentric form; s in {1..d} gives l_j = [j = s]).  O(nnz + d) field operations, one batch inversion.
"""
import numpy as np

N = 65000549695646603732796438742359905742570406053903786389881062969044166799969


def batch_inverse(xs):
    """[1/x mod N for x in xs] with one modular inversion (xs all non-zero)"""
    pre, run = [], 1
    for x in xs:
        pre.append(run)
        run = run * x % N
    inv = pow(run, N - 2, N)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % N
        inv = inv * xs[i] % N
    return out


def lagrange_at(s, d):
    """([l_1(s), .., l_d(s)], t(s)) for the points 1..d"""
    s %= N
    if 1 <= s <= d:
        ell = [0] * d
        ell[s - 1] = 1
        return ell, 0
    t = 1
    for j in range(1, d + 1):
        t = t * (s - j) % N
    fact = [1] * (d + 1)
    for k in range(1, d + 1):
        fact[k] = fact[k - 1] * k % N
    den = []
    for j in range(1, d + 1):
        w = fact[j - 1] * fact[d - j] % N
        if (d - j) & 1:
            w = N - w
        den.append((s - j) * w % N)
    return [t * iv % N for iv in batch_inverse(den)], t


def horner(coeffs, s):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * s + int(c)) % N
    return acc


def entries_of_rows(rows):
    """dense R1CS rows (code_to_r1cs.flatcode_to_r1cs) -> [(row, col, value)] of the non-zero entries"""
    return [(r, c, int(x)) for r, row in enumerate(rows) for c, x in enumerate(row) if int(x) % N]


def column_values(entries, n_cols, ell):
    """v_i(s) = sum over the entries (row, col, value) of column i of value * l_{row+1}(s)"""
    out = [0] * n_cols
    for r, c, x in entries:
        out[c] = (out[c] + x * ell[r]) % N
    return out


def qap_at(V, W, Y, n_cols, d, s):
    """(v(s), w(s), y(s), t(s)) of an R1CS given as three entry lists"""
    ell, t = lagrange_at(s, d)
    return column_values(V, n_cols, ell), column_values(W, n_cols, ell), column_values(Y, n_cols, ell), t


def interpolate_columns(entries, n_cols, d):
    """the reference's dense QAP polynomials (coefficient lists of length d) by plain Lagrange interpolation"""
    basis = []
    for j in range(1, d + 1):
        poly, den = [1], 1
        for k in range(1, d + 1):
            if k != j:
                poly = [((poly[i - 1] if i else 0) - k * (poly[i] if i < len(poly) else 0)) % N
                        for i in range(len(poly) + 1)]
                den = den * (j - k) % N
        inv = pow(den, N - 2, N)
        basis.append([c * inv % N for c in poly])
    cols = [[0] * d for _ in range(n_cols)]
    for r, c, x in entries:
        for k in range(d):
            cols[c][k] = (cols[c][k] + x * basis[r][k]) % N
    return cols


# the seven exponent vectors in the order of pynocchio._ELEMENTS, with their zero-knowledge tails over the deltas
# (v, w, y): per vector, the tail rows' coefficients of t(s) (None: the point at infinity)
ELEMENT_NAMES = ("r_v*v_mid*g1", "r_w*w_mid*g2", "r_y*y_mid*g1", "r_v*alpha_v*v_mid*g1", "r_w*alpha_w*w_mid*g1",
                 "r_y*alpha_y*y_mid*g1", "r_v*beta*v_mid+r_w*beta*w_mid+r_y*beta*y_mid*g1")


def coefficients(td):
    return {"rv": td.r_v % N, "rw": td.r_w % N, "ry": td.r_y % N, "avrv": td.alpha_v * td.r_v % N,
            "awrw": td.alpha_w * td.r_w % N, "ayry": td.alpha_y * td.r_y % N, "brv": td.beta * td.r_v % N,
            "brw": td.beta * td.r_w % N, "bry": td.beta * td.r_y % N}


def key_exponents(td, v, w, y, t, wires):
    """{element: [exponent per wire] + zero-knowledge tail} as PreparedKey.generate lays its vectors out (the shared
    G1 vectors carry three tail rows for the deltas v, w, y, 0 where unused; the twist vector one)"""
    c = coefficients(td)
    ex = {
        ELEMENT_NAMES[0]: [c["rv"] * v[i] % N for i in wires] + [c["rv"] * t % N, 0, 0],
        ELEMENT_NAMES[1]: [c["rw"] * w[i] % N for i in wires] + [c["rw"] * t % N],
        ELEMENT_NAMES[2]: [c["ry"] * y[i] % N for i in wires] + [0, 0, c["ry"] * t % N],
        ELEMENT_NAMES[3]: [c["avrv"] * v[i] % N for i in wires] + [c["avrv"] * t % N, 0, 0],
        ELEMENT_NAMES[4]: [c["awrw"] * w[i] % N for i in wires] + [0, c["awrw"] * t % N, 0],
        ELEMENT_NAMES[5]: [c["ayry"] * y[i] % N for i in wires] + [0, 0, c["ayry"] * t % N],
        ELEMENT_NAMES[6]: [(c["brv"] * v[i] + c["brw"] * w[i] + c["bry"] * y[i]) % N for i in wires]
        + [c["brv"] * t % N, c["brw"] * t % N, c["bry"] * t % N],
    }
    return ex


def evalkey_exponents(td, v, w, y, t, mid, d):
    """[(name, group, exponent)] of the reference's evalkey, in its insertion order (pynocchio.py:106-166)"""
    c = coefficients(td)
    s = td.s % N
    out = []
    out += [(f"r_v*v{i}*g1", 1, c["rv"] * v[i] % N) for i in mid]
    out += [(f"r_w*w{i}*g2", 2, c["rw"] * w[i] % N) for i in mid]
    out += [(f"r_y*y{i}*g1", 1, c["ry"] * y[i] % N) for i in mid]
    out += [(f"r_v*alpha_v*v{i}*g1", 1, c["avrv"] * v[i] % N) for i in mid]
    out += [(f"r_w*alpha_w*w{i}*g1", 1, c["awrw"] * w[i] % N) for i in mid]
    out += [(f"r_y*alpha_y*y{i}*g1", 1, c["ayry"] * y[i] % N) for i in mid]
    out += [("s^" + str(i) + "*g1", 1, pow(s, i, N)) for i in range(d + 1)]
    out += [(f"r_v*beta*v+r_w*beta*w+r_y*beta*y{i}_g1", 1, (c["brv"] * v[i] + c["brw"] * w[i] + c["bry"] * y[i]) % N)
            for i in mid]
    out += [("r_v*t*g1", 1, c["rv"] * t % N), ("r_w*t*g2", 2, c["rw"] * t % N), ("r_y*t*g1", 1, c["ry"] * t % N),
            ("r_v*alpha_v*t*g1", 1, c["avrv"] * t % N), ("r_w*alpha_w*t*g1", 1, c["awrw"] * t % N),
            ("r_y*alpha_y*t*g1", 1, c["ayry"] * t % N), ("r_v*beta*t*g1", 1, c["brv"] * t % N),
            ("r_w*beta*t*g1", 1, c["brw"] * t % N), ("r_y*beta*t*g1", 1, c["bry"] * t % N), ("t*g1", 1, t % N)]
    return out


def verikey_exponents(td, v, w, y, t, io0):
    """[(name, group, exponent)] of the reference's verikey in its order (pynocchio.py:170-200); g1 / g2 are 1"""
    c = coefficients(td)
    out = [("g1", 1, 1), ("g2", 2, 1), ("alpha_v*g2", 2, td.alpha_v % N), ("alpha_w*g1", 1, td.alpha_w % N),
           ("alpha_y*g2", 2, td.alpha_y % N), ("gamma*g2", 2, td.gamma % N),
           ("beta*gamma*g1", 1, td.beta * td.gamma % N), ("beta*gamma*g2", 2, td.beta * td.gamma % N),
           ("r_y*t*g2", 2, c["ry"] * t % N)]
    out += [(f"r_v*v{i}*g1", 1, c["rv"] * v[i] % N) for i in io0]
    out += [(f"r_w*w{i}*g2", 2, c["rw"] * w[i] % N) for i in io0]
    out += [(f"r_y*y{i}*g1", 1, c["ry"] * y[i] % N) for i in io0]
    return out


def to_array(ints):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), np.uint8).reshape(-1, 32)


class TD:
    """a trapdoor from explicit values (r_y as given)"""

    def __init__(self, r_v, r_w, s, alpha_v, alpha_w, alpha_y, beta, gamma, r_y=None):
        self.r_v, self.r_w, self.s = r_v, r_w, s
        self.alpha_v, self.alpha_w, self.alpha_y, self.beta, self.gamma = alpha_v, alpha_w, alpha_y, beta, gamma
        self.r_y = r_v * r_w % N if r_y is None else r_y


def synthetic_r1cs(d, seed, n_io=4):
    """a circuit of d constraints over about d wires, made with numpy: each matrix row has 1 to 3 entries, wire 0
    ("one") sits in about 3/4 of the rows of V and W (a skewed column), the values are a mix of small ones (-3..3,
    negative included) and random 64-bit ones.  -> (V, W, Y as CSR tuples with int64 values, out_ix, m)"""
    rng = np.random.default_rng(seed)
    m = d + n_io
    mats = []
    for k in range(3):
        counts = rng.integers(1, 4, size=d)
        row_ptr = np.concatenate([[0], np.cumsum(counts)])
        nnz = int(row_ptr[-1])
        col = rng.integers(1, m + 1, size=nnz)
        if k < 2:
            first = row_ptr[:-1]
            col[first] = np.where(rng.random(d) < 0.75, 0, col[first])
        small = rng.integers(-3, 4, size=nnz)
        big = rng.integers(-(1 << 62), 1 << 62, size=nnz)
        vals = np.where(rng.random(nnz) < 0.5, small, big).astype(np.int64)
        mats.append((row_ptr, col, vals))
    return mats[0], mats[1], mats[2], n_io, m


def csr_entries(M):
    row_ptr, col, vals = M
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    return [(int(r), int(c), int(x) % N) for r, c, x in zip(rows.tolist(), np.asarray(col).tolist(),
                                                             np.asarray(vals).tolist())]
