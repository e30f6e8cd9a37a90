"""The GF(l) vector operations of csrc/frvec.hip on Python ints: the CPU restatement that tests/test_gpu_frvec.py holds
the kernels against, one entry point at a time.  Written from the formulas of include/vmpc.h, no numpy arithmetic.

    axpy                out[i] = c x[i] + y[i]  (y None: c x[i]), with `tail` one more element behind them
    dot                 sum a[i] b[i]
    challenge_products  out[j] = z[j mod 2^low_bits] * prod_{i < R} (c_i if bit (low_bits + R - 1 - i) of j is 0 else 1)
    tail_scalars        with s[j] = prod_{r < t} (c_r if bit (log2_m0 - 1 - r) of j is 0 else 1), m = 2^log2_m0 >> t,
                        h = m / 2, u = j mod m:   A[j] = z[u - h] s[j] if u >= h else 0
                                                  B[j] = z[u + h] s[j] if u <  h else 0

The product over the challenges depends on R (or t) bits of j only, so both functions take it from a table of 2^R
entries.  `bit_products` fills that table by the formula, bit by bit; `bit_products_by_halves` builds the same table
from its meaning (round 0 multiplies the left half by c_0, round 1 the left half of either half by c_1, ..) with one
multiplication per entry, which is what a test can afford at R = 20.  tests/test_frvec_ref.py holds the two together
and pins both functions, in exponent space, against the generator fold they stand for.
"""
from oracle.ed25519_ref import ELL


def axpy(c, x, y=None, tail=None):
    out = [(c * a) % ELL for a in x] if y is None else [(c * a + b) % ELL for a, b in zip(x, y, strict=True)]
    return out if tail is None else out + [tail % ELL]


def dot(a, b):
    return sum(u * v for u, v in zip(a, b, strict=True)) % ELL


def bit_products(cs):
    """table[b], b < 2^R: the product of the c_i whose bit (R - 1 - i) of b is 0 (the first challenge looks at the top
    bit)"""
    R = len(cs)
    table = []
    for b in range(1 << R):
        s = 1
        for i, c in enumerate(cs):
            if (b >> (R - 1 - i)) & 1 == 0:
                s = s * c % ELL
        table.append(s)
    return table


def bit_products_by_halves(cs):
    table = [1]
    for c in reversed(cs):
        table = [c * s % ELL for s in table] + table
    return table


def challenge_products(cs, low_bits, z, table=None):
    """`table`: bit_products(cs) made elsewhere (bit_products_by_halves at R = 20)"""
    assert len(z) == 1 << low_bits
    table = bit_products(cs) if table is None else table
    assert len(table) == 1 << len(cs)
    mask = (1 << low_bits) - 1
    return [z[j & mask] * table[j >> low_bits] % ELL for j in range(1 << (len(cs) + low_bits))]


def tail_scalars_block(cs, log2_m0, z, j0, count):
    """(A[j0 : j0 + count], B[j0 : j0 + count]) of tail_scalars"""
    t, m0 = len(cs), 1 << log2_m0
    assert 0 <= t < log2_m0 and 0 <= j0 and j0 + count <= m0
    m = m0 >> t
    h = m // 2
    assert len(z) == m
    table = bit_products(cs)
    A, B = [], []
    for j in range(j0, j0 + count):
        s = table[j >> (log2_m0 - t)]
        u = j % m
        A.append(z[u - h] * s % ELL if u >= h else 0)
        B.append(z[u + h] * s % ELL if u < h else 0)
    return A, B


def tail_scalars(cs, log2_m0, z):
    return tail_scalars_block(cs, log2_m0, z, 0, 1 << log2_m0)
