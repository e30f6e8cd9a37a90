"""A circuit that EVERY choice of its inputs extends to a satisfying witness, for the batch Pinocchio prover's tests
(tests/h_ref.satisfiable_r1cs fits its Y to one witness): constraint j multiplies two random sparse combinations of the
wires 0 .. n_io + j - 1 and DEFINES wire n_io + j - row j of Y is a single 1 on that wire, never on wire 0 (DESIGN.md
section 19's note on the reference verifier's H check).  The independent side of tests/test_pinocchio_batch_host.py and
the two GPU files."""
import random

from tests import h_ref as H

N = H.N


def chain_r1cs(d, seed, n_io=2):
    """-> (V, W, Y as CSR tuples (row_ptr, col, list of ints), out_ix = n_io, m = n_io + d); wire 0 is the constant 1,
    1 .. n_io the inputs, n_io + 1 + j the product of constraint j (0-based)"""
    rng = random.Random(seed)

    def matrix():
        ptr, col, vals = [0], [], []
        for j in range(d):
            for _ in range(rng.randint(1, 3)):
                col.append(rng.randrange(0, n_io + j + 1))
                vals.append(rng.choice([rng.randint(1, 3), -rng.randint(1, 3), rng.randrange(1, N)]))
            ptr.append(len(col))
        return ptr, col, vals
    V, W = matrix(), matrix()
    Y = (list(range(d + 1)), [n_io + 1 + j for j in range(d)], [1] * d)
    return V, W, Y, n_io, n_io + d


def extend(built, inputs):
    """the satisfying witness (ints, c[0] = 1) that the n_io `inputs` extend to"""
    V, W, Y, n_io, m = built
    assert len(inputs) == n_io
    c = [1] + [int(x) % N for x in inputs]
    for j in range(m - n_io):
        a = sum(V[2][e] * c[V[1][e]] for e in range(V[0][j], V[0][j + 1])) % N
        b = sum(W[2][e] * c[W[1][e]] for e in range(W[0][j], W[0][j + 1])) % N
        c.append(a * b % N)
    return c


def witnesses(built, k, seed):
    """k satisfying witnesses from k random input vectors"""
    rng = random.Random(seed)
    return [extend(built, [rng.randrange(N) for _ in range(built[3])]) for _ in range(k)]


def rows(built, c):
    """(a, b, y): the row values of the witness c"""
    return tuple(H.csr_row_values(M, c) for M in built[:3])
