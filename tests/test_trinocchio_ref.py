"""tests/trinocchio_ref.py against itself and tests/h_ref.py on the CPU: the quadratic interpolation and the quotient
against the naive route, Shamir dealing against recombination, and the algebra the M-party prover rests on - the
quotient of share vectors is a degree-2t sharing of the witness's h, although no party's rows satisfy a constraint."""
import random

import pytest

from tests import h_ref as H
from tests import trinocchio_ref as tr

N = tr.N


@pytest.mark.parametrize("d", [1, 2, 3, 17])
def test_interpolation_and_quotient_match_the_naive_route(d):
    rng = random.Random(d)
    a, b, y = ([rng.randrange(N) for _ in range(d)] for _ in range(3))
    assert tr.interpolate(a) == H.interpolate_values(a)
    dl = tuple(rng.randrange(N) for _ in range(3))
    assert tr.quotient(a, b, y) == H.naive_h(a, b, y)
    assert tr.quotient(a, b, y, dl) == H.naive_h(a, b, y, dl)


def test_deal_recombine_and_kernel_restatements():
    rng = random.Random(1)
    for parties, t in ((1, 0), (3, 1), (5, 2), (5, 4)):
        v = rng.randrange(N)
        shares = tr.deal(v, [rng.randrange(N) for _ in range(t)], parties)
        assert tr.recombine(shares) == v
        if t and parties > t + 1:
            assert tr.recombine(shares[:t + 1], list(range(1, t + 2))) == v
    rows = tr.mul_deal([3, 4], [5, 6], [[7, 8]], 3)
    assert rows == [[15 + 7 * q, 24 + 8 * q] for q in (1, 2, 3)]
    assert tr.combine(rows, [1, 1, 1], addend=[1, N - 1]) == [15 * 3 + 7 * 6 + 1, 24 * 3 + 8 * 6 - 1]
    assert tr.residual([2, 3], [5, 7], [10, 20], 9) == 9 and tr.residual([2, 3], [5, 7], [10, 21], 9) == 0


@pytest.mark.parametrize("d,M,t", [(3, 3, 1), (9, 5, 2)])
def test_quotients_of_share_vectors_share_h(d, M, t):
    V, W, Y, out_ix, m, c = H.satisfiable_r1cs(d, seed=d)
    rng = random.Random(d)
    shares = tr.share_vector(c, t, M, rng)
    dl = tuple(rng.randrange(N) for _ in range(3))
    dshares = tr.share_vector(dl, t, M, rng)
    a, b, y = (H.csr_row_values(Mx, c) for Mx in (V, W, Y))
    want, rem = tr.quotient(a, b, y, dl)
    assert not any(rem)
    hs = []
    for p in range(M):
        ap, bp, yp = (H.csr_row_values(Mx, shares[p]) for Mx in (V, W, Y))
        hp, rp = tr.quotient(ap, bp, yp, tuple(dshares[p]))
        assert any(rp)                       # the party's rows satisfy nothing
        hs.append(hp)
    assert [tr.recombine([hs[p][k] for p in range(M)]) for k in range(d + 1)] == want
    # and the residuals of the parties share 0
    rho = rng.randrange(N)
    res = [tr.residual(*(H.csr_row_values(Mx, shares[p]) for Mx in (V, W, Y)), rho) for p in range(M)]
    assert any(res) and tr.recombine(res) == 0
