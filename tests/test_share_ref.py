"""tests/share_ref.py against itself: dealing and recombining, the degree of a product of sharings, and the extension
points against tests/p8_ref.py's z tail."""
import random

import pytest

from tests import p8_ref as ref
from tests import share_ref as sh

ELL = sh.ELL
CASES = [(1, 0), (3, 1), (5, 2), (7, 3)]


@pytest.mark.parametrize("parties,t", CASES)
def test_deal_then_recombine_returns_the_value(parties, t):
    rng = random.Random(parties)
    for value in (0, 1, ELL - 1, rng.randrange(ELL)):
        shares = sh.deal(value, [rng.randrange(ELL) for _ in range(t)], parties)
        assert sh.recombine(shares) == value
        # any t + 1 parties suffice, and fewer see a value that is not the secret
        nodes = list(range(parties - t, parties + 1))
        assert sh.recombine(shares[parties - t - 1:], nodes) == value
        # the sharing has degree t: t + 1 shares determine every other one
        for q in range(parties):
            assert sh.recombine(shares[:t + 1], list(range(1, t + 2)), at=q + 1) == shares[q]


@pytest.mark.parametrize("parties,t", CASES)
def test_products_need_the_two_t_degree_weights(parties, t):
    rng = random.Random(100 + parties)
    u, v = rng.randrange(ELL), rng.randrange(ELL)
    su = sh.deal(u, [rng.randrange(1, ELL) for _ in range(t)], parties)
    sv = sh.deal(v, [rng.randrange(1, ELL) for _ in range(t)], parties)
    prod = [x * y % ELL for x, y in zip(su, sv)]
    assert sh.recombine(prod[:2 * t + 1], list(range(1, 2 * t + 2))) == u * v % ELL
    assert sh.recombine(prod) == u * v % ELL
    if t >= 1:
        assert sh.recombine(prod[:t + 1], list(range(1, t + 2))) != u * v % ELL


@pytest.mark.parametrize("parties,t", CASES)
def test_mul_deal_then_combine_is_a_degree_reduction(parties, t):
    """schur_prod as the kernels do it: every party re-shares its product, the sums with the Lagrange weights are a
    degree-t sharing of the product"""
    rng = random.Random(200 + parties)
    n = 5
    u, v = [rng.randrange(ELL) for _ in range(n)], [rng.randrange(ELL) for _ in range(n)]
    su = sh.mul_deal(u, None, [[rng.randrange(ELL) for _ in range(n)] for _ in range(t)], parties)
    sv = sh.mul_deal(v, None, [[rng.randrange(ELL) for _ in range(n)] for _ in range(t)], parties)
    dealt = [sh.mul_deal(su[p], sv[p], [[rng.randrange(ELL) for _ in range(n)] for _ in range(t)], parties)
             for p in range(parties)]
    lam = sh.weights(list(range(1, parties + 1)))
    mine = [sh.combine([dealt[p][q] for p in range(parties)], lam) for q in range(parties)]
    for i in range(n):
        col = [mine[q][i] for q in range(parties)]
        assert sh.recombine(col[:t + 1], list(range(1, t + 2))) == u[i] * v[i] % ELL
        assert sh.recombine(col) == u[i] * v[i] % ELL


def test_combine_scatters_and_leaves_the_rest():
    parts = [[1, 2, 3], [10, 20, 30]]
    assert sh.combine(parts, [1, 1]) == [11, 22, 33]
    assert sh.combine(parts, [ELL - 1, 1], dst=[4, 0, 2], out=[7] * 5) == [18, 7, 27, 7, 9]


@pytest.mark.parametrize("m", [0, 1, 2, 3, 9])
def test_extension_points_multiply_to_the_z_tail(m):
    rng = random.Random(300 + m)
    a, b = [rng.randrange(ELL) for _ in range(m + 1)], [rng.randrange(ELL) for _ in range(m + 1)]
    f, g = sh.extend_fg(a, b)
    assert len(f) == len(g) == max(m, 1)
    tail = ref.z_tail_naive(a[:m], b[:m], a[m], b[m])       # f(0), g(0), h(0), h(1..2m) from coefficient lists
    assert [f[0], g[0], f[0] * g[0] % ELL] == tail[:3]
    assert [x * y % ELL for x, y in zip(f[1:], g[1:])] == tail[3 + m + 1:]
