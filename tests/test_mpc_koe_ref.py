"""tests/mpc_koe_ref.py against itself and tests/p8_field_ref.py (no GPU): the statements the M-party knowledge-of-exponent
prover and the joint setup rest on, on Python ints."""
import random

import pytest

from tests import mpc_koe_ref as ref
from tests import p8_field_ref as fref

N = ref.N
ONE = fref.KoeTrapdoor(1, 1, 1)


@pytest.mark.parametrize("M,t", [(1, 0), (3, 1), (5, 2)])
def test_deal_and_recombine(M, t):
    rng = random.Random(10 * M + t)
    vals = [0, 1, N - 1] + [rng.randrange(N) for _ in range(5)]
    shares = ref.deal(vals, t, M, rng)
    assert ref.recombine(shares) == vals
    assert sum(ref.weights(M)) % N == 1               # a public constant is a share of itself
    # a product of two degree-t sharings recombines as long as 2t < M
    prod = [[a * b % N for a, b in zip(sa, sb)] for sa, sb in zip(shares, ref.deal(vals[::-1], t, M, rng))]
    assert ref.recombine(prod) == [a * b % N for a, b in zip(vals, vals[::-1])]


@pytest.mark.parametrize("M,t", [(1, 0), (3, 1), (5, 2)])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_the_product_recombines_coefficient_for_coefficient(M, t, n):
    """(gamma, z) * reversed(L) is linear in (gamma, z) for a public L: the parties' products are shares of the product"""
    rng = random.Random(100 * M + n)
    z, gamma = [rng.randrange(N) for _ in range(n)], rng.randrange(1, N)
    L = [rng.randrange(N) for _ in range(n)]
    z_sh, g_sh = ref.deal(z, t, M, rng), [s[0] for s in ref.deal([gamma], t, M, rng)]
    parts = ref.party_products(L, z_sh, g_sh)
    want = ONE.product(L, z, gamma)
    assert len(want) == 2 * n and all(len(c) == 2 * n for c in parts)
    assert ref.recombine(parts) == want
    assert want[n] == sum(a * b for a, b in zip(L, z)) % N


@pytest.mark.parametrize("M,t", [(3, 1), (5, 2)])
def test_the_joint_opening_is_the_single_provers(M, t):
    rng = random.Random(7 * M)
    n = 6
    trap = fref.KoeTrapdoor(rng.randrange(1, N), rng.randrange(1, N), rng.randrange(1, N))
    z, gamma, L = [rng.randrange(N) for _ in range(n)], rng.randrange(1, N), [rng.randrange(N) for _ in range(n)]
    z_sh, g_sh = ref.deal(z, t, M, rng), [s[0] for s in ref.deal([gamma], t, M, rng)]
    Q_exp, u = ref.joint_opening(trap, L, z_sh, g_sh)
    assert (Q_exp, u) == trap.opening(L, z, gamma) == trap.opening_by_evaluation(L, z, gamma)
    P_exp, pi_exp = trap.commitment(z, gamma)
    w = ref.weights(M)
    assert sum(w[p] * trap.commitment(z_sh[p], g_sh[p])[0] for p in range(M)) % N == P_exp
    assert trap.restriction_check(P_exp, pi_exp) and trap.prq_check(L, P_exp, Q_exp, u)


def test_a_pass_multiplies_the_trapdoors():
    rng = random.Random(3)
    draws = [tuple(rng.randrange(1, N) for _ in range(3)) for _ in range(3)]
    trap = ref.joint_trapdoor(draws[:1])
    for k in (1, 2):
        lhs, rhs = ref.updated_exps(trap, *draws[k], 10)
        trap = ref.joint_trapdoor(draws[:k + 1])
        assert lhs == [trap.lhs_exp(i) for i in range(10)] and rhs == [trap.rhs_exp(i) for i in range(10)]
    assert (trap.g_exp, trap.alpha, trap.s) == tuple(
        draws[0][j] * draws[1][j] * draws[2][j] % N for j in range(3))


@pytest.mark.parametrize("m", [0, 1, 2, 3, 9])
def test_the_barycentric_extension_is_the_interpolating_polynomial(m):
    rng = random.Random(40 + m)
    F = fref.P8(N)
    v = [rng.randrange(N) for _ in range(m + 1)]
    poly = F.interpolate(v)
    assert ref.extend_fg(v) == [F.poly_eval(poly, x) for x in [0] + list(range(m + 2, 2 * m + 1))]
    assert len(ref.extend_fg(v)) == max(m, 1)
