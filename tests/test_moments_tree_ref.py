"""The subproduct-tree route to the moments (tests/moments_tree_ref.py) equals their definition, on big integers: no
device.  Small leaves so that several levels, padded leaves and n_out on either side of d all occur."""
import random

import pytest

from tests import moments_tree_ref as R

PAIRS = [(1, 8), (2, 2), (3, 5), (5, 5), (17, 17), (33, 40), (64, 64), (65, 30), (100, 100)]


@pytest.mark.parametrize("d,n_out", PAIRS)
@pytest.mark.parametrize("s_max", [4, 7])
def test_tree_route_equals_the_definition(d, n_out, s_max):
    rng = random.Random(1000 * d + n_out)
    u = [rng.randrange(R.N) for _ in range(d)]
    got, (s, L, dp) = R.tree_moments(u, n_out, s_max)
    assert got == R.moments(u, n_out)
    assert s <= s_max and dp >= d and dp - d < (1 << L) and (L == 0 or 2 * s > s_max)
    assert L == 0 or d > s_max          # several levels occur for the larger pairs


def test_unreduced_and_degenerate_inputs():
    d, n_out = 21, 25
    for u in ([0] * d, [5] + [0] * (d - 1), [0] * (d - 1) + [7], [R.N - 1] * d, [R.N + 3, 2 ** 256 - 1] + [1] * (d - 2)):
        assert R.tree_moments(u, n_out, 4)[0] == R.moments(u, n_out)


def test_newton_inverse_is_an_inverse():
    rng = random.Random(7)
    for n in (1, 2, 3, 8, 13):
        D = [1] + [rng.randrange(R.N) for _ in range(n - 1)]
        assert R.mul(D, R.inv_series(D, n))[:n] == [1] + [0] * (n - 1)


def test_geometry_and_plan_layout():
    for d in list(range(1, 1026)) + [(1 << 20) - 1]:
        s, L, dp = R.geometry(d)
        assert s <= R.S_MAX and dp >= d and dp - d < (1 << L) and (L == 0 or 2 * s > R.S_MAX)
        assert dp <= 1 << 20 and L <= 13
        for n_max in (1, d, 2 * d):
            levels, dinv, tmp, total = R.plan_scalars(d, n_max)
            ends = [levels[l] + dp + (1 << (L - l)) for l in range(L + 1)]
            assert levels[0] == 0 and [levels[l] for l in range(1, L + 1)] == ends[:-1]
            assert dinv == ends[-1] and tmp == dinv + n_max and total == tmp + 2 * n_max
            assert total == (L + 1) * dp + (1 << (L + 1)) - 1 + 3 * n_max
