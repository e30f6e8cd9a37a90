"""tests/ptvec_ref.py held against oracle/ed25519_ref.py and against its own definitions (no GPU)."""
import random

import pytest

from oracle import ed25519_ref as ed
from tests import ptvec_ref as ref

P, ELL = ed.P, ed.ELL


@pytest.fixture(scope="module")
def points():
    rng = random.Random(4096)
    return [ed.pt_repeat(ed.BASE, rng.randrange(1, ELL)) for _ in range(12)] + [ed.IDENTITY, ed.BASE]


def test_normalize_is_pt_affine_where_z_is_not_zero(points):
    assert all(z != 1 for _, _, z in points[:12])
    assert ref.normalize(points) == [ed.pt_affine(p) for p in points]
    assert ref.normalize([]) == []


def test_normalize_of_z_zero_is_zero_zero_and_touches_no_neighbour(points):
    void = [(5, 7, 0), (P - 1, 1, 0), (0, 0, 0), (3, 4, P)]         # P is 0 as well
    assert ref.normalize(void) == [(0, 0)] * 4
    mixed = [points[0], void[0], points[1], void[1], void[2], points[2]]
    want = [ed.pt_affine(points[0]), (0, 0), ed.pt_affine(points[1]), (0, 0), (0, 0), ed.pt_affine(points[2])]
    assert ref.normalize(mixed) == want


def test_rescale_keeps_the_group_element(points):
    rng = random.Random(7)
    for p in points:
        for lam in (1, 2, P - 1, rng.randrange(1, P)):
            q = ref.rescale(p, lam)
            assert ed.pt_eq(p, q) and ref.normalize([q]) == ref.normalize([p])
            assert all(0 <= c < P for c in q)
    x, y, z = points[0]
    assert ref.rescale(points[0], (P - 1) * pow(z, P - 2, P))[2] == P - 1
    assert ref.rescale(points[0], (P - 1) * pow(x, P - 2, P))[0] == P - 1
    assert ref.rescale(ed.IDENTITY, 12345) == (0, 12345, 12345)
    with pytest.raises(AssertionError):
        ref.rescale(points[0], P)


EDGE_EXPONENTS = [0, 1, -1, ELL - 1, 1 - ELL, ELL, -ELL, (1 << 255) - 1, 1 - (1 << 255)]


def test_sign_magnitude_round_trips():
    for n in EDGE_EXPONENTS:
        b = ref.sign_magnitude(n)
        assert len(b) == 32 and ref.from_sign_magnitude(b) == n
        assert b[31] >> 7 == (n < 0)
        assert int.from_bytes(b, "little") & ((1 << 255) - 1) == abs(n)
    assert ref.sign_magnitude(0) == bytes(32)
    assert ref.sign_magnitude(0, negative_zero=True) == bytes(31) + b"\x80"
    assert ref.from_sign_magnitude(ref.sign_magnitude(0, negative_zero=True)) == 0
    assert ref.sign_magnitude(-1) == b"\x01" + bytes(30) + b"\x80"
    for n in (1 << 255, -(1 << 255)):
        with pytest.raises(AssertionError):
            ref.sign_magnitude(n)


def test_low_order_points_are_on_the_curve_and_zero_zero_is_not():
    assert len(set(ref.LOW_ORDER)) == 4
    for x, y in ref.LOW_ORDER:
        assert ed.on_curve((x, y, 1)) and ref.is_valid_affine(x, y)
        four = ed.pt_repeat((x, y, 1), 4)
        assert ed.pt_affine(four) == (0, 1)
    assert ed.pt_affine(ed.pt_repeat((0, P - 1, 1), 2)) == (0, 1)
    assert ed.pt_affine(ed.pt_repeat((ed.SQRT_M1, 0, 1), 2)) == (0, P - 1)
    assert not ed.on_curve((0, 0, 1)) and not ref.is_valid_affine(0, 0)


def test_is_valid_affine_is_on_curve_and_below_p(points):
    for p in points:
        x, y = ed.pt_affine(p)
        assert ref.is_valid_affine(x, y)
        assert not ref.is_valid_affine(x, y ^ 1) and not ed.on_curve((x, y ^ 1, 1))
        assert not ref.is_valid_affine(x ^ 1, y)
        assert not ref.is_valid_affine(x | 1 << 255, y)
        assert not ref.is_valid_affine(x, y | 1 << 255)
    # the same residues, one encoding too high: on the curve for ed.on_curve, which reduces, and refused here
    for x, y in ((P, 1), (0, P + 1), (ed.SQRT_M1, P), (P, P - 1)):
        assert ed.on_curve((x, y, 1)) and not ref.is_valid_affine(x, y)
    assert not ref.is_valid_affine(0, P)            # (0, p) is (0, 0)
    assert not ref.is_valid_affine(-1, 1)


def test_points_with_a_small_coordinate():
    found_x = [ref.affine_with_x(x) for x in range(19)]
    found_y = [ref.affine_with_y(y) for y in range(19)]
    assert found_x[0] in ((0, 1), (0, P - 1)) and found_y[0] in ((ed.SQRT_M1, 0), (P - ed.SQRT_M1, 0))
    for x, pt in enumerate(found_x):
        assert pt is None or (pt[0] == x and ref.is_valid_affine(*pt))
    for y, pt in enumerate(found_y):
        assert pt is None or (pt[1] == y and ref.is_valid_affine(*pt))
    # some coordinate in 1..18 exists for either, so x + p and y + p stay below 2^255 with a non-zero residue
    assert any(pt for pt in found_x[1:]) and any(pt for pt in found_y[1:])
    assert ref.affine_with_x(ed.BASE_X) in ((ed.BASE_X, ed.BASE_Y), (ed.BASE_X, P - ed.BASE_Y))
    assert ref.affine_with_y(ed.BASE_Y) in ((ed.BASE_X, ed.BASE_Y), (P - ed.BASE_X, ed.BASE_Y))


def test_the_guard_pattern_is_no_point():
    pat = int.from_bytes(b"\x5a" * 32, "little")
    assert not ref.is_valid_affine(pat, pat)
    assert ref.normalize([(pat, pat, pat)]) == [(1, 1)] and not ref.is_valid_affine(1, 1)
