"""The Python restatement of the BN-256 optimal-ate pairing (tests/bn256_pairing_ref.py) against the values the
reference's own pairing.py produced (tests/golden/bn256_pairing.json, tests/golden/make_pairing_fixtures.py), and
against the defining properties of a pairing.  CPU only."""
import random

import pytest

from tests import bn256_pairing_ref as R
from tests.conftest import load_golden


def _g1(v):
    return None if v is None else (int(v[0], 16), int(v[1], 16))


def _g2(v):
    return None if v is None else ((int(v[0], 16), int(v[1], 16)), (int(v[2], 16), int(v[3], 16)))


@pytest.fixture(scope="module")
def fixture():
    return load_golden("bn256_pairing.json")


def test_restatement_reproduces_reference_values(fixture):
    assert len(fixture["pairing"]) >= 8
    for case in fixture["pairing"]:
        want = tuple(int(v, 16) for v in case["gt"])
        assert R.pairing(_g1(case["g1"]), _g2(case["g2"])) == want, case["name"]


def test_infinity_gives_one(fixture):
    assert R.pairing(None, R.G2) == R.GT_ONE
    assert R.pairing(R.G1, None) == R.GT_ONE
    ones = [c for c in fixture["pairing"] if c["g1"] is None or c["g2"] is None]
    assert ones and all(tuple(int(v, 16) for v in c["gt"]) == R.GT_ONE for c in ones)


def test_bilinear():
    rng = random.Random(7)
    e = R.pairing(R.G1, R.G2)
    for _ in range(2):
        a, b = rng.randrange(1, R.N), rng.randrange(1, R.N)
        assert R.pairing(R.E1.mul(a, R.G1), R.E2.mul(b, R.G2)) == R.gt_pow(e, a * b % R.N)


def test_order_and_non_degenerate():
    e = R.pairing(R.G1, R.G2)
    assert e != R.GT_ONE
    assert R.gt_pow(e, R.N) == R.GT_ONE


def test_fixture_pinocchio_instance_verified_by_reference(fixture):
    pin = fixture["pinocchio"]
    assert pin["verification"] == {"H": True, "V": True, "W": True, "Y": True, "Z": True}
    assert set(pin["proof"]) >= {"r_v*v_mid*g1", "r_w*w_mid*g2", "h*g1"}
    assert pin["indices_io"]
