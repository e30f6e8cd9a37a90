"""The knowledge-of-exponent fixture (tests/golden/koe_bn256.json, made by the reference) checked against itself
without a GPU, so that it is confirmed before any kernel is blamed: the recorded draws g_exp, alpha, z reproduce every
pp point by oracle/bn256_ref.py scalar multiplications, and tests/bn256_pairing_ref.py reproduces both verifier checks
of every recorded opening from the recorded P, pi, Q, u."""
import pytest

from oracle import bn256_ref as bn
from tests import bn256_pairing_ref as R
from tests.conftest import load_golden

h2i = lambda s: int(s, 16)


def g1(v):
    return None if v is None else (h2i(v[0]), h2i(v[1]))


def g2(v):
    return None if v is None else ((h2i(v[0]), h2i(v[1])), (h2i(v[2]), h2i(v[3])))


@pytest.fixture(scope="module")
def fx():
    return load_golden("koe_bn256.json")


def test_cases_present(fx):
    assert [s["n"] for s in fx["setups"]] == [1, 5, 32, 4]
    for s in fx["setups"]:
        assert len(s["pp_lhs"]) == len(s["pp_rhs"]) == 2 * s["n"]
    assert all(len(s["openings"]) == 2 and h2i(s["openings"][1]["constant"]) != 0 for s in fx["setups"][:3])
    assert fx["setups"][1]["restrictions"][0]["S"] == [0, 2, 3]
    zero = fx["setups"][3]["openings"][0]
    assert zero["P"] is None and zero["pi"] is None and zero["Q"] is None and zero["u"] == "0"


def test_recorded_draws_reproduce_pp(fx):
    for s in fx["setups"]:
        g_exp, alpha, z = h2i(s["g_exp"]), h2i(s["alpha"]), h2i(s["z"])
        assert 1 <= g_exp < bn.N and alpha < bn.N and z < bn.N
        for i in range(2 * s["n"]):
            e = g_exp * pow(z, i + 1, bn.N) % bn.N
            assert bn.E1.mul(e, bn.G1) == g1(s["pp_lhs"][i]), (s["n"], i)
            assert bn.E2.mul(e * alpha % bn.N, bn.G2) == g2(s["pp_rhs"][i]), (s["n"], i)


def product_is_one(pairs):
    f = R.ONE12
    for p, q in pairs:
        if p is not None and q is not None:
            f = R.f12_mul(f, R.miller(p, q))
    return R.to_gt(R.final_exp(f)) == R.GT_ONE


def test_pairing_restatement_reproduces_verifier_checks(fx):
    for s in fx["setups"]:
        n = s["n"]
        lhs, rhs = [g1(p) for p in s["pp_lhs"]], [g2(p) for p in s["pp_rhs"]]
        neg_g1 = bn.E1.neg(lhs[0])
        for o in s["openings"]:
            P, pi, Q = g1(o["P"]), g2(o["pi"]), g1(o["Q"])
            coeffs = [h2i(c) for c in o["L"]]
            u_linear = (h2i(o["u"]) - h2i(o["constant"])) % bn.N
            Rpt = bn.E2.msm([coeffs[n - 1 - j] for j in range(n)], rhs[:n])
            got = {"restriction_arg_check": product_is_one([(P, rhs[0]), (neg_g1, pi)]),
                   "PRQ_check": product_is_one([(P, Rpt), (Q, rhs[0]), (neg_g1, bn.E2.mul(u_linear, rhs[n]))])}
            assert got == o["verification"] == {"restriction_arg_check": True, "PRQ_check": True}, o["name"]
            # u is L(x)
            x = [h2i(v) for v in o["x"]]
            assert h2i(o["u"]) == (sum(c * v for c, v in zip(coeffs, x)) + h2i(o["constant"])) % bn.N
        for r in s["restrictions"]:
            assert product_is_one([(g1(r["P"]), rhs[0]), (neg_g1, g2(r["pi"]))]) is r["verification"] is True
