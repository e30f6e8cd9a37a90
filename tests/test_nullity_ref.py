"""CPU: the restatement tests/nullity_ref.py agrees with the fixture the reference's own nullity.py produced
(tests/golden/make_nullity_fixtures.py), and the stand-in tests/refshape/ac20/nullity.py - "the reference calling the
installed functions" of tests/test_gpu_nullity.py - reproduces that fixture hash for hash on its own CPU code."""
import random

import pytest

from tests import nullity_ref as nr
from tests.conftest import load_golden
from tests.test_refshape_harness import proj_hex, record_hashes, typed_of

ELL = nr.ELL
hx = lambda v: format(int(v), "x")
CASES = load_golden("nullity_ed25519.json")["cases"]
IDS = [c["name"] for c in CASES]


def test_fixture_has_the_cases_the_issue_names():
    assert sorted((c["s"], c["n"], c["forms_typed"][0][0][0]) for c in CASES) == \
        [(1, 3, "f"), (1, 3, "i"), (3, 7, "f"), (3, 7, "i"), (5, 15, "f"), (5, 15, "i")]
    assert any(t.startswith("i:-") for c in CASES for form in c["forms_typed"] for t in form)
    nonzero = [c for c in CASES if int(c["y_typed"][2:], 16 if c["y_typed"][0] == "f" else 10) % ELL]
    assert [c["name"] for c in nonzero] == ["3x7_field_nonzero"]
    assert all(c["verified"] is True for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_agrees_with_the_fixture(case):
    forms = [[nr.typed_value(t) for t in form] for form in case["forms_typed"]]
    x = [nr.typed_value(t) for t in case["x_typed"]]
    rho = int(case["rho"], 16)
    P = [int(c, 16) for c in case["P_proj"]]
    assert nr.reference_rho(P, case["forms_typed"]) == rho == int(case["hashes"][0]["c"], 16)
    L = [nr.typed_value(t) for t in case["L_typed"]]
    assert nr.combine(forms, rho) == [c % ELL for c in L]
    if case["L_typed"][0][0] == "i":       # Python ints: the reference's L is the exact, unreduced integer sum
        assert L == [sum(form[j] * rho ** i for i, form in enumerate(forms)) for j in range(case["n"])]
    assert [hx(v) for v in nr.values(forms, x)] == case["values"]
    y = nr.typed_value(case["y_typed"]) % ELL
    assert nr.values([nr.combine(forms, rho)], x) == [y]
    assert y == sum(pow(rho, i, ELL) * int(v, 16) for i, v in enumerate(case["values"])) % ELL
    assert nr.first_nonzero(forms, x) == (1 if case["name"] == "3x7_field_nonzero" else None)


def test_compact_challenge_binds_the_point_and_every_coefficient():
    case = CASES[2]
    forms = [[nr.typed_value(t) for t in form] for form in case["forms_typed"]]
    P = [int(c, 16) for c in case["P_proj"]]
    rho = nr.compact_rho(P, nr.dense_digest(forms))
    assert 0 <= rho < ELL and rho == nr.compact_rho([2 * c % nr.P25519 for c in P], nr.dense_digest(forms))
    other = [list(f) for f in forms]
    other[4][14] += 1
    assert nr.dense_digest(other) != nr.dense_digest(forms)
    assert nr.dense_digest([f + [0] for f in forms]) != nr.dense_digest(forms)
    assert nr.dense_digest([[c + ELL for c in f] for f in forms]) == nr.dense_digest(forms)
    rows = [{j: c for j, c in enumerate(f)} for f in forms]
    assert nr.sparse_digest(rows, 15) == nr.sparse_digest([{**r, 3: r[3] + ELL} for r in rows], 15)
    assert nr.sparse_digest(rows, 15) != nr.sparse_digest(rows, 16)


# ---- the stand-in, driven with the fixture's inputs in ITS types ---------------------------------------------------------
def foreign_inputs(rs, nullity, case):
    """(generators, P, lin_forms, x, gamma, gf) in the stand-in's types, prngs seeded as the fixture's generator seeded
    the reference's; `nullity` is tests.refshape.ac20.nullity"""
    group, gf = rs.demo.group_and_field("Elliptic")
    rs.r1cs.prng = random.Random(case["seed"] + 1)
    generators = rs.r1cs.create_generators(case["n"], rs.cs.PivotChoice.compressed, group)
    rs.compressed_pivot.prng = random.Random(case["seed"] + 2)

    def value(t):
        return int(t[2:]) if t[0] == "i" else gf(int(t[2:], 16))
    x = [value(t) for t in case["x_typed"]]
    lin_forms = [rs.pivot.LinearForm([value(t) for t in form]) for form in case["forms_typed"]]
    gamma = int(case["gamma"], 16)
    P = rs.pivot.vector_commitment(x, gamma, generators["g"], generators["h"])
    return generators, P, lin_forms, x, gamma, gf


def check_nullity_fixture(case, P, proof, L, y, rho, calls, order, coords=proj_hex):
    assert coords(P) == case["P_proj"]
    assert hx(rho) == case["rho"]
    assert [typed_of(v, order) for v in L.coeffs] == case["L_typed"]
    assert typed_of(L.constant, order) == case["L_constant_typed"]
    assert typed_of(y, order) == case["y_typed"]
    pr = case["proof"]
    assert list(proof.keys()) == case["proof_keys"]
    assert typed_of(proof["t"], order) == pr["t_typed"]
    assert coords(proof["A"]) == pr["A_proj"]
    for i in range(case["rounds"]):
        assert coords(proof[f"A{i}"]) == pr["A_i_proj"][i], f"A{i}"
        assert coords(proof[f"B{i}"]) == pr["B_i_proj"][i], f"B{i}"
    assert [typed_of(v, order) for v in proof["z_prime"]] == pr["z_prime_typed"]
    assert [hx(c) for c in calls] == [h["c"] for h in case["hashes"] + case["verifier_hashes"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stand_in_nullity_reproduces_the_reference_fixture_on_cpu(refshape, case):
    from tests.refshape.ac20 import nullity
    rs = refshape
    generators, P, lin_forms, x, gamma, gf = foreign_inputs(rs, nullity, case)
    calls = []
    record_hashes(rs, calls)
    proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf)
    assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf) is case["verified"]
    check_nullity_fixture(case, P, proof, L, y, rho, calls, gf.order)
    assert isinstance(L, rs.pivot.LinearForm) is case["L_is_linear_form"]
    if case["s"] > 1:        # (a single form is its own combination, whatever rho is)
        assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho + 1, y, proof, gf) is False
