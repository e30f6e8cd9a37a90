"""CPU checks of tests/h_ref.py: the naive restatement of the prover's h reproduces the reference-made fixture
(tests/golden/pinocchio_keygen.json) with a zero remainder, the moment formula that the device implements agrees with
it, and the builder's witnesses satisfy their constraints."""
import pytest

from tests import h_ref as H
from tests.conftest import load_golden

N = H.N
h2i = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def fx():
    return load_golden("pinocchio_keygen.json")["cases"]


def _case_rows(case):
    c = [h2i(x) for x in case["c"]]
    return c, [H.row_values(case["r1cs"][k], c) for k in "VWY"]


def test_naive_restatement_reproduces_the_fixture(fx):
    for case in fx:
        c, (a, b, y) = _case_rows(case)
        deltas = tuple(h2i(x) for x in case["deltas"])
        h, rem = H.naive_h(a, b, y, deltas)
        assert h == [h2i(x) for x in case["h"]], case["name"]
        assert len(h) == case["d"] + 1 and not any(rem)
        h0, rem0 = H.naive_h(a, b, y)
        assert len(h0) == case["d"] - 1 and not any(rem0)


def test_interpolation_matches_the_fixtures_dense_qap(fx):
    for case in fx:
        c, (a, b, y) = _case_rows(case)
        d = case["d"]
        for vals, name in ((a, "v"), (b, "w"), (y, "y")):
            want = [0] * d
            for ci, poly in zip(c, case["qap"][name]):
                for k, x in enumerate(poly):
                    want[k] = (want[k] + ci * h2i(x)) % N
            assert H.interpolate_values(vals) == want
        assert H.t_coeffs(d) == [h2i(x) for x in case["qap"]["t"]]


def test_moment_formula_on_the_fixture(fx):
    for case in fx:
        c, (a, b, y) = _case_rows(case)
        deltas = tuple(h2i(x) for x in case["deltas"])
        assert H.moment_h(a, b, deltas) == [h2i(x) for x in case["h"]]


@pytest.mark.parametrize("d", list(range(1, 41)))
def test_moment_formula_agrees_with_the_naive_route(d):
    V, W, Y, out_ix, m, c = H.satisfiable_r1cs(d, seed=d)
    a, b, y = (H.csr_row_values(M, c) for M in (V, W, Y))
    assert all((ai * bi - yi) % N == 0 for ai, bi, yi in zip(a, b, y))
    deltas = (d * 7919 % N, N - d, pow(3, d, N))
    for dl in (None, deltas, (0, 0, 0)):
        want, rem = H.naive_h(a, b, y, dl)
        assert not any(rem)
        got = H.moment_h(a, b, dl)
        assert got == want and len(got) == (d + 1 if dl is not None else max(d - 1, 0))


@pytest.mark.parametrize("d", [1, 2, 65])
def test_evaluation_identity_agrees_with_the_moment_formula(d):
    """h_identity_holds accepts moment_h's h, with and without deltas, and rejects it with any one coefficient spoiled
    (sampled: the lowest, a middle and the top one)"""
    V, W, Y, out_ix, m, c = H.satisfiable_r1cs(d, seed=100 + d)
    a, b, y = (H.csr_row_values(M, c) for M in (V, W, Y))
    for dl in (None, (d * 7919 % N, N - d, pow(3, d, N)), (0, 0, 0)):
        h = H.moment_h(a, b, dl)
        assert H.h_identity_holds(a, b, y, h, dl, seed=d)
        assert H.h_identity_holds(a, b, y, h + [0], dl, seed=d)          # (a top zero is the same polynomial)
        for k in sorted({0, len(h) // 2, len(h) - 1} & set(range(len(h)))):
            spoiled = list(h)
            spoiled[k] = (spoiled[k] + 1) % N
            assert not H.h_identity_holds(a, b, y, spoiled, dl, seed=d), (dl, k)
    if d > 1:
        assert not H.h_identity_holds(a, b, y, H.moment_h(a, b), (1, 2, 3), seed=d)      # h without its deltas' terms
    # the row values decide, not the witness: a violated row fails whatever h is offered
    y[0] = (y[0] + 1) % N
    assert not H.h_identity_holds(a, b, y, H.moment_h(a, b), seed=d)


def test_builder_degenerate_forms():
    for kw in ({"zero_a": True}, {"zero_b": True}):
        V, W, Y, out_ix, m, c = H.satisfiable_r1cs(9, seed=3, **kw)
        a, b, y = (H.csr_row_values(M, c) for M in (V, W, Y))
        assert not any(y) and (not any(a) or not any(b))
        assert H.moment_h(a, b) == H.naive_h(a, b, y)[0] == [0] * 8


def test_violated_witness_leaves_a_remainder():
    V, W, Y, out_ix, m, c = H.satisfiable_r1cs(12, seed=5)
    wire = V[1][V[0][4]]          # a wire that row 5 of V reads
    c[wire] = (c[wire] + 1) % N
    a, b, y = (H.csr_row_values(M, c) for M in (V, W, Y))
    assert any((ai * bi - yi) % N for ai, bi, yi in zip(a, b, y))
    assert any(H.naive_h(a, b, y)[1])
