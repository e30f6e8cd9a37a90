"""The restatement of the solve on shares (tests/witness_share_ref.py) against the solve in the clear
(tests/witness_ref.solve): for random sharings of the inputs and random dealt coefficients, every party's output is a
share of the clear witness - any t + 1 of them recombine to it, wire by wire, so the output has degree t - on the
reference-made fixtures and on generated circuits, for every (M, t) that the GPU tests use.  No device."""
import itertools
import random

import pytest

from tests import witness_ref as WR
from tests import witness_share_ref as SR
from tests.conftest import load_golden

N = WR.N
MT = [(1, 0), (3, 1), (4, 1), (5, 2)]


def _circuits():
    cases = load_golden("pinocchio_keygen.json")["cases"]
    out = [(c["name"], WR.from_dense(c), len(c["inputs"])) for c in cases]
    out.append(("rounds-3-1-4", SR.share_layered_r1cs([3, 1, 4], [2, 0, 3, 1], seed=5), 2))
    out.append(("linear-only", SR.share_layered_r1cs([], [3], seed=6), 2))
    return out


@pytest.mark.parametrize("M,t", MT)
def test_shares_recombine_to_the_clear_witness(M, t):
    for name, r1cs, n_in in _circuits():
        rng = random.Random(f"{name}-{M}-{t}")
        inputs = [rng.randrange(N) for _ in range(n_in)]
        want = WR.solve(r1cs, inputs)
        drawn = {}
        coeff = lambda *key: drawn.setdefault(key, rng.randrange(N))
        c, rounds = SR.solve_shares(r1cs, SR.share(inputs, t, M, rng), t, coeff)
        assert rounds == len(SR.round_widths(SR.phases(r1cs, n_in)[0]))
        assert all(cp[0] == 1 for cp in c)
        for subset in itertools.combinations(range(M), t + 1):
            nodes = [p + 1 for p in subset]
            got = [SR.recombine([c[p][w] for p in subset], nodes) for w in range(len(want))]
            assert got == want, (name, subset)
        if t:
            assert any(c[0][w] != want[w] for w in range(1, len(want))), name     # shares, not the values themselves
            assert len(drawn) == M * t * sum(SR.round_widths(SR.phases(r1cs, n_in)[0]))


def test_fixture_rounds():
    """the table of DESIGN.md section 23: 2 and 7 exchanges where the clear solve has 6 and 19 levels"""
    cases = {c["name"]: c for c in load_golden("pinocchio_keygen.json")["cases"]}
    for name, widths, linear, levels in (("demo", [2, 1], 4, 6), ("larger", [5, 3, 2, 3, 1, 2, 1], 14, 19)):
        r1cs, n_in = WR.from_dense(cases[name]), len(cases[name]["inputs"])
        ph, checks = SR.phases(r1cs, n_in)
        assert SR.round_widths(ph) == widths and checks == 0
        assert sum(len(lv) for p in ph if p[0] == "L" for lv in p[2]) == linear
        assert len(WR.plan(r1cs, n_in)) == levels


@pytest.mark.parametrize("widths,local", [([1], [0, 0]), ([65, 1, 257], [3, 0, 2, 1]), ([2, 2], [1, 3, 0]), ([], [2])])
def test_generator_gives_its_prescribed_shape(widths, local):
    r1cs = SR.share_layered_r1cs(widths, local, seed=len(widths) + sum(local))
    ph, checks = SR.phases(r1cs, 2)
    assert SR.round_widths(ph) == widths and SR.local_depths(ph) == local and checks == 0
    assert [p[:2] for p in ph] == [("L", 0)] + [x for r in range(1, len(widths) + 1) for x in (("P", r), ("L", r))]
    order = [x["row"] for p in ph for lv in (p[2] if p[0] == "L" else [p[2]]) for x in lv]
    assert sorted(order) == list(range(len(r1cs[0])))
    if len(order) > 4:
        assert order != sorted(order)                                # shuffled: a plan has to reorder
    coefs = [x for M in r1cs[:3] for row in M for _, x in row]
    if len(coefs) > 100:
        assert any(x < 0 for x in coefs) and any(x > N for x in coefs) and any(N > x > 1 << 200 for x in coefs)


def test_errors_name_the_constraint():
    shared = ([[(1, 1)], [(3, 1)]], [[(1, 1)], [(2, 1)]], [[(4, 1)], [(1, 1)]], 4)       # row 2: wire 3 = x1 / x2
    with pytest.raises(SR.SharedDivisor) as e:
        SR.classify(shared, 2)
    assert e.value.args[1] == 2
    zero = ([[(1, 1)], [(3, 1)]], [[(1, 1)], []], [[(4, 1)], [(1, 1)]], 4)               # row 2: wire 3 * 0 = x1
    with pytest.raises(SR.ZeroDivisor) as e:
        SR.classify(zero, 2)
    assert e.value.args[1] == 2
