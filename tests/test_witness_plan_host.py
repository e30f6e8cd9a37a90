"""pynocchio.SolvePlan (the host half of the R1CS solve) against the big-int restatement of
tests/witness_ref.py: levels, kinds, order, inverse coefficients and stored entries on the reference-made fixture, on
tests/pinocchio_batch_ref.chain_r1cs and on shuffled layered circuits; hand-written rows of each shape; every error.
No device: nothing here creates a context."""
import functools

import numpy as np
import pytest

from tests import pinocchio_batch_ref as B
from tests import witness_ref as WR
from tests.conftest import load_golden

N = WR.N
h2i = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def pn():
    from verifiable_mpc_amd import _native, pynocchio
    real = _native.Context

    def no_context(*a, **k):
        raise AssertionError("a host test created a device context")
    _native.Context = no_context
    try:
        yield pynocchio
    finally:
        _native.Context = real


def qap_of(pn, r1cs, out_ix):
    V, W, Y, m = r1cs
    return pn.R1CSQAP(WR.csr(V), WR.csr(W), WR.csr(Y), out_ix, m=m)


def assert_same_plan(plan, levels):
    flat = [x for level in levels for x in level]
    assert plan.n_levels == len(levels)
    assert plan.level_ptr.tolist() == [0] + list(np.cumsum(WR.level_widths(levels)))
    assert plan.row.tolist() == [x[0] for x in flat]
    assert plan.kind.tolist() == [x[1] for x in flat]
    assert plan.wire.tolist() == [0xFFFFFFFF if x[2] is None else x[2] for x in flat]
    assert plan.inv == [x[3] for x in flat]
    for k, name in enumerate("VWY"):
        ptr, col, vals = plan.csr[name]
        assert len(ptr) == len(flat) + 1
        for i, x in enumerate(flat):
            assert dict(zip(col[ptr[i]:ptr[i + 1]], vals[ptr[i]:ptr[i + 1]])) == x[4][k], (name, i)
            assert ptr[i + 1] - ptr[i] == len(x[4][k])        # duplicates were added, zeros dropped


# ---- the fixture ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cases():
    return load_golden("pinocchio_keygen.json")["cases"]


@pytest.mark.parametrize("i,depth", [(0, 6), (1, 19)])
def test_fixture_plan_and_witness(pn, i, depth):
    case = _cases()[i]
    r1cs = WR.from_dense(case)
    n_in = len(case["inputs"])
    levels = WR.plan(r1cs, n_in)
    assert len(levels) == depth and sum(WR.level_widths(levels)) == case["d"]
    assert {x[1] for level in levels for x in level} == {WR.KY}
    assert WR.solve(r1cs, case["inputs"], levels) == [h2i(x) for x in case["c"]]
    r = case["r1cs"]
    assert_same_plan(pn.SolvePlan(pn.R1CSQAP(r["V"], r["W"], r["Y"], case["out_ix"], m=case["m"]), n_in), levels)


# ---- plan against restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 65, 513])
def test_chain_plan(pn, d):
    built = B.chain_r1cs(d, seed=2100 + d)
    r1cs = WR.from_csr(built)
    levels = WR.plan(r1cs, built[3])
    plan = pn.SolvePlan(qap_of(pn, r1cs, built[3]), built[3])
    assert_same_plan(plan, levels)
    assert WR.solve(r1cs, [3, 4], levels) == B.extend(built, [3, 4])


def test_chain_depths_of_the_probe(pn):
    """the level counts DESIGN.md section 22 quotes"""
    for d, depth in ((1025, 37), (4096, 50)):
        built = B.chain_r1cs(d, seed=2100 + d)
        assert pn.SolvePlan(qap_of(pn, WR.from_csr(built), built[3]), built[3]).n_levels == depth


@pytest.mark.parametrize("widths", [[1, 1, 1, 1, 1], [64], [65], [63, 65, 1, 257, 1], [256, 257, 1], [5, 3, 7]])
def test_layered_plan(pn, widths):
    r1cs = WR.layered_r1cs(widths, seed=sum(widths), checks=0 if len(widths) == 1 else 3)
    levels = WR.plan(r1cs, 2)
    want = list(widths)
    want[0] += 0 if len(widths) == 1 else 3
    assert WR.level_widths(levels) == want
    order = [x[0] for level in levels for x in level]
    if len(widths) > 1:
        assert order != sorted(order)                         # shuffled: the plan has to reorder
    if sum(widths) > 20:
        assert {x[1] for level in levels for x in level} == {WR.CHECK, WR.KY, WR.KA, WR.KB} - \
            (set() if len(widths) > 1 else {WR.CHECK})
    assert_same_plan(pn.SolvePlan(qap_of(pn, r1cs, 2), 2), levels)
    c = WR.solve(r1cs, [5, N - 7], levels)
    for j in range(len(r1cs[0])):
        a, b, y = (sum(x * c[w] for w, x in M[j]) % N for M in r1cs[:3])
        assert a * b % N == y, j


def test_plan_is_cached_per_n_in(pn):
    r1cs = WR.layered_r1cs([2, 2], seed=4, n_in=2)
    qap = qap_of(pn, r1cs, 2)
    assert pn.SolvePlan(qap, 2) is pn.SolvePlan(qap, 2)


# ---- hand-written rows -----------------------------------------------------------------------------------------------------

def _plan_of(pn, rows, m, n_in):
    r1cs = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], m)
    levels = WR.plan(r1cs, n_in)
    plan = pn.SolvePlan(qap_of(pn, r1cs, n_in), n_in)
    assert_same_plan(plan, levels)
    return plan, r1cs, levels


def test_set_row(pn):
    """(wire 2 - 5 wire 0) * wire 0 = nothing: V holds the new wire, W is the constant, Y is empty -> kind A"""
    plan, r1cs, levels = _plan_of(pn, [([(2, 1), (0, -5)], [(0, 1)], [])], 2, 1)
    assert plan.kind.tolist() == [pn.KIND_A] and plan.wire.tolist() == [2] and plan.inv == [1]
    assert plan.csr["V"] == ([0, 1], [0], [N - 5]) and plan.csr["Y"] == ([0, 0], [], [])
    assert WR.solve(r1cs, [9], levels) == [1, 9, 5]


def test_division_row(pn):
    """wire 3 * wire 2 = wire 1, wire 3 new: V holds it, W is the divisor, Y the numerator -> kind A, 12 / 4 = 3"""
    plan, r1cs, levels = _plan_of(pn, [([(3, 1)], [(2, 1)], [(1, 1)])], 3, 2)
    assert plan.kind.tolist() == [pn.KIND_A] and plan.wire.tolist() == [3]
    assert WR.solve(r1cs, [12, 4], levels) == [1, 12, 4, 3]
    with pytest.raises(WR.Failed, match="division"):
        WR.solve(r1cs, [12, 0], levels)


def test_kind_b_row(pn):
    """wire 1 * (2 wire 2 + wire 0) = wire 1 + 6: the new wire 2 stands in W with coefficient 2"""
    plan, r1cs, levels = _plan_of(pn, [([(1, 1)], [(2, 2), (0, 1)], [(1, 1), (0, 6)])], 2, 1)
    assert plan.kind.tolist() == [pn.KIND_B] and plan.wire.tolist() == [2]
    assert plan.inv == [pow(2, -1, N)] and plan.csr["W"] == ([0, 1], [0], [1])
    assert WR.solve(r1cs, [3], levels) == [1, 3, 1]                 # 3 (2 c + 1) = 9  ->  c = 1


def test_check_row_and_its_level(pn):
    """x * x = 9 reads only the input: a check row of level 0, placed before the defining row above it in row order"""
    rows = [([(1, 1)], [(1, 1)], [(2, 1)]), ([(1, 1)], [(1, 1)], [(0, 9)]), ([(2, 1)], [(2, 1)], [(0, 81)])]
    plan, r1cs, levels = _plan_of(pn, rows, 2, 1)
    assert plan.level_ptr.tolist() == [0, 2, 3] and plan.row.tolist() == [0, 1, 2]
    assert plan.kind.tolist() == [pn.KIND_Y, pn.KIND_CHECK, pn.KIND_CHECK] and plan.wire.tolist()[1:] == [0xFFFFFFFF] * 2
    assert WR.solve(r1cs, [N - 3], levels) == [1, N - 3, 9]
    with pytest.raises(WR.Failed, match="check"):
        WR.solve(r1cs, [4], levels)


def test_second_definition_becomes_a_check_row(pn):
    """two rows could define wire 2: the lower row does, the other waits one round and checks"""
    rows = [([(1, 2)], [(1, 2)], [(2, 4)]), ([(1, 1)], [(1, 1)], [(2, 1)])]
    plan, r1cs, levels = _plan_of(pn, rows, 2, 1)
    assert plan.level_ptr.tolist() == [0, 1, 2] and plan.row.tolist() == [0, 1]
    assert plan.kind.tolist() == [pn.KIND_Y, pn.KIND_CHECK] and plan.inv == [pow(4, -1, N), 0]
    assert WR.solve(r1cs, [7], levels) == [1, 7, 49]


def test_negative_large_and_duplicate_coefficients(pn):
    """-1 and N + 2 reduce; (1, 5) + (1, -5) cancels and is NOT support, so wire 1's row count stays exact;
    (3, 2) + (3, 3) add to 5 before the inverse is taken"""
    rows = [([(1, -1), (2, 5), (2, -5)], [(0, N + 2)], [(3, 2), (3, 3)])]
    plan, r1cs, levels = _plan_of(pn, rows, 3, 2)
    assert plan.csr["V"] == ([0, 1], [1], [N - 1]) and plan.csr["W"] == ([0, 1], [0], [2])
    assert plan.inv == [pow(5, -1, N)] and plan.csr["Y"] == ([0, 0], [], [])
    assert WR.solve(r1cs, [10, 77], levels) == [1, 10, 77, (-20) * pow(5, -1, N) % N]
    # the cancelled pair is all that mentions wire 2: with wire 2 NOT an input nothing defines it
    with pytest.raises(ValueError, match="wire 2"):
        pn.SolvePlan(qap_of(pn, (r1cs[0], r1cs[1], r1cs[2], 3), 1), 1)


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_errors(pn):
    # the new wire in two of V, W, Y of its defining row
    nonlinear = ([[(1, 1)], [(2, 1)]], [[(0, 1)], [(2, 1)]], [[(0, 3)], [(0, 4)]], 2)
    with pytest.raises(ValueError, match=r"constraint 2 is not linear in wire 2"):
        pn.SolvePlan(qap_of(pn, nonlinear, 1), 1)
    with pytest.raises(ValueError, match="constraint 2"):
        WR.plan(nonlinear, 1)
    # rows left over with two unknown wires each: the lowest is named
    stuck = ([[(1, 1)], [(2, 1)], [(3, 1)]], [[(1, 1)], [(3, 1)], [(2, 1)]], [[(4, 1)], [(0, 1)], [(0, 1)]], 4)
    with pytest.raises(ValueError, match=r"constraint 2 keeps 2 unknown wires"):
        pn.SolvePlan(qap_of(pn, stuck, 1), 1)
    with pytest.raises(ValueError, match="constraint 2"):
        WR.plan(stuck, 1)
    # a wire that no row mentions and that is not an input: the lowest is named
    loose = ([[(1, 1)]], [[(1, 1)]], [[(4, 1)]], 5)
    with pytest.raises(ValueError, match=r"no constraint defines wire 2 "):
        pn.SolvePlan(qap_of(pn, loose, 1), 1)
    with pytest.raises(ValueError, match="wire 2"):
        WR.plan(loose, 1)
    # more inputs than wires
    with pytest.raises(ValueError, match=r"n_in = 6"):
        pn.SolvePlan(qap_of(pn, loose, 1), 6)
    # a reference QAP object: dense polynomials, no R1CS
    class Dense:
        d, m, out_ix, v, w, y, t = 1, 1, 1, [], [], [], None
    with pytest.raises(TypeError, match=r"R1CSQAP\(V, W, Y, out_ix\)"):
        pn.SolvePlan(Dense(), 1)
    with pytest.raises(TypeError, match=r"R1CSQAP\(V, W, Y, out_ix\)"):
        pn.calculate_witness(Dense(), [1])


def test_empty_batch_needs_no_device(pn):
    qap = qap_of(pn, WR.layered_r1cs([2, 2], seed=4), 2)
    out = pn.calculate_witness_batch(qap, [])
    assert out.shape == (0, qap.m + 1, 32) and out.dtype == np.uint8
    assert pn.calculate_witness_batch(qap, np.zeros((0, 2, 32), np.uint8)).shape == (0, qap.m + 1, 32)
    with pytest.raises(ValueError, match="same number of inputs"):
        pn.calculate_witness_batch(qap, [[1, 2], [3]])


def test_launch_counts_on_the_host(pn):
    """vmpc_bn256_r1cs_solve_launches is host arithmetic on the level table: one launch per level at wide_rows = 1, one
    at SIZE_MAX, a launch per wide level and per maximal run of narrower ones in between"""
    from verifiable_mpc_amd import _native as nat
    ptr = lambda widths: np.concatenate([[0], np.cumsum(widths)]).astype(np.uint32)
    for widths in ([1, 1, 1, 1, 1], [64], [65], [63, 65, 1, 257, 1], [256, 257, 1]):
        assert nat.bn256_r1cs_solve_launches(ptr(widths), 3, 1) == len(widths)
        assert nat.bn256_r1cs_solve_launches(ptr(widths), 3, nat.R1CS_WIDE_ALL) == 1
        assert nat.bn256_r1cs_solve_launches(ptr(widths), 0, 1) == 0
    # [63] | 65 | [1] | 257 | [1]: the two lone 1-row levels are runs of their own, 257 lies between them
    assert nat.bn256_r1cs_solve_launches(ptr([63, 65, 1, 257, 1]), 2, 64) == 5
    assert nat.bn256_r1cs_solve_launches(ptr([63, 65, 1, 1, 257]), 2, 64) == 4
    assert nat.bn256_r1cs_solve_launches(ptr([63, 65, 1, 257, 1]), 2, 65) == 5
    assert nat.bn256_r1cs_solve_launches(ptr([63, 65, 1, 257, 1]), 2, 66) == 3
    assert nat.bn256_r1cs_solve_launches(ptr([63, 65, 1, 256, 1]), 2, 0) == 1           # the default: 257 rows
    assert nat.bn256_r1cs_solve_launches(ptr([3, 257, 256, 2, 4096]), 2, 0) == 4
