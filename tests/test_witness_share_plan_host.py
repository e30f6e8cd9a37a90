"""pynocchio.ShareSolvePlan (the host half of the R1CS solve on shares) against the big-int
restatement of tests/witness_share_ref.py: rounds, phases, sub-levels, order and stored entries on the reference-made
fixtures and on generated circuits with prescribed shapes; read-before-write by brute force; check rows; both errors;
the caches.  No device: nothing here creates a context."""
import functools
import re

import numpy as np
import pytest

from tests import witness_ref as WR
from tests import witness_share_ref as SR
from tests.conftest import load_golden

N = WR.N


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


def plan_phases(plan):
    """the plan's positions in solve order: [("L", r, [sub-levels of positions]), ("P", r, positions), ..]"""
    out = []
    for r in range(plan.n_rounds + 1):
        if r:
            out.append(("P", r, list(range(*plan.round_rows(r)))))
        levels = range(int(plan.phase_ptr[r]), int(plan.phase_ptr[r + 1]))
        out.append(("L", r, [list(range(int(plan.local_level_ptr[k]), int(plan.local_level_ptr[k + 1]))) for k in levels]))
    return out


def assert_same_plan(plan, r1cs, n_in):
    ph, checks = SR.phases(r1cs, n_in)
    mine = plan_phases(plan)
    assert plan.n_rounds == len(SR.round_widths(ph)) and plan.n_checks == checks
    assert [p[:2] for p in mine] == [p[:2] for p in ph]
    assert plan.round_ptr.tolist() == [0] + list(np.cumsum(SR.round_widths(ph), dtype=np.int64))
    assert plan.phase_ptr.tolist() == [0] + list(np.cumsum(SR.local_depths(ph), dtype=np.int64))
    assert len(plan.phase_ptr) == plan.n_rounds + 2 and len(plan.round_ptr) == plan.n_rounds + 1
    assert len(plan.row) == len(r1cs[0]) - checks == plan.n_linear + int(plan.round_ptr[-1])
    assert plan.local_level_ptr[0] == 0 and plan.local_level_ptr[-1] == plan.n_linear
    flat = lambda body, what: [body] if what == "P" else body
    for (what, r, got), (_, _, want) in zip(mine, ph):
        assert [len(x) for x in flat(got, what)] == [len(x) for x in flat(want, what)], (what, r)
        for pos_level, want_level in zip(flat(got, what), flat(want, what)):
            for i, x in zip(pos_level, want_level):
                assert (int(plan.row[i]), int(plan.kind[i]), int(plan.wire[i]), plan.inv[i]) == \
                    (x["row"], x["kind"], x["wire"], x["inv"]), (what, r, i)
                for k, name in enumerate("VWY"):
                    ptr, col, vals = plan.csr[name]
                    assert dict(zip(col[ptr[i]:ptr[i + 1]], vals[ptr[i]:ptr[i + 1]])) == x["mats"][k]
                    assert ptr[i + 1] - ptr[i] == len(x["mats"][k])
    return ph


def assert_reads_follow_writes(plan):
    """brute force: every wire is defined exactly once, and every stored entry of a row is wire 0, an input, or a wire
    that an EARLIER phase or sub-level defined"""
    known = set(range(plan.n_in + 1))
    for what, r, body in plan_phases(plan):
        for level in ([body] if what == "P" else body):
            assert level, (what, r)                                            # no empty round, no empty sub-level
            for i in level:
                for name in "VWY":
                    ptr, col, _ = plan.csr[name]
                    assert set(col[ptr[i]:ptr[i + 1]]) <= known, (what, r, i, name)
            new = [int(plan.wire[i]) for i in level]
            assert len(set(new)) == len(new) and not set(new) & known
            known |= set(new)
    if plan.n_checks == 0:
        assert known == set(range(plan.m + 1))


@functools.lru_cache(maxsize=None)
def _cases():
    return {c["name"]: c for c in load_golden("pinocchio_keygen.json")["cases"]}


@pytest.mark.parametrize("name,widths,linear,levels", [("demo", [2, 1], 4, 6), ("larger", [5, 3, 2, 3, 1, 2, 1], 14, 19)])
def test_fixture_rounds(pn, name, widths, linear, levels):
    case = _cases()[name]
    r = case["r1cs"]
    n_in = len(case["inputs"])
    qap = pn.R1CSQAP(r["V"], r["W"], r["Y"], case["out_ix"], m=case["m"])
    plan = pn.ShareSolvePlan(qap, n_in)
    assert pn.SolvePlan(qap, n_in).n_levels == levels
    assert plan.n_rounds == len(widths) and np.diff(plan.round_ptr).tolist() == widths
    assert plan.n_linear == linear and plan.n_checks == 0
    assert_same_plan(plan, WR.from_dense(case), n_in)
    assert_reads_follow_writes(plan)


@pytest.mark.parametrize("widths,local", [([1], [0, 0]), ([65, 1, 257], [3, 0, 2, 1]), ([2, 2], [1, 3, 0]),
                                          ([63, 64, 256], [0, 1, 0, 2]), ([3, 1, 4, 1, 5], [2, 2, 2, 2, 2, 2])])
def test_generated_circuits_give_their_prescribed_widths(pn, widths, local):
    r1cs = SR.share_layered_r1cs(widths, local, seed=sum(widths) + sum(local))
    plan = pn.ShareSolvePlan(qap_of(pn, r1cs, 2), 2)
    assert np.diff(plan.round_ptr).tolist() == widths and np.diff(plan.phase_ptr).tolist() == local
    assert_same_plan(plan, r1cs, 2)
    assert_reads_follow_writes(plan)
    if len(plan.row) > 4:
        assert plan.row.tolist() != sorted(plan.row.tolist())                 # shuffled rows: the plan had to reorder


def test_witness_ref_circuits_with_products_only(pn):
    """tests/witness_ref.layered_r1cs with KIND_Y rows alone: constant W sides make some rows linear, the rest products"""
    r1cs = WR.layered_r1cs([5, 3, 7, 2], seed=17, kinds=(WR.KY,), checks=3)
    plan = pn.ShareSolvePlan(qap_of(pn, r1cs, 2), 2)
    ph = assert_same_plan(plan, r1cs, 2)
    assert_reads_follow_writes(plan)
    assert plan.n_checks == 3 and len(plan.row) == 17
    assert plan.n_rounds >= 1 and sum(SR.local_depths(ph)) >= 1


def test_linear_only_circuit_has_no_round(pn):
    r1cs = SR.share_layered_r1cs([], [4], seed=8)
    plan = pn.ShareSolvePlan(qap_of(pn, r1cs, 2), 2)
    assert plan.n_rounds == 0 and plan.round_ptr.tolist() == [0] and plan.phase_ptr.tolist() == [0, 4]
    assert_same_plan(plan, r1cs, 2)
    assert_reads_follow_writes(plan)
    # the flattener's `set` row alone: (wire 2 - 5) * 1 = nothing
    plan = pn.ShareSolvePlan(qap_of(pn, ([[(2, 1), (0, -5)]], [[(0, 1)]], [[]], 2), 1), 1)
    assert plan.n_rounds == 0 and plan.kind.tolist() == [pn.KIND_A] and plan.local_level_ptr.tolist() == [0, 1]


def test_check_rows_are_left_out_and_counted(pn):
    """x * x = w2 defines, x * x = 9 checks at once, w2 * w2 = 81 checks a round later"""
    rows = [([(1, 1)], [(1, 1)], [(2, 1)]), ([(1, 1)], [(1, 1)], [(0, 9)]), ([(2, 1)], [(2, 1)], [(0, 81)])]
    r1cs = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], 2)
    qap = qap_of(pn, r1cs, 1)
    plan = pn.ShareSolvePlan(qap, 1)
    assert plan.n_checks == 2 and plan.row.tolist() == [0] and plan.kind.tolist() == [pn.KIND_Y]
    assert plan.n_rounds == 1 and plan.n_linear == 0 and plan.round_rows(1) == (0, 1)
    assert plan.phase_ptr.tolist() == [0, 0, 0] and plan.local_level_ptr.tolist() == [0]
    assert_same_plan(plan, r1cs, 1)


def test_shared_divisor_names_the_constraint(pn):
    r1cs = WR.layered_r1cs([3, 2], seed=12, kinds=(WR.KA,))
    with pytest.raises(SR.SharedDivisor) as e:
        SR.classify(r1cs, 2)
    j = e.value.args[1]
    rows = {x[0] + 1 for level in WR.plan(r1cs, 2) for x in level if x[1] == WR.KA}
    assert j in rows
    with pytest.raises(ValueError, match=r"division by a shared value in constraint (\d+) ") as e:
        pn.ShareSolvePlan(qap_of(pn, r1cs, 2), 2)
    assert int(re.search(r"constraint (\d+) ", str(e.value)).group(1)) in rows
    # a hand-written one: row 2 is wire 3 = x1 / x2
    shared = ([[(1, 1)], [(3, 1)]], [[(1, 1)], [(2, 1)]], [[(4, 1)], [(1, 1)]], 4)
    with pytest.raises(ValueError, match=r"division by a shared value in constraint 2 "):
        pn.ShareSolvePlan(qap_of(pn, shared, 2), 2)
    # the same row with x2 = wire 0 scaled is a division by a constant: linear
    const = ([[(1, 1)], [(3, 1)]], [[(1, 1)], [(0, 7)]], [[(4, 1)], [(1, 1)]], 4)
    plan = pn.ShareSolvePlan(qap_of(pn, const, 2), 2)
    assert plan.n_rounds == 1 and plan.n_linear == 1 and plan.kind.tolist() == [pn.KIND_A, pn.KIND_Y]


def test_zero_constant_divisor_names_the_constraint(pn):
    zero = ([[(1, 1)], [(3, 1)]], [[(1, 1)], [(0, N)]], [[(4, 1)], [(1, 1)]], 4)         # row 2: wire 3 * (n = 0) = x1
    with pytest.raises(ValueError, match=r"division by the constant 0 in constraint 2$"):
        pn.ShareSolvePlan(qap_of(pn, zero, 2), 2)
    with pytest.raises(SR.ZeroDivisor) as e:
        SR.classify(zero, 2)
    assert e.value.args[1] == 2
    empty = ([[(1, 1)], []], [[(1, 1)], [(3, 2)]], [[(4, 1)], [(1, 1)]], 4)              # row 2: 0 * (2 wire 3) = x1, kind B
    with pytest.raises(ValueError, match=r"division by the constant 0 in constraint 2$"):
        pn.ShareSolvePlan(qap_of(pn, empty, 2), 2)


def test_plans_are_cached_apart(pn):
    r1cs = SR.share_layered_r1cs([2, 1], [1, 1, 1], seed=3)
    qap = qap_of(pn, r1cs, 2)
    base = pn.SolvePlan(qap, 2)
    before = (base.level_ptr.copy(), base.row.copy(), base.kind.copy(), list(base.inv),
              {k: tuple(list(x) for x in v) for k, v in base.csr.items()})
    plan = pn.ShareSolvePlan(qap, 2)
    assert pn.ShareSolvePlan(qap, 2) is plan and pn.SolvePlan(qap, 2) is base
    assert set(qap._solve_plans) == {2} and qap._solve_plans[2] is base
    assert qap._share_solve_plans == {2: plan}
    assert np.array_equal(base.level_ptr, before[0]) and np.array_equal(base.row, before[1])
    assert np.array_equal(base.kind, before[2]) and base.inv == before[3]
    assert {k: tuple(list(x) for x in v) for k, v in base.csr.items()} == before[4]


def test_reference_qap_is_solveplans_typeerror(pn):
    class Dense:
        d, m, out_ix, v, w, y, t = 1, 1, 1, [], [], [], None
    with pytest.raises(TypeError, match=r"R1CSQAP\(V, W, Y, out_ix\)"):
        pn.ShareSolvePlan(Dense(), 1)
