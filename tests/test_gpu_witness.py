"""Pinocchio witnesses on the GPU (verifiable_mpc_amd/pynocchio.py calculate_witness, calculate_witness_batch,
prove_batch_inputs; csrc/bn256_r1cs_solve.hip): every witness against the big-int restatement of tests/witness_ref.py,
exactly - on the reference-made fixture, on layered circuits whose level widths sit at the wave and workgroup edges
under every launch schedule (the schedules must agree byte for byte: one kernel walks levels behind a barrier, the other
gets a launch per level), on tests/pinocchio_batch_ref.chain_r1cs, with strides, unreduced inputs, failing rows and
chunks, and end to end into proofs that verify."""
import ctypes
import functools
import random

import numpy as np
import pytest

from tests import h_ref as H
from tests import keygen_ref as K
from tests import pinocchio_batch_ref as B
from tests import test_gpu_pinocchio_h as TH
from tests import witness_ref as WR
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N = K.N
ALL_TRUE = {k: True for k in "HVWYZ"}


@pytest.fixture(scope="module")
def pn():
    import verifiable_mpc_amd as v
    v.get_context()
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def ctx(pn):
    from verifiable_mpc_amd import get_context
    return get_context()


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


def qap_of(pn, r1cs, out_ix):
    V, W, Y, m = r1cs
    return pn.R1CSQAP(WR.csr(V), WR.csr(W), WR.csr(Y), out_ix, m=m)


def raw_solve(pn, ctx, qap, inputs, wide_rows, pad=0, fill=0):
    """the C entry itself: inputs (K, n_in) ints or a (K, n_in, 32) array -> ((K, m + 1 + pad, 32) bytes as the device
    left them, the K status words); the slots that the caller does not fill hold `fill` bytes"""
    arr = pn._input_rows(inputs)
    k, n_in = arr.shape[:2]
    plan = pn.SolvePlan(qap, n_in)
    stride = qap.m + 1 + pad
    host = np.full((k, stride, 32), fill, np.uint8)
    host[:, 1:n_in + 1] = arr
    dc, bad = ctx.upload(host), ctx.alloc(4 * k)
    ctx.bn256_r1cs_solve_batch(plan.device(ctx)[0], plan.level_ptr, n_in, qap.m, dc.ptr, stride, k, wide_rows, bad.ptr)
    ctx.sync()
    return ctx.download(dc.ptr, host.nbytes).reshape(host.shape), ctx.download(bad.ptr, 4 * k).view("<u4")


def to_bytes(cs):
    return np.stack([K.to_array(c) for c in cs])


# ---- the fixture ------------------------------------------------------------------------------------------------------------

def test_fixture_witnesses(pn):
    for case in load_golden("pinocchio_keygen.json")["cases"]:
        qap = TH._qaps(pn, case)["r1cs"]
        c = pn.calculate_witness(qap, case["inputs"])
        assert c == [TH.h2i(x) for x in case["c"]], case["name"]
        assert c[0] == 1 and c[1:1 + len(case["inputs"])] == case["inputs"]


def test_fixture_batch_of_other_inputs(pn):
    rng = random.Random(31)
    for case in load_golden("pinocchio_keygen.json")["cases"]:
        qap = TH._qaps(pn, case)["r1cs"]
        n_in = len(case["inputs"])
        inputs = [case["inputs"], [rng.randrange(N) for _ in range(n_in)], [N - 1 - i for i in range(n_in)]]
        r1cs = WR.from_dense(case)
        want = [WR.solve(r1cs, x) for x in inputs]
        got = pn.calculate_witness_batch(qap, inputs)
        assert got.shape == (3, case["m"] + 1, 32) and got.dtype == np.uint8
        assert np.array_equal(got, to_bytes(want)), case["name"]


# ---- level widths at the wave and workgroup edges, every schedule -------------------------------------------------------------

WIDTHS = ([1, 1, 1, 1, 1], [64], [65], [63, 65, 1, 257, 1], [256, 257, 1])
KS = (1, 2, 3, 65)


@functools.lru_cache(maxsize=None)
def _layered(widths):
    """(r1cs, 65 input pairs, their 65 witnesses as bytes): computed once, shared, never changed"""
    r1cs = WR.layered_r1cs(list(widths), seed=100 + sum(widths))
    rng = random.Random(sum(widths))
    inputs = [[rng.randrange(N), rng.randrange(N)] for _ in range(max(KS))]
    levels = WR.plan(r1cs, 2)
    assert WR.level_widths(levels) == list(widths)
    want = to_bytes([WR.solve(r1cs, x, levels) for x in inputs])
    want.setflags(write=False)
    return r1cs, inputs, want


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "-".join(map(str, w)))
def test_level_widths_under_every_schedule(pn, ctx, nat, widths):
    """K in 1, 2, 3, 65 x wide_rows in 1, 64, 65, SIZE_MAX, 0: every witness of every combination is held against the
    restatement (so the combinations are byte-identical among themselves) - none is left unverified.  This is the test
    that fails if the run kernel reads a wire before the level that writes it has finished, or if the two kernels round a
    row differently."""
    r1cs, inputs, want = _layered(tuple(widths))
    qap = qap_of(pn, r1cs, 2)
    plan = pn.SolvePlan(qap, 2)
    assert (plan.level_ptr[1:] - plan.level_ptr[:-1]).tolist() == list(widths)
    unverified = 0
    for k in KS:
        for wide in (1, 64, 65, nat.R1CS_WIDE_ALL, 0):
            got, bad = raw_solve(pn, ctx, qap, inputs[:k], wide)
            assert (bad == 0xFFFFFFFF).all(), (k, wide)
            for w in range(k):
                unverified += not np.array_equal(got[w], want[w])
            assert np.array_equal(got, want[:k]), (k, wide)
            assert np.array_equal(pn.calculate_witness_batch(qap, inputs[:k], wide_rows=wide), want[:k])
        assert nat.bn256_r1cs_solve_launches(plan.level_ptr, k, 1) == len(widths)
        assert nat.bn256_r1cs_solve_launches(plan.level_ptr, k, nat.R1CS_WIDE_ALL) == 1
    assert unverified == 0


def test_launch_count_of_the_mixed_widths(pn, nat):
    """[63, 65, 1, 257, 1] at wide_rows = 64: one launch for the run [63], one each for 65 and 257, and one for each of
    the two lone 1-row levels - they are runs of their own because 257 lies between them.  FIVE launches by the
    scheduling rule (a launch per wide level, one per maximal run of consecutive narrower levels).  The request that
    introduced the solver quoted 4 for this very example while listing these same five terms; 5 is what its rule gives."""
    r1cs, _, _ = _layered((63, 65, 1, 257, 1))
    plan = pn.SolvePlan(qap_of(pn, r1cs, 2), 2)
    assert nat.bn256_r1cs_solve_launches(plan.level_ptr, 3, 64) == 5


def test_stride_and_sentinels(pn, ctx):
    r1cs, inputs, want = _layered((63, 65, 1, 257, 1))
    qap = qap_of(pn, r1cs, 2)
    for wide in (1, 0):
        got, bad = raw_solve(pn, ctx, qap, inputs[:3], wide, pad=3, fill=0xA5)       # c_stride = m + 4
        assert (bad == 0xFFFFFFFF).all()
        assert (got[:, qap.m + 1:] == 0xA5).all()                                    # nothing behind slot m is written
        assert np.array_equal(got[:, :qap.m + 1], want[:3])
        assert all(int.from_bytes(got[w, 0].tobytes(), "little") == 1 for w in range(3))


def test_unreduced_inputs_come_back_canonical(pn):
    """2^256 - 1 and n itself as inputs (n is 0: the circuit is products only, so that no divisor 1 + k c meets it)"""
    r1cs = WR.layered_r1cs([256, 257, 1], seed=9, kinds=(WR.KY,))
    qap = qap_of(pn, r1cs, 2)
    top = (1 << 256) - 1
    raw = np.stack([np.frombuffer(b"".join(v.to_bytes(32, "little") for v in pair), np.uint8).reshape(2, 32)
                    for pair in ([top, N], [N, top], [N + 5, 7])])
    got = pn.calculate_witness_batch(qap, raw)
    reduced = [[top % N, 0], [0, top % N], [5, 7]]
    assert np.array_equal(got, pn.calculate_witness_batch(qap, reduced))
    assert np.array_equal(got, to_bytes([WR.solve(r1cs, x) for x in reduced]))
    assert np.array_equal(got[:, 1:3], to_bytes(reduced))                            # the input slots themselves


# ---- the batch prover's circuit ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 65, 513])
def test_chain_r1cs(pn, ctx, d):
    built = B.chain_r1cs(d, seed=2100 + d)
    V, W, Y, n_io, m = built
    qap = pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), n_io, m=m)
    k = 3
    rng = random.Random(10 * d + k)                                # tests/pinocchio_batch_ref.witnesses' draws
    inputs = [[rng.randrange(N) for _ in range(n_io)] for _ in range(k)]
    want = B.witnesses(built, k, seed=10 * d + k)
    got = pn.calculate_witness_batch(qap, inputs)
    assert np.array_equal(got, to_bytes(want))
    # the row values of these witnesses satisfy every constraint: the batch prover's own check finds nothing
    n_wires = m + 1
    dc, aby, bad = ctx.upload(got), ctx.alloc(32 * 3 * d * k), ctx.alloc(4 * k)
    rows = pn._per_ctx(qap, "rows", ctx, lambda: pn._row_plan(ctx, qap))
    for w in range(k):
        rows.run(dc.ptr + 32 * n_wires * w, n_wires, aby.ptr + 32 * 3 * d * w)
    ctx.bn256_qap_check_batch(aby.ptr, aby.ptr + 32 * d, aby.ptr + 64 * d, 3 * d, d, bad.ptr, k)
    ctx.sync()
    assert (ctx.download(bad.ptr, 4 * k).view("<u4") == 0xFFFFFFFF).all()


# ---- failing rows --------------------------------------------------------------------------------------------------------------

def _division_circuit():
    """row 1: wire 4 = x1 * x1; row 2 has the flattener's `/` shape: V the new wire 3, W the divisor x2, Y the numerator x1"""
    return ([[(1, 1)], [(3, 1)]], [[(1, 1)], [(2, 1)]], [[(4, 1)], [(1, 1)]], 4)


def _check_circuit():
    """row 1: wire 2 = x * x; row 2: x * x = 9, a check row"""
    return ([[(1, 1)], [(1, 1)]], [[(1, 1)], [(1, 1)]], [[(2, 1)], [(0, 9)]], 2)


def test_zero_divisor_names_the_witness_and_the_constraint(pn, ctx):
    r1cs = _division_circuit()
    qap = qap_of(pn, r1cs, 2)
    with pytest.raises(ValueError, match=r"witness 1: division by zero in constraint 2$"):
        pn.calculate_witness_batch(qap, [[12, 4], [5, 0], [7, 7]])
    got, bad = raw_solve(pn, ctx, qap, [[12, 4], [5, N], [7, 7]], 1)                 # the call itself completes
    assert bad.tolist() == [0xFFFFFFFF, 1, 0xFFFFFFFF]
    good = pn.calculate_witness_batch(qap, [[12, 4], [7, 7]])                        # the context goes on working
    assert np.array_equal(good, to_bytes([[1, 12, 4, 3, 144], [1, 7, 7, 1, 49]]))
    with pytest.raises(ValueError, match=r"witness 0: division by zero in constraint 2$"):
        pn.calculate_witness(qap, [1, 0])


def test_violated_check_row_names_the_lowest_witness(pn):
    r1cs = _check_circuit()
    qap = qap_of(pn, r1cs, 1)
    with pytest.raises(ValueError, match=r"witness 0 violates constraint 2 "):
        pn.calculate_witness_batch(qap, [[4], [3], [5]])
    with pytest.raises(ValueError, match=r"witness 2 violates constraint 2 "):
        pn.calculate_witness_batch(qap, [[3], [N - 3], [5]])
    assert np.array_equal(pn.calculate_witness_batch(qap, [[3], [N - 3]]), to_bytes([[1, 3, 9], [1, N - 3, 9]]))


# ---- chunks ----------------------------------------------------------------------------------------------------------------------

def test_chunks_change_no_value(pn, monkeypatch):
    r1cs, inputs, want = _layered((63, 65, 1, 257, 1))
    qap = qap_of(pn, r1cs, 2)
    n_wires = qap.m + 1
    budget = pn.witness_batch_bytes(n_wires, 1)
    assert pn.plan_chunks(5, budget, lambda n: pn.witness_batch_bytes(n_wires, n)) == [(i, i + 1) for i in range(5)]
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", budget)
    assert np.array_equal(pn.calculate_witness_batch(qap, inputs[:5]), want[:5])
    bad = qap_of(pn, _check_circuit(), 1)
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", pn.witness_batch_bytes(3, 2))
    with pytest.raises(ValueError, match=r"witness 3 violates constraint 2 "):       # a later chunk: the index is the batch's
        pn.calculate_witness_batch(bad, [[3], [3], [N - 3], [8], [9]])


# ---- ranges --------------------------------------------------------------------------------------------------------------------

def test_ranges_before_any_pointer(ctx, nat):
    fn, h = ctx.lib.vmpc_bn256_r1cs_solve_batch_dev, ctx.handle
    nil = [None] * 14
    big = nat.BN256_R1CS_MAX_WIT + 1
    # (n_levels, n_in, m, c, c_stride, n_wit, wide_rows, first_bad)
    assert fn(h, *nil, 1, 1, 4, None, 5, big, 0, None) == nat.E_RANGE
    assert fn(h, *nil, 1, 1, 4, None, 4, 1, 0, None) == nat.E_RANGE                  # a stride below m + 1
    assert fn(h, *nil, 1, 1, 4, None, (1 << 31) + 1, 1, 0, None) == nat.E_RANGE
    assert fn(h, *nil, 1, 5, 4, None, 5, 1, 0, None) == nat.E_RANGE                  # n_in > m
    assert fn(h, *nil, 1, 1, 4, None, 5, 0, 0, None) == nat.OK                       # no witness: no launch
    assert fn(h, *nil, 1, 1, 4, None, 5, 1, 0, None) == nat.E_INVAL
    bad = ctx.upload(np.zeros(2, np.uint32))
    assert fn(h, *nil, 0, 1, 4, None, 5, 2, 0, ctypes.c_void_p(bad.ptr)) == nat.OK   # d = 0: the status words only
    ctx.sync()
    assert ctx.download(bad.ptr, 8).view("<u4").tolist() == [0xFFFFFFFF] * 2


# ---- into proofs ---------------------------------------------------------------------------------------------------------------

def test_prove_batch_inputs_end_to_end(pn):
    case = next(c for c in load_golden("pinocchio_keygen.json")["cases"] if c["name"] == "larger")
    qap = TH._qaps(pn, case)["r1cs"]
    td = TH._seeded_td(pn, case)
    gen = TH._gen(pn, td)
    key = pn.PreparedKey.generate(td, qap, gen)
    verikey = pn.generate_verikey(td, qap, gen)
    rng = random.Random(77)
    inputs = [case["inputs"], [rng.randrange(N), rng.randrange(N)], [N - 2, 11]]
    _, deltas = TH._case_inputs(case)
    dls = [deltas] + [TH._deltas([rng.randrange(N) for _ in range(3)]) for _ in range(2)]
    proofs, cs = pn.prove_batch_inputs(qap, inputs, key, dls)
    host = [WR.solve(WR.from_dense(case), x) for x in inputs]
    assert np.array_equal(cs, to_bytes(host))
    want = pn.prove_batch(qap, host, key, dls)
    for w in range(3):
        assert {k: TH._enc(p) for k, p in proofs[w].items()} == {k: TH._enc(p) for k, p in want[w].items()}, w
    assert pn.verify_batch(qap, verikey, proofs, [TH.to_ints(c) for c in cs]) == [ALL_TRUE] * 3
    assert {k: TH._enc(p) for k, p in proofs[0].items()} == dict(case["proof"].items())
