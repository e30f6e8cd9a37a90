"""The batch Pinocchio prover's host side without a GPU: the circuit of tests/pinocchio_batch_ref.py is satisfied by
every witness it makes, the restated moment formula agrees with the naive h on them, and compute_h_batch's pure helpers
- the chunk planner and the normalisation of the witnesses - do what they promise."""
import numpy as np
import pytest

from tests import h_ref as H
from tests import keygen_ref as K
from tests import pinocchio_batch_ref as B


def test_every_witness_satisfies_every_row():
    for d in (1, 2, 17, 65):
        built = B.chain_r1cs(d, seed=d)
        assert 0 not in built[2][1]                     # Y never writes wire 0
        ws = B.witnesses(built, 4, seed=100 + d)
        assert len({tuple(c) for c in ws}) == 4
        for c in ws:
            assert len(c) == built[4] + 1 and c[0] == 1
            a, b, y = B.rows(built, c)
            assert [x * z % H.N for x, z in zip(a, b)] == y


def test_moment_formula_equals_naive_h_on_two_witnesses():
    built = B.chain_r1cs(9, seed=3)
    for c, dl in zip(B.witnesses(built, 2, seed=4), (None, (5, H.N - 2, 11))):
        a, b, y = B.rows(built, c)
        want, rem = H.naive_h(a, b, y, dl)
        assert not any(rem)
        assert H.moment_h(a, b, dl) == want


@pytest.fixture(scope="module")
def pn():
    from verifiable_mpc_amd import pynocchio
    return pynocchio


def test_chunk_planner(pn):
    cost = lambda n: 100 * n + 50               # 100 bytes a witness and an arena of 50
    assert pn.plan_chunks(0, 1000, cost) == []
    assert pn.plan_chunks(7, 1000, cost) == [(0, 7)]                    # one chunk
    assert pn.plan_chunks(9, 950, cost) == [(0, 9)]                     # exact fit
    assert pn.plan_chunks(10, 950, cost) == [(0, 9), (9, 10)]
    assert pn.plan_chunks(5, 250, cost) == [(0, 2), (2, 4), (4, 5)]
    assert pn.plan_chunks(3, 10, cost) == [(0, 1), (1, 2), (2, 3)]      # below one witness: one each, never none
    for k, budget in ((23, 333), (64, 4000), (5, 1)):
        chunks = pn.plan_chunks(k, budget, cost)
        assert chunks[0][0] == 0 and chunks[-1][1] == k
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(hi > lo and (hi - lo == 1 or cost(hi - lo) <= budget) for lo, hi in chunks)


def test_witness_normalisation(pn):
    built = B.chain_r1cs(5, seed=8)
    n_wires = built[4] + 1
    ws = B.witnesses(built, 3, seed=9)
    want = np.stack([K.to_array(c) for c in ws])
    got = pn.witness_batch_array(n_wires, ws)
    assert got.shape == (3, n_wires, 32) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(pn.witness_batch_array(n_wires, want), want)                       # the array as it is
    assert np.array_equal(pn.witness_batch_array(n_wires, [K.to_array(c) for c in ws]), want)
    shifted = [[x - H.N if i % 2 else x + H.N for i, x in enumerate(c)] for c in ws]         # reduced as compute_h does
    assert np.array_equal(pn.witness_batch_array(n_wires, shifted), want)
    assert pn.witness_batch_array(n_wires, []).shape == (0, n_wires, 32)
    with pytest.raises(ValueError, match="rows"):
        pn.witness_batch_array(n_wires, want[:, :-1])
    with pytest.raises(ValueError, match="witness 1 "):
        pn.witness_batch_array(n_wires, [ws[0], ws[1][:-1], ws[2]])
    with pytest.raises(ValueError, match="witness 2 "):
        pn.witness_batch_array(n_wires, [want[0], want[1], want[2][:-1]])
