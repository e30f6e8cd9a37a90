"""The batch Pinocchio prover on the GPU (verifiable_mpc_amd/pynocchio.py compute_h_batch, compute_proof_batch,
prove_batch): every result against the single path - K calls of compute_h / compute_proof by the same build, exact - and
against the big-int restatement of tests/h_ref.py, over a circuit that every choice of inputs satisfies
(tests/pinocchio_batch_ref.py)."""
import functools
import random

import numpy as np
import pytest

from tests import h_ref as H
from tests import keygen_ref as K
from tests import pinocchio_batch_ref as B
from tests import test_gpu_pinocchio_h as TH
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


@functools.lru_cache(maxsize=None)
def _circuit(d):
    return B.chain_r1cs(d, seed=2100 + d)


def _qap(pn, d):
    V, W, Y, out_ix, m = _circuit(d)
    return pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), out_ix, m=m)


def _deltas(k, seed):
    rng = random.Random(seed)
    return [TH._deltas([rng.randrange(N) for _ in range(3)]) for _ in range(k)]


def _same(proof, other):
    return {k: TH._enc(p) for k, p in proof.items()} == {k: TH._enc(p) for k, p in other.items()}


# ---- compute_h_batch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("d", [1, 2, 65, 513, 1025])
def test_h_batch_against_singles(pn, d, k, zk):
    qap = _qap(pn, d)
    cs = B.witnesses(_circuit(d), k, seed=10 * d + k)
    dls = _deltas(k, d + k) if zk else None
    hs = pn.compute_h_batch(qap, cs, dls)
    assert len(hs) == k
    assert len({h.buf.base.ptr for h in hs}) == 1               # views into ONE device buffer
    for w in range(k):
        want = pn.compute_h(qap, cs[w], dls[w] if zk else None)
        assert len(hs[w]) == len(want) == (d + 1 if zk else max(d - 1, 0))
        assert hs[w].coeffs == want.coeffs, w


def test_h_batch_against_the_restatement_at_65(pn):
    d, k = 65, 3
    qap = _qap(pn, d)
    cs = B.witnesses(_circuit(d), k, seed=65)
    dls = _deltas(k, 66)
    h0, h1 = pn.compute_h_batch(qap, cs), pn.compute_h_batch(qap, cs, dls)
    for w in range(k):
        a, b, y = B.rows(_circuit(d), cs[w])
        assert h0[w].coeffs == H.moment_h(a, b)
        assert h1[w].coeffs == H.moment_h(a, b, (dls[w].v, dls[w].w, dls[w].y))
    assert any(h0[0].coeffs)


def test_h_batch_lists_against_array(pn):
    d, k = 65, 4
    qap = _qap(pn, d)
    cs = B.witnesses(_circuit(d), k, seed=7)
    dls = _deltas(k, 8)
    want = [h.coeffs for h in pn.compute_h_batch(qap, cs, dls)]
    arr = np.stack([K.to_array(c) for c in cs])
    assert [h.coeffs for h in pn.compute_h_batch(qap, arr, dls)] == want
    assert [h.coeffs for h in pn.compute_h_batch(qap, [arr[0], cs[1], arr[2], tuple(cs[3])], dls)] == want
    shifted = [[x - N if i % 3 == 0 else x + N * (i % 5) for i, x in enumerate(c)] for c in cs]
    assert [h.coeffs for h in pn.compute_h_batch(qap, shifted, dls)] == want
    with pytest.raises(ValueError, match="rows"):
        pn.compute_h_batch(qap, arr[:, :-1], dls)
    with pytest.raises(ValueError, match="deltas"):
        pn.compute_h_batch(qap, cs, dls[:-1])


@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_h_batch_on_the_fixture(pn, form):
    """both QAP forms: the fixture's witness three times, its own deltas first, two other sets after it"""
    for case in load_golden("pinocchio_keygen.json")["cases"]:
        qap = TH._qaps(pn, case)[form]
        c, deltas = TH._case_inputs(case)
        dls = [deltas] + _deltas(2, case["d"])
        hs = pn.compute_h_batch(qap, [c, list(c), K.to_array(c)], dls)
        assert hs[0].coeffs == [TH.h2i(x) for x in case["h"]], (case["name"], form)
        for w in range(3):
            assert hs[w].coeffs == pn.compute_h(qap, c, dls[w]).coeffs, (case["name"], form, w)
        h0 = pn.compute_h_batch(qap, [c, c])
        assert len(h0[0]) == case["d"] - 1 and h0[0].coeffs == h0[1].coeffs == pn.compute_h(qap, c).coeffs


def test_h_batch_chunks_change_no_value(pn, monkeypatch):
    d, k = 65, 5
    qap = _qap(pn, d)
    cs = B.witnesses(_circuit(d), k, seed=55)
    dls = _deltas(k, 56)
    want = [h.coeffs for h in pn.compute_h_batch(qap, cs, dls)]
    n_wires = len(qap.indices)
    budget = pn.h_batch_bytes(d, n_wires, 0, 2)
    assert pn.plan_chunks(k, budget, lambda n: pn.h_batch_bytes(d, n_wires, 0, n)) == [(0, 2), (2, 4), (4, 5)]
    assert pn.plan_chunks(k, pn.BATCH_BUDGET_BYTES, lambda n: pn.h_batch_bytes(d, n_wires, 0, n)) == [(0, 5)]
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", budget)
    assert [h.coeffs for h in pn.compute_h_batch(qap, cs, dls)] == want
    assert [h.coeffs for h in pn.compute_h_batch(qap, cs)] == [pn.compute_h(qap, c).coeffs for c in cs]


def test_h_batch_names_the_lowest_bad_witness(pn):
    """witness 2 of 4 violates constraint 41 first, witness 3 already constraint 1: the error is witness 2's, nothing is
    returned, and the context goes on working"""
    d = 65
    V, W, Y, n_io, m = _circuit(d)
    qap = _qap(pn, d)
    cs = B.witnesses(_circuit(d), 4, seed=90)
    cs[2][n_io + 1 + 40] = (cs[2][n_io + 1 + 40] + 1) % N       # the wire that constraint 41 defines; no earlier row reads it
    cs[3][n_io + 1] = (cs[3][n_io + 1] + 1) % N
    a, b, y = B.rows(_circuit(d), cs[2])
    assert min(j for j in range(d) if (a[j] * b[j] - y[j]) % N) == 40
    hs = None
    with pytest.raises(ValueError, match=r"witness 2 violates constraint 41 "):
        hs = pn.compute_h_batch(qap, cs)
    assert hs is None
    with pytest.raises(ValueError, match=r"witness 3 violates constraint 1 "):
        pn.compute_h_batch(qap, [cs[0], cs[1], cs[0], cs[3]], _deltas(4, 1))
    good = pn.compute_h_batch(qap, cs[:2])
    assert [h.coeffs for h in good] == [pn.compute_h(qap, c).coeffs for c in cs[:2]]


# ---- compute_proof_batch, prove_batch ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def keyed(pn):
    """the d = 65 circuit with a prepared key and a verification key generated from it"""
    d = 65
    qap = _qap(pn, d)
    r = random.Random(65)
    td = K.TD(*(r.randrange(N) for _ in range(8)))
    gen = TH._gen(pn, td)
    return qap, pn.PreparedKey.generate(td, qap, gen), pn.generate_verikey(td, qap, gen)


@pytest.mark.parametrize("zk", [False, True])
def test_proof_batch_against_singles(pn, keyed, zk):
    qap, key, _ = keyed
    k = 3
    cs = B.witnesses(_circuit(65), k, seed=31)
    dls = _deltas(k, 32) if zk else None
    hs = pn.compute_h_batch(qap, cs, dls)
    want = [pn.compute_proof(qap, cs[w], pn.compute_h(qap, cs[w], dls[w] if zk else None), key, dls[w] if zk else None)
            for w in range(k)]
    got = pn.compute_proof_batch(qap, cs, hs, key, dls)                         # h read in place on the device
    assert len(got) == k and list(got[0]) == list(want[0])
    for w in range(k):
        assert _same(got[w], want[w]), w
        assert _same(pn.compute_proof(qap, cs[w], hs[w], key, dls[w] if zk else None), want[w])     # a view, single path
    host = pn.compute_proof_batch(qap, cs, [list(h.coeffs) for h in hs], key, dls)                 # h as host lists
    arrs = pn.compute_proof_batch(qap, np.stack([K.to_array(c) for c in cs]), [K.to_array(h.coeffs) for h in hs], key, dls)
    for w in range(k):
        assert _same(host[w], want[w]) and _same(arrs[w], want[w]), w
    with pytest.raises(ValueError, match="one h"):
        pn.compute_proof_batch(qap, cs, hs[:-1], key, dls)


def test_prove_batch_then_verify_batch(pn, keyed):
    qap, key, verikey = keyed
    k = 5
    cs = B.witnesses(_circuit(65), k, seed=41)
    dls = _deltas(k, 42)
    proofs = pn.prove_batch(qap, cs, key, dls)
    assert len(proofs) == k
    assert pn.verify_batch(qap, verikey, proofs, cs) == [ALL_TRUE] * k
    assert _same(proofs[3], pn.compute_proof(qap, cs[3], pn.compute_h(qap, cs[3], dls[3]), key, dls[3]))
    # witness 1's proof under witness 3's inputs and the other way round: H is the check that reads the IO wires
    swapped = list(proofs)
    swapped[1], swapped[3] = proofs[3], proofs[1]
    res = pn.verify_batch(qap, verikey, swapped, cs)
    for w in range(k):
        assert res[w] == (dict(ALL_TRUE, H=False) if w in (1, 3) else ALL_TRUE), w


def test_empty_batch(pn, keyed):
    qap, key, verikey = keyed
    assert pn.compute_h_batch(qap, []) == []
    assert pn.compute_h_batch(qap, np.zeros((0, len(qap.indices), 32), np.uint8), []) == []
    assert pn.compute_proof_batch(qap, [], [], key) == []
    assert pn.prove_batch(qap, [], key) == []
    assert pn.prove_batch(qap, [], key, []) == []
