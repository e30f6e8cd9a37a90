"""The batch Pinocchio prover on the GPU (verifiable_mpc_amd/pynocchio.py compute_h_batch, compute_proof_batch,
prove_batch) over a circuit that every choice of inputs satisfies (tests/pinocchio_batch_ref.py).

The single calls ARE batches of one (compute_h, compute_h_share and compute_proof over a PreparedKey go through the batch
code), so `batch == [single(...)]` compares the code with itself: it pins the wrappers' slicing and lengths and no value.
Every such equality here therefore stands next to an anchor that does not run the code under test (as in
tests/test_gpu_batch_of_one.py): h against the big-int restatement of tests/h_ref.py - moment_h up to d = 65, the O(d)
evaluation identity h_identity_holds above that - and proofs against compute_proof over the evaluation-key DICT of the
same trapdoor, which sums with pynocchio.msm on other kernels."""
import functools
import random
import re

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


def _anchored(rows, coeffs, dl=None):
    """h's coefficients against the CPU, from the row values (a, b, y) alone: the moment formula restated in big ints up to
    d = 65, above it the evaluation identity at one seeded point (tests/h_ref.py); lengths are the caller's to assert"""
    a, b, y = rows
    dt = None if dl is None else (dl.v, dl.w, dl.y)
    if len(a) <= 65:
        return coeffs == H.moment_h(a, b, dt)
    return H.h_identity_holds(a, b, y, coeffs, dt, seed=len(a))


class _HostPoly:
    """h computed on the CPU, as the dict-key compute_proof reads it (len() and .coeffs)"""

    def __init__(self, rows, dl=None):
        self.coeffs = H.moment_h(rows[0], rows[1], None if dl is None else (dl.v, dl.w, dl.y))

    def __len__(self):
        return len(self.coeffs)


def _dict_proof(pn, qap, evalkey, d, c, dl=None):
    """the anchor of every proof here: the dict path of compute_proof (one pynocchio.msm per element) on the CPU's h"""
    return pn.compute_proof(qap, c, _HostPoly(B.rows(_circuit(d), c), dl), evalkey, dl)


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
        assert _anchored(B.rows(_circuit(d), cs[w]), hs[w].coeffs, dls[w] if zk else None), w


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
        rows = [H.row_values(case["r1cs"][k], c) for k in "VWY"]
        hs = pn.compute_h_batch(qap, [c, list(c), K.to_array(c)], dls)
        assert hs[0].coeffs == [TH.h2i(x) for x in case["h"]], (case["name"], form)
        for w in range(3):
            assert hs[w].coeffs == pn.compute_h(qap, c, dls[w]).coeffs, (case["name"], form, w)
            assert _anchored(rows, hs[w].coeffs, dls[w]), (case["name"], form, w)
        h0 = pn.compute_h_batch(qap, [c, c])
        assert len(h0[0]) == case["d"] - 1 and h0[0].coeffs == h0[1].coeffs == pn.compute_h(qap, c).coeffs
        assert _anchored(rows, h0[0].coeffs), (case["name"], form)


def test_h_batch_chunks_change_no_value(pn, monkeypatch):
    d, k = 65, 5
    qap = _qap(pn, d)
    cs = B.witnesses(_circuit(d), k, seed=55)
    dls = _deltas(k, 56)
    want = [h.coeffs for h in pn.compute_h_batch(qap, cs, dls)]
    rows = [B.rows(_circuit(d), c) for c in cs]
    assert all(_anchored(rows[w], want[w], dls[w]) for w in range(k))
    n_wires = len(qap.indices)
    budget = pn.h_batch_bytes(d, n_wires, 0, 2)
    assert pn.plan_chunks(k, budget, lambda n: pn.h_batch_bytes(d, n_wires, 0, n)) == [(0, 2), (2, 4), (4, 5)]
    assert pn.plan_chunks(k, pn.BATCH_BUDGET_BYTES, lambda n: pn.h_batch_bytes(d, n_wires, 0, n)) == [(0, 5)]
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", budget)
    assert [h.coeffs for h in pn.compute_h_batch(qap, cs, dls)] == want
    plain = [h.coeffs for h in pn.compute_h_batch(qap, cs)]
    assert plain == [pn.compute_h(qap, c).coeffs for c in cs]
    assert all(_anchored(rows[w], plain[w]) for w in range(k)) and all(len(h) == d - 1 for h in plain)


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
    assert all(_anchored(B.rows(_circuit(d), cs[w]), good[w].coeffs) for w in range(2))


# ---- compute_proof_batch, prove_batch ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def keyed(pn):
    """the d = 65 circuit with a prepared key, a verification key and the evaluation-key dict of one trapdoor"""
    d = 65
    qap = _qap(pn, d)
    r = random.Random(65)
    td = K.TD(*(r.randrange(N) for _ in range(8)))
    gen = TH._gen(pn, td)
    return qap, pn.PreparedKey.generate(td, qap, gen), pn.generate_verikey(td, qap, gen), pn.generate_evalkey(td, qap, gen)


@pytest.mark.parametrize("zk", [False, True])
def test_proof_batch_against_singles(pn, keyed, zk):
    qap, key, _, evalkey = keyed
    k = 3
    cs = B.witnesses(_circuit(65), k, seed=31)
    dls = _deltas(k, 32) if zk else None
    hs = pn.compute_h_batch(qap, cs, dls)
    want = [pn.compute_proof(qap, cs[w], pn.compute_h(qap, cs[w], dls[w] if zk else None), key, dls[w] if zk else None)
            for w in range(k)]
    got = pn.compute_proof_batch(qap, cs, hs, key, dls)                         # h read in place on the device
    assert len(got) == k and list(got[0]) == list(want[0])
    for w in range(k):
        assert _same(want[w], _dict_proof(pn, qap, evalkey, 65, cs[w], dls[w] if zk else None)), w
        assert _same(got[w], want[w]), w
        assert _same(pn.compute_proof(qap, cs[w], hs[w], key, dls[w] if zk else None), want[w])     # a view, single path
    host = pn.compute_proof_batch(qap, cs, [list(h.coeffs) for h in hs], key, dls)                 # h as host lists
    arrs = pn.compute_proof_batch(qap, np.stack([K.to_array(c) for c in cs]), [K.to_array(h.coeffs) for h in hs], key, dls)
    for w in range(k):
        assert _same(host[w], want[w]) and _same(arrs[w], want[w]), w
    with pytest.raises(ValueError, match="one h"):
        pn.compute_proof_batch(qap, cs, hs[:-1], key, dls)


def test_prove_batch_then_verify_batch(pn, keyed):
    qap, key, verikey, evalkey = keyed
    k = 5
    cs = B.witnesses(_circuit(65), k, seed=41)
    dls = _deltas(k, 42)
    proofs = pn.prove_batch(qap, cs, key, dls)
    assert len(proofs) == k
    assert pn.verify_batch(qap, verikey, proofs, cs) == [ALL_TRUE] * k
    assert _same(proofs[3], pn.compute_proof(qap, cs[3], pn.compute_h(qap, cs[3], dls[3]), key, dls[3]))
    for w in range(k):
        assert _same(proofs[w], _dict_proof(pn, qap, evalkey, 65, cs[w], dls[w])), w
    # witness 1's proof under witness 3's inputs and the other way round: H is the check that reads the IO wires
    swapped = list(proofs)
    swapped[1], swapped[3] = proofs[3], proofs[1]
    res = pn.verify_batch(qap, verikey, swapped, cs)
    for w in range(k):
        assert res[w] == (dict(ALL_TRUE, H=False) if w in (1, 3) else ALL_TRUE), w


# ---- the single calls are batches of one ------------------------------------------------------------------------------------

@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("d", [1, 2, 65, 257])
def test_single_is_batch_of_one(pn, d, zk):
    """every h entry on ONE witness: the same coefficients and length from all five, and those against the CPU.  d: the
    empty window, the first non-empty one, this file's size, a second tile and segment (tests/test_gpu_batch_of_one.py)"""
    qap = _qap(pn, d)
    c = B.witnesses(_circuit(d), 1, seed=300 + d)[0]
    dl = _deltas(1, 301 + d)[0] if zk else None
    dls = [dl] if zk else None
    arr = K.to_array(c)
    got = [pn.compute_h(qap, c, dl),
           pn.compute_h_batch(qap, [c], dls)[0],
           pn.compute_h_batch(qap, arr[None], dls)[0],
           pn.compute_h_share(qap, c, dl),
           pn.compute_h_share_batch(qap, [c], dls)[0]]
    for h in got:
        assert len(h) == (d + 1 if zk else max(d - 1, 0))
    for h, nxt in zip(got, got[1:]):
        assert h.coeffs == nxt.coeffs
    assert _anchored(B.rows(_circuit(d), c), got[0].coeffs, dl)
    assert d < 65 or any(got[0].coeffs)


@pytest.mark.parametrize("zk", [False, True])
def test_single_is_batch_of_one_proofs(pn, keyed, zk):
    """compute_proof and compute_proof_batch of one, h handed over in four forms: eight proofs, each the dict-key proof"""
    qap, key, _, evalkey = keyed
    c = B.witnesses(_circuit(65), 1, seed=365)[0]
    dl = _deltas(1, 366)[0] if zk else None
    want = _dict_proof(pn, qap, evalkey, 65, c, dl)
    h = pn.compute_h(qap, c, dl)
    forms = {"HPoly": h, "batch view": pn.compute_h_batch(qap, [c], [dl] if zk else None)[0],
             "host list": list(h.coeffs), "array": K.to_array(h.coeffs)}
    for name, hf in forms.items():
        assert _same(pn.compute_proof(qap, c, hf, key, dl), want), name
        batch = pn.compute_proof_batch(qap, [c], [hf], key, [dl] if zk else None)
        assert len(batch) == 1 and _same(batch[0], want), name
    assert list(pn.compute_proof(qap, c, h, key, dl)) == list(want)                 # the elements' order too


def test_single_is_batch_of_one_errors(pn, keyed):
    """a violated witness: each entry raises its own message, whole"""
    qap, key, _, _ = keyed
    n_io = _circuit(65)[3]
    c = B.witnesses(_circuit(65), 1, seed=367)[0]
    c[n_io + 1 + 40] = (c[n_io + 1 + 40] + 1) % N             # the wire that constraint 41 defines; no earlier row reads it
    tail = " violates constraint 41 (V(j) W(j) != Y(j) at j = 41)"
    whole = lambda text: "^" + re.escape(text) + "$"
    with pytest.raises(ValueError, match=whole("compute_h: the witness" + tail)):
        pn.compute_h(qap, c)
    with pytest.raises(ValueError, match=whole("compute_h: the witness" + tail)):
        pn.compute_h(qap, K.to_array(c), _deltas(1, 1)[0])
    with pytest.raises(ValueError, match=whole("compute_h_batch: witness 0" + tail)):
        pn.compute_h_batch(qap, [c])
    with pytest.raises(ValueError, match=whole("compute_h_batch: witness 0" + tail)):
        pn.prove_batch(qap, [c], key, _deltas(1, 1))
    # the share entries do not test the constraints: both give the polynomial part of V W / t, the same one
    assert pn.compute_h_share(qap, c).coeffs == pn.compute_h_share_batch(qap, [c])[0].coeffs
    with pytest.raises(ValueError, match=whole("compute_h: the witness has 66 rows, the QAP 68 wires")):
        pn.compute_h(qap, K.to_array(c)[:-2])
    with pytest.raises(ValueError, match=whole("compute_h_batch: witness 0 has 66 rows, the QAP 68 wires")):
        pn.compute_h_batch(qap, [K.to_array(c)[:-2]])


def test_empty_batch(pn, keyed):
    qap, key, verikey, _ = keyed
    assert pn.compute_h_batch(qap, []) == []
    assert pn.compute_h_batch(qap, np.zeros((0, len(qap.indices), 32), np.uint8), []) == []
    assert pn.compute_proof_batch(qap, [], [], key) == []
    assert pn.prove_batch(qap, [], key) == []
    assert pn.prove_batch(qap, [], key, []) == []
