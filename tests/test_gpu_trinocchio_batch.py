"""K Pinocchio proofs from secret-shared witnesses in the exchanges of one (trinocchio.prove_batch, prove_inputs_batch,
Runtime.recombine_points, pynocchio.compute_h_share_batch): the M parties over one LocalHub -
agreement, parity of every proof with the single prover for the deltas recombined from the first exchange,
verification, the number of exchanges whatever K is, masking, a wrong wire in one witness of three with and without the
check, the flow from shares of the inputs, an empty batch, a chunk boundary, the recombination's refusal of a point off
its curve and a batch whose h*g1 shares are infinity, and the h shares against compute_h.  Every comparison is exact.
The helpers follow tests/test_gpu_trinocchio.py."""
import asyncio
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import h_ref as H
from tests import keygen_ref as K
from tests import trinocchio_ref as tr
from tests import witness_share_ref as SR
from tests.test_gpu_pinocchio_h import ALL_TRUE, _deltas, _gen, _qaps, _r1cs_qap, _seeded_td, load_golden, to_ints
from tests.test_gpu_witness_shares import _circuit

pytestmark = pytest.mark.gpu
N = tr.N
PARTIES = [(3, 1), (5, 2)]


@pytest.fixture(scope="module")
def pn():
    import verifiable_mpc_amd as v
    v.get_context()
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def tn(pn):
    from verifiable_mpc_amd import trinocchio
    return trinocchio


@pytest.fixture(scope="module")
def ctx(pn):
    from verifiable_mpc_amd import get_context
    return get_context()


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


@pytest.fixture(scope="module")
def fx():
    return {case["name"]: case for case in load_golden("pinocchio_keygen.json")["cases"]}


class RecordingHub:
    """LocalHub that keeps what every party sent: log[(kind, number)][pid] = value"""

    def __init__(self, tn, parties):
        self.inner, self.log = tn.LocalHub(parties), {}

    async def exchange(self, pid, tag, value):
        self.log.setdefault(tag, {})[pid] = value
        return await self.inner.exchange(pid, tag, value)


def _to_ints(rows):
    return [int.from_bytes(bytes(r), "little") for r in rows]


def _same(proof, other):
    return list(proof) == list(other) and all(type(proof[k]) is type(other[k]) and proof[k] == other[k] for k in proof)


@pytest.fixture(scope="module")
def inputs(pn, fx):
    """name -> (qap, prepared key, verikey, three witnesses as ints), made once.  The fixtures' witnesses come from
    calculate_witness_batch on three input vectors; r64's helper makes one witness per matrix, so it is the same
    witness three times (the tests deal it three times with different polynomials)."""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "r64":
                built = H.satisfiable_r1cs(64, seed=68)         # (the seed: see tests/test_gpu_trinocchio.py)
                assert 0 not in built[2][1]
                qap, cs = _r1cs_qap(pn, built), [built[5]] * 3
                r = random.Random(64)
                td = K.TD(*(r.randrange(N) for _ in range(8)))
            else:
                case_name, form = name.split("/")
                case = fx[case_name]
                qaps = _qaps(pn, case)
                qap = qaps[form]
                cs = [to_ints(row) for row in pn.calculate_witness_batch(qaps["r1cs"], _circuit(case_name)[2])]
                assert cs == _circuit(case_name)[3] and len({tuple(c) for c in cs}) == 3
                td = _seeded_td(pn, case)
            gen = _gen(pn, td)
            cache[name] = (qap, pn.PreparedKey.generate(td, qap, gen), pn.generate_verikey(td, qap, gen), cs)
        return cache[name]
    return get


def _deal(tn, cs, M, t, seed):
    """K witnesses -> per party a (K, n_wires, 32) array of degree-t shares, every witness with polynomials of its own"""
    rng = random.Random(seed)
    dealt = [tn.deal_witness(c, t, M, rng) for c in cs]
    return [np.stack([dealt[w][p] for w in range(len(cs))]) for p in range(M)]


def _run(tn, qap, key, shares, M, t, seed, zk=True, check=True, log=False):
    """the M parties as coroutines over one hub -> (results or exceptions in party order, runtimes, hub)"""
    hub = RecordingHub(tn, M)
    rts = [tn.Runtime(p, M, t, random.Random(1000 * seed + p), hub) for p in range(M)]
    if log:
        for rt in rts:
            rt.stage_log = []

    async def main():
        return await asyncio.gather(*(tn.prove_batch(rts[p], qap, key, shares[p], zk=zk, check=check)
                                      for p in range(M)), return_exceptions=True)
    return asyncio.run(main()), rts, hub


def _recombined_deltas(hub, M, w):
    """from the first exchange: party p's share of a random value is the sum of what the M dealers addressed to it;
    witness w's deltas are the random values 3 w .. 3 w + 2"""
    sent = hub.log[("vec", 1)]
    shares = [[sum(_to_ints(sent[q][p][3 * w:3 * w + 3])[k] for q in range(M)) % N for k in range(3)] for p in range(M)]
    return tuple(tr.recombine([shares[p][k] for p in range(M)]) for k in range(3))


def _agree(results):
    for r in results:
        assert not isinstance(r, Exception), r
    first = results[0]
    for other in results[1:]:
        assert len(other) == len(first)
        for (proof, cc), (op, oc) in zip(first, other):
            assert _same(proof, op) and oc == cc
    return first


# ---- end to end ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Kw", [1, 3])
@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", ["demo/r1cs", "demo/dense", "larger/r1cs", "r64"])
def test_prove_batch_end_to_end(pn, tn, inputs, name, M, t, Kw):
    qap, key, verikey, cs = inputs(name)
    cs = cs[:Kw]
    shares = _deal(tn, cs, M, t, seed=M)
    results, rts, hub = _run(tn, qap, key, shares, M, t, seed=7)
    batch = _agree(results)
    assert len(batch) == Kw
    for w, (proof, c_client) in enumerate(batch):
        c = cs[w]
        assert c_client == [1] + [x % N for x in c[1:qap.out_ix + 1]]
        deltas = _deltas(_recombined_deltas(hub, M, w))                        # parity with the single prover
        assert _same(proof, pn.compute_proof(qap, c, pn.compute_h(qap, c, deltas), key, deltas)), w
    assert pn.verify_batch(qap, verikey, [p for p, _ in batch], [cc for _, cc in batch]) == [ALL_TRUE] * Kw
    assert [rt.exchanges for rt in rts] == [4] * M and len(hub.log) == 4


@pytest.mark.parametrize("Kw", [1, 3])
def test_exchanges_and_stages_do_not_grow_with_the_batch(tn, inputs, Kw):
    qap, key, verikey, cs = inputs("demo/r1cs")
    shares = _deal(tn, cs[:Kw], 3, 1, seed=9)
    for zk, check, want in [(True, True, 4), (False, True, 4), (True, False, 2), (False, False, 2)]:
        results, rts, hub = _run(tn, qap, key, shares, 3, 1, seed=3, zk=zk, check=check, log=True)
        _agree(results)
        assert [rt.exchanges for rt in rts] == [want] * 3 and len(hub.log) == want
        names = [name for name, _ in rts[0].stage_log]
        assert names.count("recombine") == 1 and names.count("proof_share") == 1
        assert names.count("residual") == (1 if check else 0)


@pytest.mark.parametrize("M,t", PARTIES)
def test_without_deltas(pn, tn, inputs, M, t):
    """zk=False: the no-delta single prover's proofs; two runs that differ only in the parties' randomness send different
    h*g1 shares (each masked by a fresh sharing of zero) and end in the same proofs"""
    qap, key, verikey, cs = inputs("larger/r1cs")
    shares = _deal(tn, cs, M, t, seed=M)
    runs = [_run(tn, qap, key, shares, M, t, seed=s, zk=False, check=False) for s in (1, 2)]
    sent = []
    for results, rts, hub in runs:
        batch = _agree(results)
        for w, (proof, _) in enumerate(batch):
            assert _same(proof, pn.compute_proof(qap, cs[w], pn.compute_h(qap, cs[w]), key)), w
        tag = [k for k in hub.log if k[0] == "pts"]
        assert len(tag) == 1
        at = list(batch[0][0]).index("h*g1")
        sent.append([[hub.log[tag[0]][p][0][8 * w + at] for w in range(3)] for p in range(M)])
    assert all(sent[0][p][w] != sent[1][p][w] for p in range(M) for w in range(3))


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("zk", [True, False])
def test_one_wrong_wire_in_witness_1_of_3(pn, tn, inputs, M, t, zk):
    qap, key, verikey, cs = inputs("larger/r1cs")
    bad = list(cs[1])
    wire = list(qap.indices_mid)[len(qap.indices_mid) // 2]
    bad[wire] = (bad[wire] + 1) % N
    shares = _deal(tn, [cs[0], bad, cs[2]], M, t, seed=M)
    results, rts, hub = _run(tn, qap, key, shares, M, t, seed=5, zk=zk, check=True)
    for r in results:                                                         # every party, the same error
        assert isinstance(r, ValueError) and str(r) == "inconsistent shares: witness 1", r
    assert not [k for k in hub.log if k[0] == "pts"]                          # before any proof share is exchanged
    results, rts, hub = _run(tn, qap, key, shares, M, t, seed=5, zk=zk, check=False)
    batch = _agree(results)
    verdicts = pn.verify_batch(qap, verikey, [p for p, _ in batch], [cc for _, cc in batch])
    assert verdicts[0] == ALL_TRUE and verdicts[2] == ALL_TRUE and verdicts[1]["H"] is False


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", ["demo", "larger"])
def test_prove_inputs_batch(pn, tn, inputs, name, M, t):
    qap, key, verikey, _ = inputs(name + "/r1cs")
    r1cs, n_in, xs, want = _circuit(name)
    rng = random.Random(M)
    shared = [SR.share(x, t, M, rng) for x in xs]
    batch_in = [np.stack([K.to_array(shared[w][p]) for w in range(3)]) for p in range(M)]
    hub = RecordingHub(tn, M)
    rts = [tn.Runtime(p, M, t, random.Random(70 + p), hub) for p in range(M)]

    async def main():
        return await asyncio.gather(*(tn.prove_inputs_batch(rts[p], qap, key, batch_in[p]) for p in range(M)))
    batch = _agree(asyncio.run(main()))
    assert [cc for _, cc in batch] == [[1] + want[w][1:qap.out_ix + 1] for w in range(3)]
    assert pn.verify_batch(qap, verikey, [p for p, _ in batch], [cc for _, cc in batch]) == [ALL_TRUE] * 3
    assert [rt.exchanges for rt in rts] == [pn.ShareSolvePlan(qap, n_in).n_rounds + 4] * M


def test_empty_batch(tn, inputs):
    qap, key, verikey, cs = inputs("demo/r1cs")
    hub = RecordingHub(tn, 3)
    rt = tn.Runtime(0, 3, 1, random.Random(1), hub)
    assert asyncio.run(tn.prove_batch(rt, qap, key, np.zeros((0, len(cs[0]), 32), np.uint8))) == []
    assert asyncio.run(tn.prove_inputs_batch(rt, qap, key, np.zeros((0, 1, 32), np.uint8))) == []
    assert rt.exchanges == 0 and not hub.log


def test_a_chunk_boundary_changes_no_proof(pn, tn, inputs, monkeypatch):
    qap, key, verikey, cs = inputs("larger/r1cs")
    shares = _deal(tn, cs, 3, 1, seed=4)
    whole = _agree(_run(tn, qap, key, shares, 3, 1, seed=8)[0])
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", 1)
    assert pn.batch_ranges(qap, 3) == [(0, 1), (1, 2), (2, 3)]
    cut = _agree(_run(tn, qap, key, shares, 3, 1, seed=8)[0])
    assert all(_same(a, b) and ca == cb for (a, ca), (b, cb) in zip(whole, cut))


# ---- the recombination -------------------------------------------------------------------------------------------------

def test_recombine_points_refuses_a_point_off_the_curve(pn, tn, nat, inputs):
    qap, key, verikey, cs = inputs("demo/r1cs")
    rt = tn.Runtime(0, 3, 1, random.Random(1), tn.LocalHub(3), ctx=key.ctx)
    g1, g2 = pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2)
    good = rt.recombine_points([[g1, g2, pn.BN256Point(None)]] * 3, key.ctx)
    assert good == [g1, g2, pn.BN256Point(None)]                              # the weights sum to 1
    off = pn.BN256Point((1, 1))
    with pytest.raises(nat.VmpcError) as e:
        rt.recombine_points([[g1, g2], [off, g2], [g1, g2]], key.ctx)
    assert e.value.code == nat.E_NOTONCURVE
    with pytest.raises(ValueError, match="differ"):
        rt.recombine_points([[g1, g2], [g2, g1], [g1, g2]], key.ctx)


def test_a_batch_whose_h_shares_are_infinity(pn, tn):
    """d = 1 without deltas: h is empty, every party's h*g1 share is the point at infinity, nothing is dealt"""
    built = H.satisfiable_r1cs(1, seed=5)
    qap, c = _r1cs_qap(pn, built), built[5]
    r = random.Random(11)
    td = K.TD(*(r.randrange(N) for _ in range(8)))
    key = pn.PreparedKey.generate(td, qap, _gen(pn, td))
    shares = _deal(tn, [c, c], 3, 1, seed=2)
    results, rts, hub = _run(tn, qap, key, shares, 3, 1, seed=1, zk=False, check=False)
    batch = _agree(results)
    single = pn.compute_proof(qap, c, pn.compute_h(qap, c), key)
    assert single["h*g1"].coords is None
    assert all(_same(proof, single) for proof, _ in batch)
    at = list(single).index("h*g1")
    (tag,) = hub.log
    assert tag[0] == "pts" and [rt.exchanges for rt in rts] == [1] * 3
    assert all(hub.log[tag][p][0][8 * w + at] == (1, bytes(64)) for p in range(3) for w in range(2))


# ---- h on K share vectors ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("d", [1, 2, 3, 64, 257])
def test_h_share_batch(pn, ctx, d, M, t):
    """one witness shared three times with different polynomials: every party's K results are compute_h_share's, and the
    M parties' results recombine to compute_h, without deltas and with them (K objects, and a device buffer of 3 K)"""
    built = H.satisfiable_r1cs(d, seed=2000 + d)
    qap, c = _r1cs_qap(pn, built), built[5]
    rng = random.Random(10 * d + M)
    Kw = 3
    vec = [tr.share_vector(c, t, M, rng) for _ in range(Kw)]                  # vec[w][p]
    dls = [tuple(rng.randrange(N) for _ in range(3)) for _ in range(Kw)]
    dsh = [tr.share_vector(dl, t, M, rng) for dl in dls]
    got0, got1 = [], []
    for p in range(M):
        arr = np.stack([K.to_array(vec[w][p]) for w in range(Kw)])
        h0 = pn.compute_h_share_batch(qap, arr)
        h1 = pn.compute_h_share_batch(qap, [vec[w][p] for w in range(Kw)], [_deltas(dsh[w][p]) for w in range(Kw)])
        buf = ctx.upload(K.to_array([x for w in range(Kw) for x in dsh[w][p]]))
        h2 = pn.compute_h_share_batch(qap, arr, buf)
        assert [len(h) for h in h0] == [max(d - 1, 0)] * Kw and [len(h) for h in h1] == [d + 1] * Kw
        for w in range(Kw):
            assert h0[w].coeffs == pn.compute_h_share(qap, vec[w][p]).coeffs, (p, w)
            assert h1[w].coeffs == pn.compute_h_share(qap, vec[w][p], _deltas(dsh[w][p])).coeffs == h2[w].coeffs, (p, w)
        got0.append([h.coeffs for h in h0])
        got1.append([h.coeffs for h in h1])
    want0 = pn.compute_h(qap, c).coeffs
    for w in range(Kw):
        assert [tr.recombine([got0[p][w][k] for p in range(M)]) for k in range(max(d - 1, 0))] == want0
        assert [tr.recombine([got1[p][w][k] for p in range(M)]) for k in range(d + 1)] == \
            pn.compute_h(qap, c, _deltas(dls[w])).coeffs
