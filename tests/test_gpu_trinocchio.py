"""Pinocchio proofs from a secret-shared witness (verifiable_mpc_amd/trinocchio.py, pynocchio.compute_h_share): every
party's h share against the quotient tests/trinocchio_ref.py gives for THAT party's row values (whose remainder is not
zero: the unsatisfied case is what runs), the recombined shares against compute_h on the plain witness, and the
M-party prover end to end over one LocalHub - agreement, parity with the single prover for the recombined deltas,
verification, masking, a wrong wire with and without the check, the degree rule and the number of exchanges.  Every
comparison is exact."""
import asyncio
import random

import pytest

from tests import h_ref as H
from tests import keygen_ref as K
from tests import trinocchio_ref as tr
from tests.test_gpu_pinocchio_h import ALL_TRUE, _case_inputs, _deltas, _gen, _qaps, _r1cs_qap, _seeded_td, load_golden

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
def fx():
    return {case["name"]: case for case in load_golden("pinocchio_keygen.json")["cases"]}


# ---- h on shares -----------------------------------------------------------------------------------------------------

def _check_h_shares(pn, qap, rows_of, c, M, t, seed):
    """rows_of(vector) -> (a, b, y).  Without deltas, then with delta shares against the recombined deltas."""
    d = int(qap.d)
    rng = random.Random(seed)
    shares = tr.share_vector(c, t, M, rng)
    dl = tuple(rng.randrange(N) for _ in range(3))
    dshares = tr.share_vector(dl, t, M, rng)
    got0, got1 = [], []
    for p in range(M):
        h0, rem, V, W, tc = tr.quotient_parts(*rows_of(shares[p]))
        assert any(rem), "this party's rows satisfy the constraints: the test would not exercise the unsatisfied case"
        g0 = pn.compute_h_share(qap, shares[p])
        assert len(g0) == max(d - 1, 0) and g0.coeffs == h0, (p,)
        g1 = pn.compute_h_share(qap, K.to_array(shares[p]), _deltas(dshares[p]))
        assert len(g1) == d + 1 and g1.coeffs == tr.add_zk(h0, V, W, tc, tuple(dshares[p])), (p,)
        got0.append(g0.coeffs)
        got1.append(g1.coeffs)
    assert [tr.recombine([g[k] for g in got0]) for k in range(max(d - 1, 0))] == pn.compute_h(qap, c).coeffs
    assert [tr.recombine([g[k] for g in got1]) for k in range(d + 1)] == pn.compute_h(qap, c, _deltas(dl)).coeffs


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("d", [1, 2, 3, 64, 257])
def test_h_share_random_r1cs(pn, d, M, t):
    built = H.satisfiable_r1cs(d, seed=2000 + d)
    V, W, Y, out_ix, m, c = built
    _check_h_shares(pn, _r1cs_qap(pn, built), lambda v: tuple(H.csr_row_values(Mx, v) for Mx in (V, W, Y)), c, M, t,
                    seed=10 * d + M)


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("form", ["dense", "r1cs"])
@pytest.mark.parametrize("name", ["demo", "larger"])
def test_h_share_fixture(pn, fx, name, form, M, t):
    case = fx[name]
    c, _ = _case_inputs(case)
    _check_h_shares(pn, _qaps(pn, case)[form], lambda v: tuple(H.row_values(case["r1cs"][k], v) for k in "VWY"), c, M, t,
                    seed=M)


def test_h_share_takes_a_device_buffer_of_deltas(pn, ctx, fx):
    case = fx["demo"]
    c, deltas = _case_inputs(case)
    qap = _qaps(pn, case)["r1cs"]
    buf = ctx.upload(K.to_array([deltas.v, deltas.w, deltas.y]))
    assert pn.compute_h_share(qap, c, buf).coeffs == pn.compute_h(qap, c, deltas).coeffs


# ---- end to end ------------------------------------------------------------------------------------------------------

class RecordingHub:
    """LocalHub that keeps what every party sent: log[(kind, number)][pid] = value"""

    def __init__(self, tn, parties):
        self.inner, self.log = tn.LocalHub(parties), {}

    async def exchange(self, pid, tag, value):
        self.log.setdefault(tag, {})[pid] = value
        return await self.inner.exchange(pid, tag, value)


def _to_ints(rows):
    return [int.from_bytes(bytes(r), "little") for r in rows]


@pytest.fixture(scope="module")
def inputs(pn, fx):
    """name -> (qap, prepared key, verikey, witness as ints), made once"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "r64":
                # The reference's verify leaves verikey["r_y*y0*g1"] out of its H check (trinocchio/pynocchio.py:
                # 282-291 sums y over indices_io and the mid wires only), and pynocchio.verify follows it: a circuit
                # whose Y reads the constant wire does not verify under either, whoever made the proof.  The first
                # seed from 64 on whose Y has no entry on wire 0 (64..67 have one) gives a circuit they can accept.
                built = H.satisfiable_r1cs(64, seed=68)
                assert 0 not in built[2][1]
                qap, c = _r1cs_qap(pn, built), built[5]
                r = random.Random(64)
                td = K.TD(*(r.randrange(N) for _ in range(8)))
            else:
                case_name, form = name.split("/")
                case = fx[case_name]
                qap, c = _qaps(pn, case)[form], _case_inputs(case)[0]
                td = _seeded_td(pn, case)
            gen = _gen(pn, td)
            cache[name] = (qap, pn.PreparedKey.generate(td, qap, gen), pn.generate_verikey(td, qap, gen), c)
        return cache[name]
    return get


def _run(tn, qap, key, shares, M, t, seed, zk, check):
    """the M parties as coroutines over one hub -> (results or exceptions in party order, runtimes, hub)"""
    hub = RecordingHub(tn, M)
    rts = [tn.Runtime(p, M, t, random.Random(1000 * seed + p), hub) for p in range(M)]

    async def main():
        return await asyncio.gather(*(tn.prove(rts[p], qap, key, shares[p], zk=zk, check=check) for p in range(M)),
                                    return_exceptions=True)
    return asyncio.run(main()), rts, hub


def _recombined_deltas(hub, M):
    """from the first exchange: party p's share of delta_k is the sum of what the M dealers addressed to it"""
    sent = hub.log[("vec", 1)]
    shares = [[sum(_to_ints(sent[q][p][:3])[k] for q in range(M)) % N for k in range(3)] for p in range(M)]
    return tuple(tr.recombine([shares[p][k] for p in range(M)]) for k in range(3))


def _same(proof, other):
    return list(proof) == list(other) and all(type(proof[k]) is type(other[k]) and proof[k] == other[k] for k in proof)


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", ["demo/r1cs", "demo/dense", "larger/r1cs", "r64"])
def test_prove_end_to_end(pn, tn, inputs, name, M, t):
    qap, key, verikey, c = inputs(name)
    shares = tn.deal_witness(c, t, M, random.Random(M))
    want_client = [1] + [x % N for x in c[1:qap.out_ix + 1]]
    for zk in (True, False):
        results, rts, hub = _run(tn, qap, key, shares, M, t, seed=7, zk=zk, check=True)
        for r in results:
            assert not isinstance(r, Exception), r
        proof, c_client = results[0]
        for other, oc in results[1:]:                                         # agreement
            assert _same(proof, other) and oc == c_client
        assert c_client == want_client
        deltas = _deltas(_recombined_deltas(hub, M)) if zk else None           # parity with the single prover
        single = pn.compute_proof(qap, c, pn.compute_h(qap, c, deltas), key, deltas)
        assert _same(proof, single)
        assert pn.verify(qap, verikey, proof, c_client) == ALL_TRUE
        assert [rt.exchanges for rt in rts] == [4] * M


def test_zk_proofs_differ_and_verify_batch_takes_them(pn, tn, inputs):
    qap, key, verikey, c = inputs("demo/r1cs")
    shares = tn.deal_witness(c, 1, 3, random.Random(3))
    runs = [_run(tn, qap, key, shares, 3, 1, seed=s, zk=True, check=False)[0][0] for s in (1, 2)]
    assert not _same(runs[0][0], runs[1][0])
    assert pn.verify_batch(qap, verikey, [r[0] for r in runs], [r[1] for r in runs]) == [ALL_TRUE, ALL_TRUE]


@pytest.mark.parametrize("M,t", PARTIES)
def test_masking(pn, tn, inputs, M, t):
    """two zk=False runs that differ only in the parties' randomness: different exchanged shares of h*g1 (each is
    masked by a fresh sharing of zero), the same recombined proof"""
    qap, key, verikey, c = inputs("larger/r1cs")
    shares = tn.deal_witness(c, t, M, random.Random(M))
    runs = [_run(tn, qap, key, shares, M, t, seed=s, zk=False, check=False) for s in (1, 2)]
    sent = []
    for results, rts, hub in runs:
        tag = [k for k in hub.log if k[0] == "pts"]
        assert len(tag) == 1
        names = list(results[0][0])
        sent.append([hub.log[tag[0]][p][0][names.index("h*g1")] for p in range(M)])
    assert all(sent[0][p] != sent[1][p] for p in range(M))
    assert _same(runs[0][0][0][0], runs[1][0][0][0])
    assert _same(runs[0][0][0][0], pn.compute_proof(qap, c, pn.compute_h(qap, c), key))


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("zk", [True, False])
def test_one_wrong_wire(pn, tn, inputs, M, t, zk):
    qap, key, verikey, c = inputs("larger/r1cs")
    bad = list(c)
    wire = list(qap.indices_mid)[len(qap.indices_mid) // 2]
    bad[wire] = (bad[wire] + 1) % N
    shares = tn.deal_witness(bad, t, M, random.Random(M))
    results, rts, hub = _run(tn, qap, key, shares, M, t, seed=5, zk=zk, check=True)
    for r in results:                                                         # every party, the same error
        assert isinstance(r, ValueError) and str(r) == "inconsistent shares", r
    assert not [k for k in hub.log if k[0] == "pts"]                          # before any proof share is exchanged
    results, rts, hub = _run(tn, qap, key, shares, M, t, seed=5, zk=zk, check=False)
    proof, c_client = results[0]
    assert pn.verify(qap, verikey, proof, c_client)["H"] is False


@pytest.mark.parametrize("M,t", [(2, 1), (4, 2)])
def test_degree_rule_refuses_before_any_launch(tn, ctx, M, t):
    ctx.profile(True)
    try:
        ctx.profile_read()
        with pytest.raises(ValueError, match="2 t < M"):
            tn.Runtime(0, M, t, random.Random(1), tn.LocalHub(M))
        # the stage log: stages that ran earlier in the process keep their names after a reset, with a count of zero
        assert all(count == 0 for _, count in ctx.profile_read().values())
    finally:
        ctx.profile(False)


@pytest.mark.parametrize("zk,check,want", [(True, True, 4), (False, True, 4), (True, False, 2), (False, False, 2)])
def test_exchanges_per_party(tn, inputs, zk, check, want):
    qap, key, verikey, c = inputs("demo/r1cs")
    shares = tn.deal_witness(c, 1, 3, random.Random(9))
    results, rts, hub = _run(tn, qap, key, shares, 3, 1, seed=3, zk=zk, check=check)
    assert not any(isinstance(r, Exception) for r in results), results
    assert [rt.exchanges for rt in rts] == [want] * 3
    assert len(hub.log) == want                                               # and the hub saw as many tags


def test_runtime_primitives(tn, ctx):
    """random_shares has degree t, zero_shares has degree 2t and opens to zero, output opens a share vector"""
    M, t = 5, 2
    hub = tn.LocalHub(M)
    rts = [tn.Runtime(p, M, t, random.Random(p), hub) for p in range(M)]

    async def party(rt):
        r = await rt.random_shares(3)
        z = await rt.zero_shares(4)
        return r.to_ints(), z.to_ints(), await rt.output(r), await rt.output(z)

    async def main():
        return await asyncio.gather(*(party(rt) for rt in rts))
    res = asyncio.run(main())
    for k in range(3):
        col = [res[p][0][k] for p in range(M)]
        secret = tr.recombine(col)
        assert tr.recombine(col[:t + 1], list(range(1, t + 2))) == secret     # degree t: t + 1 shares suffice
        assert all(res[p][2][k] == secret for p in range(M))
    for k in range(4):
        col = [res[p][1][k] for p in range(M)]
        assert any(col) and tr.recombine(col) == 0
        assert tr.recombine(col[:2 * t], list(range(1, 2 * t + 1))) != 0      # not of a lower degree
        assert all(res[p][3][k] == 0 for p in range(M))
