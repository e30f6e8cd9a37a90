"""Protocol 8 over a secret-shared witness with the knowledge-of-exponent pivot over BN-256 (mpc_circuit_sat.py's branch
for a pp, mpc_koe.py): M parties in one process on one GPU (LocalHub) produce ONE proof, every party
the same bytes, the UNCHANGED circuit_sat_verifier accepts it, and - the proof being a deterministic function of
(x, r_a, r_b, gamma) - it is byte for byte the single prover's under the draws that the test recombines from the parties'
recorded shares.  The exchanges are counted, the gamma_witness path and the NTT modes are run, tampered proofs fail the
check that names what was tampered with, and everything that has to be refused is refused before any exchange.

The circuits are the reference-made ones of tests/golden/p8_circuits.json read at order = n, a circuit without a
multiplication gate, one without an output, and a chain of 130 gates (depth 130: 135 exchanges).  The chain's vector has
1 + 3 + 260 = 264 scalars and its pp 528 points a side, the largest here."""
import asyncio
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import mpc_koe_ref as mref
from tests import p8_field_ref as fref
from tests import p8_ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N = fref.BN_N
F = fref.P8(N)
FIXTURE = load_golden("p8_circuits.json")["cases"]
ALL_TRUE = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True,
            "pivot_verification": {"restriction_arg_check": True, "PRQ_check": True}}
PARTIES = [(1, 0), (3, 1), (5, 2)]


class Replay:
    """stands in for a module's prng: hands out the given draws in order"""

    def __init__(self, draws):
        self.draws = list(draws)

    def randrange(self, *args):
        return self.draws.pop(0)


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def mods(vm):
    from verifiable_mpc_amd import circuit_sat_gpu, knowledge_of_exponent, mpc_ac20, mpc_circuit_sat, mpc_koe
    return SimpleNamespace(cs=circuit_sat_gpu, koe=knowledge_of_exponent, mpc_ac20=mpc_ac20, mcs=mpc_circuit_sat, mk=mpc_koe)


# ---- the circuits under test: name -> (SparseCircuit of order n, x) ---------------------------------------------------
def sparse(mods, n_x, A, B, O):
    return mods.cs.SparseCircuit(n_x, fref.to_csr(A), fref.to_csr(B), fref.to_csr(O), order=N)


@pytest.fixture(scope="module")
def circuits(mods):
    out = {}
    for case in FIXTURE:
        sc = mods.cs.SparseCircuit.from_circuit(p8_ref.circuit_from_fixture(case), order=N)
        out["fixture-" + case["name"]] = (sc, [p8_ref.untyped(v) % N for v in case["x_typed"]])
    rng = random.Random(17)
    A, B, O = F.random_circuit(rng, 4, 0, 1)                 # no multiplication gate at all
    out["m0"] = (sparse(mods, 4, A, B, O), [rng.randrange(N) for _ in range(4)])
    A, B, O = F.random_circuit(rng, 6, 9, 0)                 # no output
    out["out0"] = (sparse(mods, 6, A, B, O), [rng.randrange(N) for _ in range(6)])
    A, B, O = F.random_circuit(rng, 5, 65, 2)                # past VMPC_FR_CS_EXT_NTT_MIN gates
    out["m65"] = (sparse(mods, 5, A, B, O), [rng.randrange(N) for _ in range(5)])
    # x^(2^130) as a chain of 130 squarings: depth 130
    A = [({i: 1}, 0) for i in range(130)]
    sc = sparse(mods, 1, A, A, [({130: 1}, 5)])
    assert sc.m == 130 and len(sc.level_ptr) - 1 == 130
    out["chain130"] = (sc, [3])
    return out


CIRCUIT_NAMES = ["fixture-" + c["name"] for c in FIXTURE] + ["m0", "out0", "m65", "chain130"]


def rows_of(sc):
    raw = sc.raw_forms()
    return raw["A"], raw["B"], raw["O"]


def clear_outputs(sc, x):
    A, B, O = rows_of(sc)
    _, _, gamma = F.triples(sc.n_x, A, B, x)
    return [F.row_eval(r, sc.n_x, x, gamma) for r in O], gamma


_PP = {}


def pp_for(vm, mods, monkeypatch, n_z):
    """a pp for vectors of n_z scalars, made once per length (knowledge_of_exponent.trusted_setup under replayed draws)"""
    if n_z not in _PP:
        rng = random.Random(8000 + n_z)
        monkeypatch.setattr(mods.koe, "prng", Replay([rng.randrange(1, N) for _ in range(3)]))
        _PP[n_z] = mods.koe.trusted_setup(vm.pynocchio.BN256Point(bn.G1), vm.pynocchio.BN256TwistPoint(bn.G2), n_z, N)
    return _PP[n_z]


def n_z_of(sc, x):
    return len(x) + 3 + 2 * sc.m


# ---- M parties in one process ------------------------------------------------------------------------------------------
class Parties:
    def __init__(self, mods, M, t, seed=1):
        calls = self.calls = [0] * M

        class CountingHub(mods.mpc_ac20.LocalHub):
            async def exchange(self, pid, tag, value):
                calls[pid] += 1
                return await super().exchange(pid, tag, value)

        class Recording(mods.mk.Runtime):
            """keeps this party's shares of everything random_shares dealt"""
            async def random_shares(self, n):
                r = await super().random_shares(n)
                self.dealt.append(r.to_ints())
                return r
        self.M, self.t, self.mods = M, t, mods
        self.hub = CountingHub(M)
        self.rng = random.Random(seed)
        self.rts = [Recording(p, M, t, random.Random(seed * 100 + p), self.hub) for p in range(M)]
        for rt in self.rts:
            rt.dealt = []

    def share(self, values):
        """one SharedVector per party"""
        dealt = mref.deal(values, self.t, self.M, self.rng)
        return [self.mods.mk.SharedVector.from_shares(dealt[p], self.rts[p]) for p in range(self.M)]

    def dealt(self, k=0):
        """the secrets of the k-th random_shares call, recombined on the host"""
        return mref.recombine([rt.dealt[k] for rt in self.rts])

    def run(self, fn, return_exceptions=False):
        """fn(party index, runtime) on every party, concurrently"""
        async def everybody():
            return await asyncio.gather(*[fn(p, rt) for p, rt in enumerate(self.rts)], return_exceptions=return_exceptions)
        loop = asyncio.new_event_loop()
        try:
            return loop.run_until_complete(everybody())
        finally:
            loop.close()


def proof_bytes(proof):
    """every value of a proof as canonical bytes"""
    assert sorted(proof) == ["L", "outputs", "pivot_proof", "y1", "y2", "y3", "z_commitment"]
    assert sorted(proof["z_commitment"]) == ["P", "pi"] and sorted(proof["pivot_proof"]) == ["P", "Q", "pi"]
    parts = [proof["z_commitment"][k].to_bytes() for k in ("P", "pi")]
    parts += [proof["pivot_proof"][k].to_bytes() for k in ("P", "pi", "Q")]
    parts += [(int(proof[k]) % N).to_bytes(32, "little") for k in ("y1", "y2", "y3")]
    parts += [(int(v) % N).to_bytes(32, "little") for v in proof["outputs"]]
    parts += [v.to_bytes(32, "little") for v in proof["L"].coeffs.to_ints()]
    parts.append((int(proof["L"].constant) % N).to_bytes(32, "little"))
    return b"".join(parts)


def single_prover(vm, mods, monkeypatch, pp, sc, x, draws, **kw):
    monkeypatch.setattr(mods.cs, "prng", Replay(draws))
    proof = mods.cs.circuit_sat_prover(pp, sc, x, vm.GF(N), "koe", **kw)
    assert mods.cs.prng.draws == []
    return proof


# ---- 1. proofs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", CIRCUIT_NAMES)
def test_every_party_returns_the_single_provers_proof(vm, mods, circuits, monkeypatch, name, M, t):
    sc, x = circuits[name]
    pp, gf = pp_for(vm, mods, monkeypatch, n_z_of(sc, x)), vm.GF(N)
    ps = Parties(mods, M, t)
    xs = ps.share(x)
    proofs = ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt))
    mine = proof_bytes(proofs[0])
    assert all(proof_bytes(other) == mine for other in proofs[1:])
    proof = proofs[0]
    assert [int(o) % N for o in proof["outputs"]] == clear_outputs(sc, x)[0]
    assert type(proof["y1"]) is type(gf(0)) and type(proof["L"].coeffs).__name__ == "BnScalarVector"
    assert mods.cs.circuit_sat_verifier(proof, pp, sc, gf, "koe") == ALL_TRUE
    # D + 5 exchanges for D depth levels: the levels, ONE deal of (r_a, r_b, gamma), h, (P, pi), the y's and outputs, Q and u
    D = len(sc.level_ptr) - 1
    assert ps.calls == [D + 5] * M and [rt.exchanges for rt in ps.rts] == [D + 5] * M
    # the single prover under the recombined draws: the same bytes
    assert all(len(rt.dealt) == 1 and len(rt.dealt[0]) == 3 for rt in ps.rts)
    r_a, r_b, gamma = ps.dealt()
    assert proof_bytes(single_prover(vm, mods, monkeypatch, pp, sc, x, [r_a, r_b, gamma])) == mine


@pytest.mark.parametrize("kind", ["array", "list"])
def test_shares_as_an_array_or_a_list(vm, mods, circuits, monkeypatch, kind):
    sc, x = circuits["fixture-" + FIXTURE[0]["name"]]
    pp, gf = pp_for(vm, mods, monkeypatch, n_z_of(sc, x)), vm.GF(N)
    ps = Parties(mods, 3, 1)
    dealt = mref.deal(x, 1, 3, ps.rng)
    if kind == "array":
        dealt = [np.frombuffer(b"".join(v.to_bytes(32, "little") for v in d), np.uint8).reshape(-1, 32) for d in dealt]
    proofs = ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, dealt[p], gf, "koe", rt=rt))
    assert mods.cs.circuit_sat_verifier(proofs[1], pp, sc, gf, "koe") == ALL_TRUE
    assert proof_bytes(proofs[0]) == proof_bytes(single_prover(vm, mods, monkeypatch, pp, sc, x, ps.dealt()))


def test_gamma_witness_saves_the_exchanges_per_level(vm, mods, circuits, monkeypatch):
    """shares of the TRUE gate outputs: 5 exchanges whatever the depth, the same proof as the single prover's with the
    same gamma_witness; a share of a WRONG gate output: ValueError("inconsistent shares") on every party"""
    sc, x = circuits["chain130"]
    pp, gf = pp_for(vm, mods, monkeypatch, n_z_of(sc, x)), vm.GF(N)
    _, gamma = clear_outputs(sc, x)
    ps = Parties(mods, 3, 1)
    xs, gs = ps.share(x), mref.deal(gamma, 1, 3, ps.rng)
    proofs = ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt, gamma_witness=gs[p]))
    assert ps.calls == [5, 5, 5] and [rt.exchanges for rt in ps.rts] == [5, 5, 5]
    assert mods.cs.circuit_sat_verifier(proofs[0], pp, sc, gf, "koe") == ALL_TRUE
    assert proof_bytes(proofs[0]) == proof_bytes(proofs[2]) == \
        proof_bytes(single_prover(vm, mods, monkeypatch, pp, sc, x, ps.dealt(), gamma_witness=gamma))
    ps = Parties(mods, 3, 1)
    xs, gs = ps.share(x), mref.deal(gamma, 1, 3, ps.rng)
    gs[1][77] = (gs[1][77] + 1) % N
    res = ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt, gamma_witness=gs[p]), True)
    assert len(res) == 3 and all(isinstance(r, ValueError) and "inconsistent shares" in str(r) for r in res), res
    with pytest.raises(ValueError, match="130 gate outputs expected"):
        ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt, gamma_witness=gs[p][:-1]))


def test_an_altered_share_is_refused_by_every_party(vm, mods, monkeypatch):
    """x^4 by two squarings; party 2's share of x is off by one.  The three shares then lie on a polynomial of degree 2,
    their squares on one of degree 4, which three parties do not reduce: gamma_0 is not the square of the x the shares
    recombine to, f(c) g(c) != h(c) except with probability 2m / n, and the parties see it when they open y1, y2, y3"""
    sc = sparse(mods, 1, [({0: 1}, 0), ({1: 1}, 0)], [({0: 1}, 0), ({1: 1}, 0)], [({2: 1}, 0)])
    pp, gf = pp_for(vm, mods, monkeypatch, 1 + 3 + 4), vm.GF(N)
    ps = Parties(mods, 3, 1)
    dealt = mref.deal([3], 1, 3, ps.rng)
    dealt[2][0] = (dealt[2][0] + 1) % N
    res = ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, dealt[p], gf, "koe", rt=rt), True)
    assert len(res) == 3 and all(isinstance(r, ValueError) and "inconsistent shares" in str(r) for r in res), res


@pytest.mark.parametrize("name", ["fixture-" + FIXTURE[0]["name"], "m65"])
def test_ntt_modes_give_the_same_proof_bytes(vm, mods, circuits, monkeypatch, name):
    sc, x = circuits[name]
    pp, gf = pp_for(vm, mods, monkeypatch, n_z_of(sc, x)), vm.GF(N)
    got = []
    for ntt in (False, True):
        ps = Parties(mods, 3, 1, seed=9)                     # the same seeds: the same shares, masks and draws
        xs = ps.share(x)
        run = lambda: ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt))   # noqa: E731
        if ntt:
            with vm.device.cs_extension("ntt"), vm.device.poly_product("ntt"):
                proofs = run()
        else:
            proofs = run()
        got.append(proof_bytes(proofs[0]))
        assert proof_bytes(proofs[1]) == got[-1]
    assert got[0] == got[1]


def test_tampering_fails_the_named_check(vm, mods, circuits, monkeypatch):
    sc, x = circuits["fixture-" + FIXTURE[0]["name"]]
    pp, gf, P = pp_for(vm, mods, monkeypatch, n_z_of(sc, x)), vm.GF(N), vm.pynocchio
    ps = Parties(mods, 3, 1)
    xs = ps.share(x)
    proof = ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt))[0]
    verify = lambda p: mods.cs.circuit_sat_verifier(p, pp, sc, gf, "koe")           # noqa: E731
    assert verify(proof) == ALL_TRUE
    pv = proof["pivot_proof"]
    twice = lambda pt: P.BN256Point(bn.E1.add(pt.coords, pt.coords))               # noqa: E731
    got = verify({**proof, "pivot_proof": {**pv, "Q": twice(pv["Q"])}})
    assert got == {**ALL_TRUE, "pivot_verification": {"restriction_arg_check": True, "PRQ_check": False}}
    got = verify({**proof, "pivot_proof": {**pv, "P": twice(pv["P"])}})
    assert got["y1*y2=y3"] is True and got["L_wellformed_from_Cfgh_forms"] is True
    assert got["pivot_verification"]["restriction_arg_check"] is False
    # the commitment itself: another first challenge, another L
    got = verify({**proof, "z_commitment": {"P": twice(pv["P"]), "pi": pv["pi"]}})
    assert got == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": False}


# ---- 2. refusals: all before any exchange ------------------------------------------------------------------------------
def test_two_t_not_below_m_is_refused(vm, mods, monkeypatch):
    from verifiable_mpc_amd import _native
    launched = []
    for name in ("bn256_share_mul_deal", "bn256_share_combine"):
        monkeypatch.setattr(_native.Context, name, lambda self, *args, name=name: launched.append(name))
    for M, t in ((2, 1), (4, 2), (1, 1)):
        with pytest.raises((ValueError, AssertionError)):
            mods.mk.Runtime(0, M, t)
    rt = mods.mk.Runtime(0, 3, 1)
    rt.threshold = 2                                         # past the constructor: schur_prod still refuses
    a = mods.mk.SharedVector.from_shares([1, 2, 3], rt)
    with pytest.raises(ValueError, match="2 t < M"):
        asyncio.new_event_loop().run_until_complete(rt.schur_prod(a, a))
    assert launched == [] and rt.exchanges == 0
    with pytest.raises(ValueError, match="2 t < M"):
        mods.mk.Runtime(0, 2, 1)


def test_refusals_come_before_any_exchange(vm, mods, circuits, monkeypatch):
    sc, x = circuits["fixture-" + FIXTURE[0]["name"]]
    n_z = n_z_of(sc, x)
    pp, gf = pp_for(vm, mods, monkeypatch, n_z), vm.GF(N)
    ELL = fref.ELL
    raw = sc.raw_forms()
    over_l = mods.cs.SparseCircuit(sc.n_x, *(fref.to_csr(raw[k]) for k in ("A", "B", "O")))

    def refused(error, match, circuit=sc, pp=pp, gf=gf, runtime=None, choice="koe", entry="circuit_sat_prover"):
        ps = Parties(mods, 3, 1)
        xs = ps.share(x)
        rts = runtime or ps.rts
        fn = getattr(mods.mcs, entry)
        args = (choice,) if entry == "circuit_sat_prover" else ()
        with pytest.raises(error, match=match):
            ps.run(lambda p, rt: fn(pp, circuit, xs[p] if runtime is None else x, gf, *args, rt=rts[p]))
        assert ps.calls == [0, 0, 0] and [rt.exchanges for rt in ps.rts] == [0, 0, 0]

    # a runtime over GF(l) with a pp
    gl = [mods.mpc_ac20.PartyRuntime(p, 3, 1, random.Random(p)) for p in range(3)]
    refused(ValueError, "mpc_koe.Runtime", runtime=gl)
    refused(ValueError, "mpc_koe.Runtime", runtime=gl, entry="protocol_8_excl_pivot_prover")
    # wrong orders: _check_field's ValueErrors
    refused(ValueError, "circuit's order", circuit=over_l)
    refused(ValueError, "gf.order", gf=vm.GF(ELL))
    # a pp goes with PivotChoice.koe
    refused(ValueError, "goes with PivotChoice.koe", choice="compressed")
    # a pp of another length, shorter or longer
    refused(ValueError, "takes %d on either side" % (2 * n_z), pp=pp_for(vm, mods, monkeypatch, n_z - 1))
    refused(ValueError, "takes %d on either side" % (2 * n_z), pp=pp_for(vm, mods, monkeypatch, n_z + 1))
    # too few inputs
    ps = Parties(mods, 3, 1)
    xs = ps.share(x[:sc.n_x - 1])
    with pytest.raises(ValueError, match="inputs"):
        ps.run(lambda p, rt: mods.mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt))
    assert ps.calls == [0, 0, 0]


def test_ed25519_generators_keep_refusing_koe(vm, mods, circuits):
    """no pp, no knowledge-of-exponent variant: NotImplementedError as before this branch existed"""
    sc, x = circuits["m0"]
    group = vm.EllipticCurve("Ed25519", "projective")
    gens = {"g": [group.generator], "h": group.generator, "k": group.generator}
    rt = mods.mpc_ac20.PartyRuntime(0, 1, 0)
    loop = asyncio.new_event_loop()
    try:
        with pytest.raises(NotImplementedError):
            loop.run_until_complete(mods.mcs.circuit_sat_prover(gens, sc, x, vm.GF(fref.ELL), "koe", rt=rt))
        with pytest.raises(NotImplementedError):
            loop.run_until_complete(mods.mcs.protocol_8_excl_pivot_prover(gens, sc, x, vm.GF(fref.ELL), True, rt=rt))
    finally:
        loop.close()


# ---- 3. the provers of mpc_koe on their own -----------------------------------------------------------------------------
@pytest.mark.parametrize("M,t", [(3, 1), (5, 2)])
def test_commitment_and_opening_are_the_trapdoors(vm, mods, monkeypatch, M, t):
    """(P, pi, Q) of the M-party provers against the trapdoor's exponents times the generators, u against <L, x> + constant"""
    n = 7
    rng = random.Random(50 + M)
    trapdoor = [rng.randrange(1, N) for _ in range(3)]
    monkeypatch.setattr(mods.koe, "prng", Replay(trapdoor))
    pp = mods.koe.trusted_setup(vm.pynocchio.BN256Point(bn.G1), vm.pynocchio.BN256TwistPoint(bn.G2), n, N)
    trap = fref.KoeTrapdoor(*trapdoor)
    x, gamma = [rng.randrange(N) for _ in range(n)], rng.randrange(1, N)
    co, const = [rng.randrange(N) for _ in range(n)], rng.randrange(N)
    L = vm.pivot.AffineForm(vm.device.BnScalarVector.from_ints(co), vm.GF(N)(const))
    ps = Parties(mods, M, t)
    xs, gs = ps.share(x), mref.deal([gamma], t, M, ps.rng)
    res = ps.run(lambda p, rt: mods.mk.koe_opening_linear_form_prover(L, xs[p], gs[p][0], pp, rt=rt))
    assert ps.calls == [2] * M                               # (P, pi), then Q with the share of u
    P_exp, pi_exp = trap.commitment(x, gamma)
    Q_exp, u_lin = trap.opening(co, x, gamma)
    for proof, u in res:
        assert proof["P"].to_bytes() == bn.g1_to_bytes(bn.E1.mul(P_exp, bn.G1))
        assert proof["pi"].to_bytes() == bn.g2_to_bytes(bn.E2.mul(pi_exp, bn.G2))
        assert proof["Q"].to_bytes() == bn.g1_to_bytes(bn.E1.mul(Q_exp, bn.G1))
        assert u == (u_lin + const) % N
    assert mods.koe.opening_linear_form_verifier(L, pp, res[0][0], res[0][1]) == ALL_TRUE["pivot_verification"]
    with pytest.raises(ValueError, match="as a whole"):
        ps.run(lambda p, rt: mods.mk.koe_restriction_argument_prover(range(n - 1), xs[p], gs[p][0], pp, rt=rt))


def test_schur_prod_and_the_share_vector(vm, mods):
    ps = Parties(mods, 5, 2)
    rng = random.Random(3)
    a, b = [rng.randrange(N) for _ in range(70)], [0, 1, N - 1] + [rng.randrange(N) for _ in range(67)]
    as_, bs = ps.share(a), ps.share(b)
    prods = ps.run(lambda p, rt: rt.schur_prod(as_[p], bs[p]))
    assert ps.calls == [1] * 5
    assert mref.recombine([v.sv.to_ints() for v in prods]) == [x * y % N for x, y in zip(a, b)]
    # degree t again: any t + 1 = 3 parties' shares determine the others'
    col = [v.sv.to_ints()[5] for v in prods]
    for q in (4, 5):
        lag = []
        for i in (1, 2, 3):
            num = den = 1
            for j in (1, 2, 3):
                if j != i:
                    num, den = num * (q - j) % N, den * (i - j) % N
            lag.append(num * pow(den, N - 2, N) % N)
        assert sum(c * s for c, s in zip(lag, col[:3])) % N == col[q - 1]
    # out / dst: results scattered into an existing vector
    outs = [mods.mk.SharedVector.from_shares([7] * 80, rt) for rt in ps.rts]
    dst = [vm.get_context().upload(np.arange(79, 9, -1).astype(np.uint32)) for _ in range(5)]
    ps.run(lambda p, rt: rt.schur_prod(as_[p], bs[p], out=outs[p], dst=dst[p].ptr))
    got = mref.recombine([v.sv.to_ints() for v in outs])
    assert got[:10] == [7] * 10 and got[10:] == [x * y % N for x, y in zip(a, b)][::-1]
    # the wrapper: len, slices (views), form
    v = as_[0]
    assert len(v) == 70 and len(v[3:10]) == 7 and v[3:10].sv.to_ints() == v.sv.to_ints()[3:10] and v[4] == v.sv.to_ints()[4]
    co = [rng.randrange(N) for _ in range(70)]
    L = vm.pivot.AffineForm(vm.device.BnScalarVector.from_ints(co), vm.GF(N)(11))
    assert mref.recombine([[s.form(L)] for s in as_]) == [(sum(c * x for c, x in zip(co, a)) + 11) % N]
