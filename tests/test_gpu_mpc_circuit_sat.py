"""Protocol 8 over a secret-shared witness (verifiable_mpc_amd/mpc_circuit_sat.py, csrc/mpc_share.hip): M parties in one
process on one GPU (LocalHub) produce ONE proof, every party the same, and the UNCHANGED single-party verifiers accept
it.  z is opened in the test and compared with the single prover's z element for element; altered shares are refused;
the degree-t randomness and the device path of the MPC Protocol 5 are pinned on their own."""
import asyncio
import random

import numpy as np
import pytest

from tests import p8_ref as ref
from tests import share_ref as sh
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
ELL = ref.ELL
FIXTURE = load_golden("p8_circuits.json")["cases"]
ALL_TRUE = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True, "pivot_verification": True}
PARTIES = [(1, 0), (3, 1), (5, 2)]


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def mods(vm):
    from verifiable_mpc_amd import circuit_sat_gpu, mpc_ac20, mpc_circuit_sat
    return circuit_sat_gpu, mpc_ac20, mpc_circuit_sat


@pytest.fixture(scope="module")
def crs(vm):
    rng = np.random.default_rng(20153)
    exps = rng.integers(0, 256, size=(1023, 32), dtype=np.uint8)
    exps[:, 31] &= 0x0f
    exps[:, 0] |= 1
    group = vm.EllipticCurve("Ed25519", "projective")
    g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
    # Protocol 2 hashes the generators' text: it needs their projective representatives (the circuits stop at N = 255)
    g_proj = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps[:255]))
    return {"g": g, "g_proj": g_proj, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 0x1234567 * 0x89abcdef + 5),
            "gf": vm.GF(group.order)}


def gens_for(crs, N, key="g"):
    return {"g": crs[key][:N], "h": crs["h"], "k": crs["k"]}


# ---- the circuits under test: name -> (n_x, A, B, O, x) ------------------------------------------------------------------
def rows_of(sc):
    raw = sc.raw_forms()
    return raw["A"], raw["B"], raw["O"]


@pytest.fixture(scope="module")
def circuits(mods):
    cs = mods[0]
    out = {}
    for case in FIXTURE:                                     # the reference-made circuits
        sc = cs.SparseCircuit.from_circuit(ref.circuit_from_fixture(case))
        out["fixture-" + case["name"]] = (sc, sc.pad([ref.untyped(v) % ELL for v in case["x_typed"]]))
    # x^4 as a chain of three gates: depth 3
    A = [({0: 1}, 0), ({1: 1}, 0), ({2: 1}, 0)]
    B = [({0: 1}, 0)] * 3
    sc = ref.sparse(1, A, B, [({3: 1}, 5)])
    assert len(sc.level_ptr) - 1 == 3
    out["chain3"] = (sc, sc.pad([3]))
    rng = random.Random(7)
    A, B, O = ref.random_circuit(rng, 4, 0, 1)               # no multiplication gate at all
    sc = ref.sparse(4, A, B, O)
    out["m0"] = (sc, sc.pad([rng.randrange(ELL) for _ in range(4)]))
    # an inner product of 64 terms, <x[0:64], x[60:124]>: the two windows overlap so that N = 124 + 3 + 128 = 255
    # needs no padding
    A = [({i: 1}, 0) for i in range(64)]
    B = [({60 + i: 1}, 0) for i in range(64)]
    sc = ref.sparse(124, A, B, [({124 + i: 1 for i in range(64)}, 0)])
    assert sc.padding() == 0 and 124 + 3 + 128 == 255
    out["inner64"] = (sc, [rng.randrange(ELL) for _ in range(124)])
    return out


CIRCUIT_NAMES = ["fixture-" + c["name"] for c in FIXTURE] + ["chain3", "m0", "inner64"]


def clear_outputs(sc, x):
    A, B, O = rows_of(sc)
    _, _, gamma = ref.triples(sc.n_x, A, B, x)
    return [ref.row_eval(r, sc.n_x, x, gamma) for r in O], gamma


# ---- M parties in one process -----------------------------------------------------------------------------------------------
class Parties:
    def __init__(self, mpc_ac20, M, t, seed=1):
        calls = self.calls = [0] * M

        class CountingHub(mpc_ac20.LocalHub):
            async def exchange(self, pid, tag, value):
                calls[pid] += 1
                return await super().exchange(pid, tag, value)
        self.M, self.t, self.mpc = M, t, mpc_ac20
        self.hub = CountingHub(M)
        self.rng = random.Random(seed)
        self.rts = [mpc_ac20.PartyRuntime(p, M, t, random.Random(seed * 100 + p), self.hub) for p in range(M)]

    def share(self, values):
        """one SecureVector per party"""
        dealt = self.mpc.deal(values, self.t, self.M, self.rng)
        return [self.mpc.SecureVector.from_shares(dealt[p], self.rts[p]) for p in range(self.M)]

    def run(self, fn, return_exceptions=False):
        """fn(party index, runtime) on every party, concurrently"""
        async def everybody():
            return await asyncio.gather(*[fn(p, rt) for p, rt in enumerate(self.rts)], return_exceptions=return_exceptions)
        loop = asyncio.new_event_loop()
        try:
            return loop.run_until_complete(everybody())
        finally:
            loop.close()

    def opened(self, vectors):
        """the secrets of one SecureVector per party, recombined on the host"""
        cols = [v.sv.to_ints() for v in vectors]
        return [sh.recombine([cols[p][i] for p in range(self.M)]) for i in range(len(cols[0]))]


def same_value(a, b):
    if hasattr(a, "to_affine_bytes"):
        return a.to_affine_bytes() == b.to_affine_bytes()
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_value(u, v) for u, v in zip(a, b))
    if hasattr(a, "coeffs"):
        ca, cb = a.coeffs, b.coeffs
        return (ca.to_ints() if hasattr(ca, "to_ints") else [int(v) % ELL for v in ca]) == \
            (cb.to_ints() if hasattr(cb, "to_ints") else [int(v) % ELL for v in cb]) and \
            int(a.constant) % ELL == int(b.constant) % ELL
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    return int(a) % ELL == int(b) % ELL


# ---- 1. proofs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", CIRCUIT_NAMES)
def test_every_party_returns_the_proof_the_single_verifier_accepts(vm, mods, crs, circuits, name, M, t):
    cs, mpc_ac20, mcs = mods
    sc, x = circuits[name]
    N = len(x) + 3 + 2 * sc.m
    gens, gf = gens_for(crs, N), crs["gf"]
    want_outputs, _ = clear_outputs(sc, x)
    kept = []
    for choice in ("compressed", "compressed", "pivot"):
        gens = gens_for(crs, N, "g" if choice == "compressed" else "g_proj")
        ps = Parties(mpc_ac20, M, t, seed=len(kept) + 1)
        xs = ps.share(x)
        proofs = ps.run(lambda p, rt: mcs.circuit_sat_prover(gens, sc, xs[p], gf, choice, rt=rt))
        for other in proofs[1:]:
            assert other.keys() == proofs[0].keys()
            for key in other:
                assert same_value(other[key], proofs[0][key]), key
        proof = proofs[0]
        assert [int(o) % ELL for o in proof["outputs"]] == want_outputs
        assert cs.circuit_sat_verifier(proof, gens, sc, gf, choice) == ALL_TRUE
        kept.append(proof)
    assert not same_value(kept[0]["z_commitment"], kept[1]["z_commitment"])      # fresh randomness per proof
    assert cs.circuit_sat_verifier_batch(kept[:2], gens_for(crs, N), sc, gf) == [ALL_TRUE, ALL_TRUE]


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", ["fixture-" + FIXTURE[0]["name"], "chain3", "m0", "inner64"])
def test_opened_z_is_the_single_provers_z(vm, mods, crs, circuits, monkeypatch, name, M, t):
    cs, mpc_ac20, mcs = mods
    sc, x = circuits[name]
    ps = Parties(mpc_ac20, M, t)
    xs = ps.share(x)
    got = ps.run(lambda p, rt: mcs._witness_on_device(sc, xs[p], rt))
    z = ps.opened([zr[0] for zr in got])
    r_a, r_b = ps.opened([zr[1] for zr in got])

    class Draws:
        def __init__(self, values):
            self.values = list(values)

        def randrange(self, *a):
            return self.values.pop(0)
    monkeypatch.setattr(cs, "prng", Draws([r_a, r_b]))
    assert z == cs._witness_on_device(sc, x, ELL).to_ints()
    # every party's shares of (r_a, r_b) lie on a polynomial of degree t
    for i in range(2):
        col = [int(zr[1].sv.to_ints()[i]) for zr in got]
        assert all(sh.recombine(col[:t + 1], list(range(1, t + 2)), at=q + 1) == col[q] for q in range(M))


def test_gamma_witness_saves_the_exchanges_per_level(vm, mods, crs, circuits):
    """Exchanges of one party for the compressed pivot: levels (the gates) + 5 (r_a r_b, h, gamma, [z], the y's and
    outputs) in Protocol 8, then 4 + rounds in Protocol 5 (y, A, t, the rounds, z').  Shares of the TRUE gate outputs
    take the `levels` away.  Shares of a WRONG gate output end in ValueError("inconsistent shares") on every party,
    not in a proof: z then carries h(j) != f(j) g(j) at that gate's node, so the degree-2m polynomial h through z's
    2m + 1 values is not f g, and at the random challenge f(c) g(c) = h(c) fails except with probability 2m / l -
    which the parties see themselves when they open y1, y2, y3."""
    cs, mpc_ac20, mcs = mods
    sc, x = circuits["chain3"]
    N = len(x) + 3 + 2 * sc.m
    gens, gf = gens_for(crs, N), crs["gf"]
    rounds = (N + 1).bit_length() - 2
    levels = len(sc.level_ptr) - 1
    _, gamma = clear_outputs(sc, x)
    counts = []
    for gw in (None, gamma):
        ps = Parties(mpc_ac20, 3, 1)
        xs = ps.share(x)
        gs = ps.share(gw) if gw is not None else [None] * 3
        proofs = ps.run(lambda p, rt: mcs.circuit_sat_prover(gens, sc, xs[p], gf, rt=rt, gamma_witness=gs[p]))
        assert cs.circuit_sat_verifier(proofs[0], gens, sc, gf) == ALL_TRUE
        assert len(set(ps.calls)) == 1
        counts.append(ps.calls[0])
    assert counts == [levels + 9 + rounds, 9 + rounds]
    bad = list(gamma)
    bad[1] = (bad[1] + 1) % ELL
    ps = Parties(mpc_ac20, 3, 1)
    xs, gs = ps.share(x), ps.share(bad)
    res = ps.run(lambda p, rt: mcs.circuit_sat_prover(gens, sc, xs[p], gf, rt=rt, gamma_witness=gs[p]), True)
    assert all(isinstance(r, ValueError) and "inconsistent shares" in str(r) for r in res)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def test_an_altered_share_is_refused_by_every_party(vm, mods, crs, circuits):
    cs, mpc_ac20, mcs = mods
    sc, x = circuits["inner64"]
    gens, gf = gens_for(crs, 255), crs["gf"]
    ps = Parties(mpc_ac20, 3, 1)
    dealt = mpc_ac20.deal(x, 1, 3, ps.rng)
    dealt[1][5] = (dealt[1][5] + 1) % ELL                    # x_5 is gate 5's left wire
    xs = [mpc_ac20.SecureVector.from_shares(dealt[p], ps.rts[p]) for p in range(3)]
    res = ps.run(lambda p, rt: mcs.circuit_sat_prover(gens, sc, xs[p], gf, rt=rt), True)
    assert len(res) == 3 and all(isinstance(r, ValueError) and "inconsistent shares" in str(r) for r in res)


def test_two_parties_cannot_multiply_degree_one_sharings(vm, mods, monkeypatch):
    from verifiable_mpc_amd import _native
    cs, mpc_ac20, mcs = mods
    rt = mpc_ac20.PartyRuntime(0, 2, 1)
    a = mpc_ac20.SecureVector.from_shares([1, 2, 3], rt)
    launched = []
    for name in ("share_mul_deal", "share_combine"):
        monkeypatch.setattr(_native.Context, name, lambda self, *args, name=name: launched.append(name))
    with pytest.raises(ValueError, match="2 t < M"):
        asyncio.new_event_loop().run_until_complete(rt.schur_prod(a, a))
    assert launched == []


def test_koe_is_refused(vm, mods, crs, circuits):
    cs, mpc_ac20, mcs = mods
    sc, x = circuits["chain3"]
    ps = Parties(mpc_ac20, 1, 0)
    xs = ps.share(x)
    gens = gens_for(crs, len(x) + 3 + 2 * sc.m)
    with pytest.raises(NotImplementedError):
        ps.run(lambda p, rt: mcs.circuit_sat_prover(gens, sc, xs[p], crs["gf"], "koe", rt=rt))
    with pytest.raises(NotImplementedError):
        ps.run(lambda p, rt: mcs.protocol_8_excl_pivot_prover(gens, sc, xs[p], crs["gf"], True, rt=rt))


# ---- 3. randomness and the SecureVector --------------------------------------------------------------------------------------
def test_random_shares_have_degree_t(vm, mods):
    cs, mpc_ac20, mcs = mods
    ps = Parties(mpc_ac20, 3, 1)
    first = ps.run(lambda p, rt: rt.random_shares(5))
    second = ps.run(lambda p, rt: rt.random_shares(5))
    cols = [v.sv.to_ints() for v in first]
    for i in range(5):
        col = [cols[p][i] for p in range(3)]
        for q in range(3):                                   # any two parties' shares determine the third's
            others = [p for p in range(3) if p != q]
            assert sh.recombine([col[p] for p in others], [p + 1 for p in others], at=q + 1) == col[q]
    assert ps.opened(first) != ps.opened(second) and len(set(ps.opened(first))) == 5
    assert "share" in repr(first[0]) and str(cols[0][0]) not in repr(first[0])


def test_secure_vector_arithmetic_is_linear_in_the_secrets(vm, mods):
    cs, mpc_ac20, mcs = mods
    ps = Parties(mpc_ac20, 3, 1)
    rng = random.Random(3)
    u, v = [rng.randrange(ELL) for _ in range(65)], [rng.randrange(ELL) for _ in range(65)]
    pub = [rng.randrange(ELL) for _ in range(65)]
    us, vs = ps.share(u), ps.share(v)
    L = vm.pivot.AffineForm(vm.ScalarVector.from_ints(pub), 11)

    def opened(fn):
        return ps.opened([fn(us[p], vs[p]) for p in range(3)])
    assert opened(lambda a, b: a + b) == [(x + y) % ELL for x, y in zip(u, v)]
    assert opened(lambda a, b: a - b) == [(x - y) % ELL for x, y in zip(u, v)]
    assert opened(lambda a, b: 7 * a - b * pub + 5) == [(7 * x - y * w + 5) % ELL for x, y, w in zip(u, v, pub)]
    assert opened(lambda a, b: a[3:10].concat(b[60:], [9])) == u[3:10] + v[60:] + [9]
    shares = [us[p].form(L).share for p in range(3)]
    assert sh.recombine(shares) == (sum(w * x for w, x in zip(pub, u)) + 11) % ELL
    assert [int(w) % ELL for w in ps.run(lambda p, rt: rt.output(us[p]))[2]] == u
    prod = ps.run(lambda p, rt: rt.schur_prod(us[p], vs[p]))
    assert ps.opened(prod) == [x * y % ELL for x, y in zip(u, v)]
    with pytest.raises(NotImplementedError):
        us[0] * vs[0]


class Replay:
    """stands in for a runtime's rng: hands out the queued values in order"""

    def __init__(self, values):
        self.values = list(values)

    def randrange(self, *a):
        return self.values.pop(0)


@pytest.mark.parametrize("n1", [8, 1024])
def test_protocol_5_device_path_gives_the_list_paths_proof(vm, mods, crs, n1):
    cs, mpc_ac20, mcs = mods
    n, M, t = n1 - 1, 3, 1
    gens, gf = gens_for(crs, n), crs["gf"]
    rng = random.Random(n1)
    x = [rng.randrange(ELL) for _ in range(n)]
    co = [rng.randrange(ELL) for _ in range(n)]
    gamma = rng.randrange(1, ELL)
    y = gf(sum(c * v for c, v in zip(co, x)) % ELL)
    P = vm.pivot.vector_commitment(vm.ScalarVector.from_ints(x), gamma, gens["g"], gens["h"])
    masks = [[rng.randrange(ELL) for _ in range(n + 1)] for _ in range(M)]      # per party: r, then rho
    dealt = mpc_ac20.deal(x + [gamma], t, M, rng)

    dev = Parties(mpc_ac20, M, t)
    L_dev = vm.pivot.LinearForm(vm.ScalarVector.from_ints(co))
    got = dev.run(lambda p, rt: mpc_ac20.protocol_5_prover(
        gens, P, L_dev, y, mpc_ac20.SecureVector.from_shares(dealt[p][:n], rt), rt.secret(dealt[p][n]), gf, rt=rt,
        transcript="compact", r=mpc_ac20.SecureVector.from_shares(masks[p][:n], rt), rho=rt.secret(masks[p][n])))
    assert vm.compressed_pivot.protocol_5_verifier(gens, P, L_dev, y, got[0], gf, transcript="compact") is True
    assert len(set(dev.calls)) == 1 and dev.calls[0] == 3 + (n1.bit_length() - 2)    # A, t, the rounds, z'

    lst = Parties(mpc_ac20, M, t)
    for p, rt in enumerate(lst.rts):
        rt.rng = Replay(masks[p])
    L_lst = vm.pivot.LinearForm([gf(c) for c in co])
    want = lst.run(lambda p, rt: mpc_ac20.protocol_5_prover(
        gens, P, L_lst, y, [rt.secret(s) for s in dealt[p][:n]], rt.secret(dealt[p][n]), gf, rt=rt,
        transcript="compact"))
    for p in range(M):
        assert got[p].keys() == want[p].keys()
        for key in want[p]:
            assert same_value(got[p][key], want[p][key]), (p, key)
