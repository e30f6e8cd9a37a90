"""Protocol 8's provers under device.cs_extension("ntt") (csrc/circuit_sat.hip's NTT route): given
the same random draws each prover returns the proof it returns in the default mode, field by field - the single prover,
the batch of K = 3, the M = 3 party prover - and the reference-made fixture circuit is reproduced value for value.  No
caller names the route: they pick it up through the context, and the profile's stage names show that they did."""
import asyncio
import random

import numpy as np
import pytest

from tests import p8_ref as ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ELL = ref.ELL
FIXTURE = load_golden("p8_circuits.json")["cases"]
ALL_TRUE = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True, "pivot_verification": True}


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def cs(vm):
    from verifiable_mpc_amd import circuit_sat_gpu
    return circuit_sat_gpu


@pytest.fixture(scope="module")
def crs(vm):
    """1023 generators, k; a case takes the prefix it needs"""
    rng = np.random.default_rng(20154)
    exps = rng.integers(0, 256, size=(1023, 32), dtype=np.uint8)
    exps[:, 31] &= 0x0f
    exps[:, 0] |= 1
    group = vm.EllipticCurve("Ed25519", "projective")
    g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
    return {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 0x1234567 * 0x89abcdef + 5),
            "gf": vm.GF(group.order)}


def gens_for(crs, N):
    return {"g": crs["g"][:N], "h": crs["h"], "k": crs["k"]}


class Draws:
    """stands in for the module's prng: hands out the queued values in order"""

    def __init__(self, values):
        self.values = list(values)

    def randrange(self, *a):
        return self.values.pop(0)


def make_batch(seed, n_x, m, n_out, K):
    rng = random.Random(seed)
    A, B, O = ref.random_circuit(rng, n_x, m, n_out, long_col=1 if m >= 100 else None)
    sc = ref.sparse(n_x, A, B, O)
    xs = [sc.pad([rng.randrange(ELL) for _ in range(n_x)]) for _ in range(K)]
    return sc, xs


def wire_of(point):
    from verifiable_mpc_amd import wire
    return wire.compress_point(point)


def same_proof(got, want):
    """two Protocol 8 proofs with the compressed pivot's part, field by field"""
    assert list(got) == list(want)
    assert wire_of(got["z_commitment"]) == wire_of(want["z_commitment"])
    for k in ("y1", "y2", "y3"):
        assert int(got[k]) % ELL == int(want[k]) % ELL, k
    assert [int(o) % ELL for o in got["outputs"]] == [int(o) % ELL for o in want["outputs"]]
    assert got["L"].coeffs.to_ints() == want["L"].coeffs.to_ints()
    assert int(got["L"].constant) % ELL == int(want["L"].constant) % ELL
    gp, wp = got["pivot_proof"], want["pivot_proof"]
    assert list(gp) == list(wp)
    for k in wp:
        if k == "z_prime":
            assert [int(v) % ELL for v in gp[k]] == [int(v) % ELL for v in wp[k]]
        elif k == "t":
            assert int(gp[k]) % ELL == int(wp[k]) % ELL
        else:
            assert wire_of(gp[k]) == wire_of(wp[k]), k


def under(vm, mode, fn):
    """fn() under the mode -> (its result, the stage names the context recorded meanwhile)"""
    ctx = vm.get_context()
    with vm.device.cs_extension(mode):
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            res = fn()
            ctx.sync()
            seen = {k for k, v in ctx.profile_read(reset=True).items() if v[1]}
        finally:
            ctx.profile(False)
    assert ("cs_extend_ntt_crt" in seen) == (mode == "ntt") and ("cs_extend_corr" in seen) == (mode == "direct"), seen
    return res


def test_single_prover(vm, cs, crs, monkeypatch):
    m = 300
    sc, (x,) = make_batch(4300, 5, m, 2, 1)
    N = len(x) + 3 + 2 * m
    assert N == 1023 and N < vm.compressed_pivot.MASKS_ON_DEVICE_MIN      # the pivot's masks come from its seeded prng
    gens, gf = gens_for(crs, N), crs["gf"]
    proofs = {}
    for mode in ("direct", "ntt"):
        monkeypatch.setattr(cs, "prng", random.Random(43))
        monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(44))
        proofs[mode] = under(vm, mode, lambda: cs.circuit_sat_prover(gens, sc, x, gf))
    same_proof(proofs["ntt"], proofs["direct"])
    assert cs.circuit_sat_verifier(proofs["ntt"], gens, sc, gf) == ALL_TRUE


def test_batch_prover(vm, cs, crs, monkeypatch):
    m, K = 300, 3
    sc, xs = make_batch(4301, 5, m, 2, K)
    N = len(xs[0]) + 3 + 2 * m
    gens, gf = gens_for(crs, N), crs["gf"]
    proofs = {}
    for mode in ("direct", "ntt"):
        monkeypatch.setattr(cs, "prng", random.Random(45))
        monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(46))
        proofs[mode] = under(vm, mode, lambda: cs.circuit_sat_prover_batch(gens, sc, xs, gf))
    assert len(proofs["ntt"]) == K
    for got, want in zip(proofs["ntt"], proofs["direct"]):
        same_proof(got, want)
    assert vm.circuit_sat_verifier_batch(proofs["ntt"], gens, sc, gf) == [ALL_TRUE] * K


def test_three_party_prover(vm, cs, crs, monkeypatch):
    from verifiable_mpc_amd import mpc_ac20, mpc_circuit_sat as mcs
    assert mpc_ac20.cp is vm.compressed_pivot           # whose masks() deals the parties' device-side randomness
    M, t, m = 3, 1, 65
    sc, (x,) = make_batch(4365, 5, m, 2, 1)
    N = len(x) + 3 + 2 * m
    gens, gf = gens_for(crs, N), crs["gf"]

    def prove():
        """M parties over one hub, every generator seeded: the same shares and the same masks each time"""
        mask_rng = np.random.default_rng(898)

        def masks(n, ctx):
            raw = mask_rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            raw[:, 31] &= 0x0f
            return vm.ScalarVector.from_array(raw, ctx)
        monkeypatch.setattr(vm.compressed_pivot, "masks", masks)
        hub = mpc_ac20.LocalHub(M)
        rts = [mpc_ac20.PartyRuntime(p, M, t, random.Random(900 + p), hub) for p in range(M)]
        dealt = mpc_ac20.deal(x, t, M, random.Random(899))
        xs = [mpc_ac20.SecureVector.from_shares(dealt[p], rts[p]) for p in range(M)]

        async def everybody():
            return await asyncio.gather(*[mcs.circuit_sat_prover(gens, sc, xs[p], gf, "compressed", rt=rt)
                                          for p, rt in enumerate(rts)])
        loop = asyncio.new_event_loop()
        try:
            return loop.run_until_complete(everybody())
        finally:
            loop.close()

    proofs = {mode: under(vm, mode, prove) for mode in ("direct", "ntt")}
    for got, want in zip(proofs["ntt"], proofs["direct"]):
        same_proof(got, want)
    assert cs.circuit_sat_verifier(proofs["ntt"][0], gens, sc, gf, "compressed") == ALL_TRUE


def typed_of(v):
    return "i:" + str(v) if isinstance(v, int) else "f:" + format(int(v) % ELL, "x")


def test_fixture_circuit_reference_transcript(vm, cs, monkeypatch):
    """the reference-made chain circuit (m = 5) with the recorded draws: z, the commitment, the y's, the outputs and L
    are the reference's, value for value, with the extension on the NTT route"""
    case = next(c for c in FIXTURE if c["name"] == "chain")
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    sc = cs.SparseCircuit.from_circuit(ref.circuit_from_fixture(case, gf))
    assert sc.m == 5
    x = [ref.untyped(v, gf) for v in case["x_typed"]]
    gens = {"g": vm.PointVector.fixed_base(group.generator, [int(e, 16) for e in case["gen_exponents"]]),
            "h": group.generator}
    monkeypatch.setattr(cs, "prng", Draws([int(case[k], 16) for k in ("r_a", "r_b", "gamma")]))
    proof, zc, L, z, gamma = under(
        vm, "ntt", lambda: cs.protocol_8_excl_pivot_prover(gens, sc, x, gf, transcript="reference"))
    assert gamma == int(case["gamma"], 16)
    assert [typed_of(v) for v in z] == case["z_typed"]
    assert [format(int(v), "x") for v in zc.coords] == case["z_commitment_proj"]
    assert [typed_of(proof[k]) for k in ("y1", "y2", "y3")] == case["y_typed"]
    assert [typed_of(v) for v in proof["outputs"]] == case["outputs_typed"]
    assert {"coeffs": [typed_of(v) for v in L.coeffs], "constant": typed_of(L.constant)} == case["L"]
