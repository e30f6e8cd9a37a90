"""Protocol 8 on the GPU from a sparse circuit (verifiable_mpc_amd/circuit_sat_gpu.py, csrc/circuit_sat.hip) against the
CPU restatement tests/p8_ref.py: z, both challenges, the Lagrange vectors, the three forms and L bit for bit on random
circuits (compact transcript), prove -> verify for both pivots with cross-verification under oracle/ac20_ref.py,
soundness plumbing, a first challenge on an interpolation node, and the unchanged dispatch of other circuit objects.
Every comparison is exact.

The reference-made fixture circuits (tests/golden/p8_circuits.json) tie the path to the reference itself: with the
reference transcript and the recorded draws, z, both hashes, y1..y3, outputs, L and [z] are the reference's, value for
value and representative for representative."""
import random

import numpy as np
import pytest

from oracle import ac20_ref as ac
from oracle import ed25519_ref as ed
from tests import p8_ref as ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
GPU_CASES, sparse = ref.GPU_CASES, ref.sparse
FIXTURE = load_golden("p8_circuits.json")["cases"]
ELL = ref.ELL
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
    """2^16 - 1 generators, k; a case takes the prefix it needs"""
    rng = np.random.default_rng(20152)
    exps = rng.integers(0, 256, size=((1 << 16) - 1, 32), dtype=np.uint8)
    exps[:, 31] &= 0x0f
    exps[:, 0] |= 1
    group = vm.EllipticCurve("Ed25519", "projective")
    g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
    ek = 0x1234567 * 0x89abcdef + 5
    return {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, ek), "gf": vm.GF(group.order),
            "exps": exps, "ek": ek}


def gens_for(crs, N):
    return {"g": crs["g"][:N], "h": crs["h"], "k": crs["k"]}


class Draws:
    """stands in for the module's prng: hands out the queued values in order"""

    def __init__(self, values):
        self.values = list(values)

    def randrange(self, *a):
        return self.values.pop(0)


def make_case(seed, n_x, m, n_out):
    rng = random.Random(seed)
    A, B, O = ref.random_circuit(rng, n_x, m, n_out, long_col=1 if m >= 100 else None)
    sc = sparse(n_x, A, B, O)
    x = sc.pad([rng.randrange(ELL) for _ in range(n_x)])
    draws = [rng.randrange(1, ELL) for _ in range(3)]       # r_a, r_b, gamma
    return A, B, O, sc, x, draws


def wire_of(vm, point):
    from verifiable_mpc_amd import wire
    return wire.compress_point(point)


# ---- 1. the reference's own circuits, reference transcript ----------------------------------------------------------------
def typed_of(v):
    return "i:" + str(v) if isinstance(v, int) else "f:" + format(int(v) % ELL, "x")


def form_of(f):
    return {"coeffs": [typed_of(v) for v in f.coeffs], "constant": typed_of(f.constant)}


@pytest.mark.parametrize("case", FIXTURE, ids=[c["name"] for c in FIXTURE])
def test_fixture_circuit_reference_transcript(vm, cs, monkeypatch, case):
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    circuit = ref.circuit_from_fixture(case, gf)
    sc = cs.SparseCircuit.from_circuit(circuit)
    raw = sc.raw_forms()
    for key in "ABO":       # the recorded construct_affine_form output, value and Python type
        want = ref.fixture_rows(case[key], gf)
        got = [({c: v for c, v in e.items() if not (isinstance(v, int) and v == 0)}, k) for e, k in raw[key]]
        assert [({c: typed_of(v) for c, v in e.items()}, typed_of(k)) for e, k in got] == \
            [({c: typed_of(v) for c, v in e.items()}, typed_of(k)) for e, k in want]
    x = [ref.untyped(v, gf) for v in case["x_typed"]]
    gens = {"g": vm.PointVector.fixed_base(group.generator, [int(e, 16) for e in case["gen_exponents"]]),
            "h": group.generator}
    monkeypatch.setattr(cs, "prng", Draws([int(case[k], 16) for k in ("r_a", "r_b", "gamma")]))
    hashes = []
    real_hash = vm.pivot.fiat_shamir_hash
    monkeypatch.setattr(vm.pivot, "fiat_shamir_hash", lambda lst, order: hashes.append(real_hash(lst, order)) or hashes[-1])
    proof, zc, L, z, gamma = cs.protocol_8_excl_pivot_prover(gens, sc, x, gf, transcript="reference")
    assert gamma == int(case["gamma"], 16)
    assert [typed_of(v) for v in z] == case["z_typed"]
    assert [format(int(v), "x") for v in zc.coords] == case["z_commitment_proj"]
    assert [format(h, "x") for h in hashes] == [h["c"] for h in case["hashes"]]
    assert [typed_of(proof[k]) for k in ("y1", "y2", "y3")] == case["y_typed"]
    assert [typed_of(v) for v in proof["outputs"]] == case["outputs_typed"]
    assert form_of(L) == case["L"]
    # the verifier recomputes both hashes and the same L; the compact path proves the same statement
    verification, L2 = cs.protocol_8_excl_pivot_verifier(proof, sc, gf, transcript="reference")
    assert verification == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True} and form_of(L2) == case["L"]
    assert hashes[2:] == hashes[:2]
    monkeypatch.setattr(cs, "prng", Draws([int(case[k], 16) for k in ("r_a", "r_b", "gamma")]))
    _, _, Lc, zd, _ = cs.protocol_8_excl_pivot_prover(gens, sc, x, gf)
    assert zd.to_ints() == [ref.untyped(v) % ELL for v in case["z_typed"]]
    assert int(Lc(zd)) % ELL == 0


def test_reference_transcript_end_to_end(vm, cs):
    """the padded fixture circuit (N + 1 = 16) through circuit_sat_prover / _verifier in list mode, both pivots"""
    case = next(c for c in FIXTURE if c["name"] == "padded")
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    sc = cs.SparseCircuit.from_circuit(ref.circuit_from_fixture(case, gf))
    x = [ref.untyped(v, gf) for v in case["x_typed"]]
    rng = random.Random(77)
    gens = {"g": vm.PointVector.fixed_base(group.generator, [int(e, 16) for e in case["gen_exponents"]]),
            "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ELL))}
    for choice in ("compressed", "pivot"):
        proof = cs.circuit_sat_prover(gens, sc, x, gf, choice, transcript="reference")
        assert cs.circuit_sat_verifier(proof, gens, sc, gf, choice, transcript="reference") == ALL_TRUE
        proof["outputs"] = [proof["outputs"][0] + 1]
        assert cs.circuit_sat_verifier(proof, gens, sc, gf, choice, transcript="reference")["L_wellformed_from_Cfgh_forms"] \
            is False


# ---- 2. random sparse circuits against the CPU restatement --------------------------------------------------------------
@pytest.mark.parametrize("seed,n_x,m,n_out", GPU_CASES)
def test_random_circuit_matches_cpu_restatement(vm, cs, crs, monkeypatch, seed, n_x, m, n_out):
    A, B, O, sc, x, draws = make_case(seed, n_x, m, n_out)
    n_in, N = len(x), len(x) + 3 + 2 * m
    assert bin(N + 1).count("1") == 1
    monkeypatch.setattr(cs, "prng", Draws(draws))
    gf = crs["gf"]
    proof, zc, L, z, gamma = cs.protocol_8_excl_pivot_prover(gens_for(crs, N), sc, x, gf)
    assert gamma == draws[2]
    want = ref.prove(n_x, A, B, O, x, draws[0], draws[1], lambda z_: wire_of(vm, zc))
    got_z = z.to_ints()
    assert len(got_z) == N
    assert got_z[:n_in] == want["z"][:n_in]
    assert got_z[n_in + 3:n_in + 3 + m] == want["gamma"]
    assert got_z == want["z"]
    # the commitment is the one to this z (spot check against the oracle's ladders on the small cases)
    if N <= 256:
        og = [ed.pt_repeat(ed.BASE, int.from_bytes(crs["exps"][i].tobytes(), "little")) for i in range(N)]
        assert tuple(zc.normalize().coords[:2]) == ed.pt_affine(ac.vector_commitment(want["z"], gamma, og, ed.BASE))
    # challenges, Lagrange vectors, forms, L
    digest = cs._first_digest(zc, sc, n_in)
    c = cs.first_challenge(digest, ELL)
    assert c == want["c"]
    forms = cs._Forms(sc, n_in, c, ELL)
    assert forms.lam.to_ints() == want["lambda_m"]
    assert forms.H.to_ints()[n_in + 2:] == want["lambda_2m"]
    for V, k, (wc, wk) in zip((forms.F, forms.G, forms.H), forms.k, (want["F"], want["G"], want["H"])):
        assert V.to_ints() == wc
        assert k == wk
    assert [int(proof[k]) % ELL for k in ("y1", "y2", "y3")] == want["y"]
    assert [int(o) % ELL for o in proof["outputs"]] == want["outputs"]
    assert cs._second_challenge(digest, want["y"], want["outputs"], ELL) == want["rho"]
    assert L.coeffs.to_ints() == want["L"]
    assert int(L.constant) % ELL == want["L_const"]
    assert int(L(z)) % ELL == 0
    # the verifier's side recomputes the same L
    verification, L2 = cs.protocol_8_excl_pivot_verifier(proof, sc, gf)
    assert verification == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True}
    assert L2.coeffs.to_ints() == want["L"]
    # a caller that already has the gate outputs: one launch, the same z
    monkeypatch.setattr(cs, "prng", Draws(draws))
    _, zc2, _, z2, _ = cs.protocol_8_excl_pivot_prover(gens_for(crs, N), sc, x, gf, gamma_witness=want["gamma"])
    assert z2.to_ints() == want["z"] and zc2 == zc


def test_chain_circuit_costs_one_level_per_gate(vm, cs, crs, monkeypatch):
    """x^(m+1) as a product chain: depth = m"""
    m = 30
    A = [({0 if i == 0 else 1 + i - 1: 1}, 0) for i in range(m)]
    B = [({0: 1}, 0) for _ in range(m)]
    O = [({1 + m - 1: 1}, 0)]
    sc = sparse(1, A, B, O)
    assert sc.depth.tolist() == list(range(m)) and len(sc.level_ptr) == m + 1
    x = sc.pad([3])
    monkeypatch.setattr(cs, "prng", Draws([11, 13, 17]))
    proof, zc, L, z, _ = cs.protocol_8_excl_pivot_prover(gens_for(crs, len(x) + 3 + 2 * m), sc, x, crs["gf"])
    assert [int(o) % ELL for o in proof["outputs"]] == [pow(3, m + 1, ELL)]
    assert z.to_ints() == ref.prove(1, A, B, O, x, 11, 13, lambda z_: wire_of(vm, zc))["z"]


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_x,m,n_out", [GPU_CASES[3], GPU_CASES[6], GPU_CASES[8], GPU_CASES[9]])
def test_prove_and_verify_compressed_pivot(vm, cs, crs, seed, n_x, m, n_out):
    A, B, O, sc, x, _ = make_case(seed, n_x, m, n_out)
    N = len(x) + 3 + 2 * m
    gens, gf = gens_for(crs, N), crs["gf"]
    proof = vm.circuit_sat_prover(gens, sc, x, gf, vm.PivotChoice.compressed)
    assert vm.circuit_sat_verifier(proof, gens, sc, gf, vm.PivotChoice.compressed) == ALL_TRUE
    if N <= 256:
        # the pivot proof under the oracle's Protocol 5 verifier, given the CPU-side L
        z = None
        digest = cs._first_digest(proof["z_commitment"], sc, len(x))
        c = cs.first_challenge(digest, ELL)
        y = [int(proof[k]) % ELL for k in ("y1", "y2", "y3")]
        outs = [int(o) % ELL for o in proof["outputs"]]
        rho = ref.second_challenge(digest, *y, outs)
        co, const, _ = ref.combine(n_x, len(x), A, B, O, c, rho, y, outs)
        ogens = {"g": [ed.pt_repeat(ed.BASE, int.from_bytes(crs["exps"][i].tobytes(), "little")) for i in range(N)],
                 "h": ed.BASE, "k": ed.pt_repeat(ed.BASE, crs["ek"])}
        pp = proof["pivot_proof"]
        oproof = {k: tuple(int(v) for v in p.normalize().coords) for k, p in pp.items() if k not in ("t", "z_prime")}
        oproof["t"] = int(pp["t"]) % ELL
        oproof["z_prime"] = [int(v) % ELL for v in pp["z_prime"]]
        oP = tuple(int(v) for v in proof["z_commitment"].normalize().coords)
        assert ac.protocol_5_verifier(ogens, oP, co, const, 0, oproof, "compact") is True
        assert ac.protocol_5_verifier(ogens, oP, co, (const + 1) % ELL, 0, oproof, "compact") is False
        del z


def test_prove_and_verify_plain_pivot(vm, cs):
    rng = random.Random(5)
    A, B, O, sc, x, _ = make_case(103, 5, 3, 2)
    N = len(x) + 3 + 6
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    gens = {"g": vm.PointVector.fixed_base(group.generator, [rng.randrange(1, ELL) for _ in range(N)]), "h": group.generator}
    proof = vm.circuit_sat_prover(gens, sc, x, gf, vm.PivotChoice.pivot)
    assert vm.circuit_sat_verifier(proof, gens, sc, gf, vm.PivotChoice.pivot) == ALL_TRUE
    z, phi, c = proof["pivot_proof"]
    proof["pivot_proof"] = (z, phi + 1, c)
    assert vm.circuit_sat_verifier(proof, gens, sc, gf, vm.PivotChoice.pivot)["pivot_verification"] is False


def test_koe_is_refused_by_name(vm, cs, crs):
    A, B, O, sc, x, _ = make_case(103, 5, 3, 2)
    gens = gens_for(crs, len(x) + 9)
    with pytest.raises(NotImplementedError, match="BN-256"):
        vm.circuit_sat_prover(gens, sc, x, crs["gf"], vm.PivotChoice.koe)
    with pytest.raises(ValueError, match="unknown transcript"):
        cs.circuit_sat_prover(gens, sc, x, crs["gf"], transcript="other")


def test_builder_shaped_circuit_is_converted(vm, cs, crs):
    case = next(c for c in FIXTURE if c["name"] == "mixed")
    circuit = ref.circuit_from_fixture(case)
    sc = cs.SparseCircuit.from_circuit(circuit)
    x = sc.pad([ref.untyped(v) for v in case["x_typed"]])
    gens = gens_for(crs, len(x) + 3 + 2 * sc.m)
    proof, *_ = cs.protocol_8_excl_pivot_prover(gens, circuit, x, crs["gf"])       # converted on the way in
    assert [int(o) % ELL for o in proof["outputs"]] == [ref.untyped(v) % ELL for v in case["outputs_typed"]]
    full = cs.circuit_sat_prover(gens, sc, x, crs["gf"])
    assert cs.circuit_sat_verifier(full, gens, sc, crs["gf"]) == ALL_TRUE


# ---- 4. soundness plumbing -------------------------------------------------------------------------------------------------
def test_altered_proofs_fail_the_named_check(vm, cs, crs):
    A, B, O, sc, x, _ = make_case(163, 5, 63, 2)
    N = len(x) + 3 + 2 * 63
    gens, gf = gens_for(crs, N), crs["gf"]
    proof = vm.circuit_sat_prover(gens, sc, x, gf)
    assert vm.circuit_sat_verifier(proof, gens, sc, gf) == ALL_TRUE

    def verdict(**changes):
        return vm.circuit_sat_verifier(dict(proof, **changes), gens, sc, gf)

    assert verdict(y1=proof["y1"] + 1) == {"y1*y2=y3": False}
    assert verdict(y3=proof["y3"] + 1) == {"y1*y2=y3": False}
    assert cs.protocol_8_excl_pivot_verifier(dict(proof, y1=proof["y1"] + 1), sc, gf) == ({"y1*y2=y3": False}, None)
    outs = list(proof["outputs"])
    outs[1] = outs[1] + 1
    assert verdict(outputs=outs)["L_wellformed_from_Cfgh_forms"] is False
    co = proof["L"].coeffs.to_ints()
    co[N // 2] = (co[N // 2] + 1) % ELL
    bad_L = vm.pivot.AffineForm(vm.ScalarVector.from_ints(co), proof["L"].constant)
    assert verdict(L=bad_L)["L_wellformed_from_Cfgh_forms"] is False
    other = vm.Ed25519Point.operation(proof["z_commitment"], crs["h"])
    # another commitment is another first challenge, so another L
    v = verdict(z_commitment=other)
    assert v["y1*y2=y3"] is True and v["L_wellformed_from_Cfgh_forms"] is False
    # the verifier's circuit differs in one CSR value
    A2 = [(dict(e), k) for e, k in A]
    row = next(i for i, (e, _) in enumerate(A2) if e)
    col = next(iter(A2[row][0]))
    A2[row][0][col] += 1
    v = vm.circuit_sat_verifier(proof, gens, sparse(5, A2, B, O), gf)
    assert v["L_wellformed_from_Cfgh_forms"] is False
    # what remains when L is the verifier's own but the pivot proof is for another statement
    pp = dict(proof["pivot_proof"])
    pp["t"] = pp["t"] + 1
    assert verdict(pivot_proof=pp) == dict(ALL_TRUE, pivot_verification=False)


def test_wrong_gamma_witness_names_the_smallest_bad_gate(vm, cs, crs):
    A, B, O, sc, x, draws = make_case(1100, 5, 1000, 2)
    gamma = ref.triples(5, A, B, x)[2]
    gamma[700] = (gamma[700] + 1) % ELL
    gamma[345] = (gamma[345] + 1) % ELL
    with pytest.raises(ValueError, match="multiplication gate 345 "):
        cs.protocol_8_excl_pivot_prover(gens_for(crs, len(x) + 2003), sc, x, crs["gf"], gamma_witness=gamma)


# ---- 5. the first challenge on an interpolation node -------------------------------------------------------------------
def test_challenge_on_a_node(vm, cs, crs, monkeypatch):
    A, B, O, sc, x, draws = make_case(164, 5, 64, 2)
    m, n_in = 64, len(x)
    gens, gf = gens_for(crs, n_in + 3 + 2 * m), crs["gf"]
    honest = vm.circuit_sat_prover(gens, sc, x, gf)
    launched = []
    real_forms = cs._Forms
    monkeypatch.setattr(cs, "_Forms", lambda *a: launched.append(a) or real_forms(*a))
    for node in (0, m, 2 * m):
        monkeypatch.setattr(cs, "first_challenge", lambda digest, order, node=node: node)
        with pytest.raises(cs.ChallengeOnNode, match="interpolation node"):
            cs.circuit_sat_prover(gens, sc, x, gf)
        assert vm.circuit_sat_verifier(honest, gens, sc, gf) == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": False}
        assert launched == []            # no Lagrange kernel saw the zero
    # the first non-node
    c = 2 * m + 1
    monkeypatch.setattr(cs, "first_challenge", lambda digest, order: c)
    monkeypatch.setattr(cs, "prng", Draws(draws))
    proof, zc, L, z, gamma = cs.protocol_8_excl_pivot_prover(gens, sc, x, gf)
    want = ref.prove(5, A, B, O, x, draws[0], draws[1], lambda z_: wire_of(vm, zc), c_override=c)
    assert L.coeffs.to_ints() == want["L"] and [int(proof[k]) % ELL for k in ("y1", "y2", "y3")] == want["y"]
    assert launched
    forms = real_forms(sc, n_in, c, ELL)
    assert forms.F.to_ints() == want["F"][0] and forms.G.to_ints() == want["G"][0] and forms.H.to_ints() == want["H"][0]
    monkeypatch.setattr(cs, "prng", random.SystemRandom())
    full = cs.circuit_sat_prover(gens, sc, x, gf)
    assert vm.circuit_sat_verifier(full, gens, sc, gf) == ALL_TRUE


# ---- 6. unchanged dispatch ------------------------------------------------------------------------------------------------
def test_other_circuit_objects_still_reach_the_reference(vm):
    class NotSparse:
        input_ct, mul_ct = 1, 0
    try:
        import verifiable_mpc.ac20.circuit_sat_cb  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="circuit front end, out of scope of this package"):
            vm.circuit_sat_prover({}, NotSparse(), [1], None)
        with pytest.raises(ImportError, match="delegate to the reference"):
            vm.circuit_sat_verifier({}, {}, NotSparse(), None)
    else:
        assert vm.circuit_sat._reference_circuit_sat() is not None
