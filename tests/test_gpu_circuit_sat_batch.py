"""The batch Protocol 8 prover (verifiable_mpc_amd/circuit_sat_gpu.py: protocol_8_excl_pivot_prover_batch,
circuit_sat_prover_batch): K witnesses of one circuit through every stage together.  The contract is that the batch
returns exactly the proofs that K single calls with the same random draws return, so the oracles are the CPU
restatement tests/p8_ref.py and the single prover itself.  Every comparison is exact."""
import random

import numpy as np
import pytest

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
    """2^12 generators, k; a case takes the prefix it needs"""
    rng = np.random.default_rng(20153)
    exps = rng.integers(0, 256, size=(1 << 12, 32), dtype=np.uint8)
    exps[:, 31] &= 0x0f
    exps[:, 0] |= 1
    group = vm.EllipticCurve("Ed25519", "projective")
    g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
    ek = 0x1234567 * 0x89abcdef + 5
    return {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, ek), "gf": vm.GF(group.order)}


def gens_for(crs, N):
    return {"g": crs["g"][:N], "h": crs["h"], "k": crs["k"]}


class Draws:
    """stands in for the module's prng: hands out the queued values in order"""

    def __init__(self, values):
        self.values = list(values)

    def randrange(self, *a):
        return self.values.pop(0)


def make_batch(seed, n_x, m, n_out, K):
    """one random circuit, K distinct inputs and K distinct (r_a, r_b, gamma)"""
    rng = random.Random(seed)
    A, B, O = ref.random_circuit(rng, n_x, m, n_out, long_col=1 if m >= 100 else None)
    sc = sparse(n_x, A, B, O)
    xs = [sc.pad([rng.randrange(ELL) for _ in range(n_x)]) for _ in range(K)]
    draws = [[rng.randrange(1, ELL) for _ in range(3)] for _ in range(K)]
    return A, B, O, sc, xs, draws


def flat(draws):
    return [v for d in draws for v in d]


def wire_of(point):
    from verifiable_mpc_amd import wire
    return wire.compress_point(point)


def same_proof(got, want):
    """two Protocol 8 proofs (with or without the pivot's part) field by field"""
    assert list(got) == list(want)
    assert wire_of(got["z_commitment"]) == wire_of(want["z_commitment"])
    for k in ("y1", "y2", "y3"):
        assert int(got[k]) % ELL == int(want[k]) % ELL, k
    assert [int(o) % ELL for o in got["outputs"]] == [int(o) % ELL for o in want["outputs"]]
    assert got["L"].coeffs.to_ints() == want["L"].coeffs.to_ints()
    assert int(got["L"].constant) % ELL == int(want["L"].constant) % ELL
    if "pivot_proof" in want:
        gp, wp = got["pivot_proof"], want["pivot_proof"]
        assert list(gp) == list(wp)
        for k in wp:
            if k == "z_prime":
                assert [int(v) % ELL for v in gp[k]] == [int(v) % ELL for v in wp[k]]
            elif k == "t":
                assert int(gp[k]) % ELL == int(wp[k]) % ELL
            else:
                assert wire_of(gp[k]) == wire_of(wp[k]), k


# ---- 1. z against the CPU restatement -------------------------------------------------------------------------------------
# K <= 3 at m = 1000: what the restatement's Python affords there
Z_CASES = [(m, K) for m in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 258, 1000) for K in (1, 2, 3, 5) if m < 1000 or K <= 3]


@pytest.mark.parametrize("m,K", Z_CASES, ids=[f"m{m}_K{k}" for m, k in Z_CASES])
def test_every_row_of_z_matches_the_cpu_restatement(vm, cs, m, K):
    A, B, O, sc, xs, draws = make_batch(3000 + 7 * m + K, 5, m, 2, K)
    n_in = len(xs[0])
    N = n_in + 3 + 2 * m
    rows = np.stack([vm.sparse.residue_array(x, ELL) for x in xs])
    Z = cs._witnesses_on_device(sc, rows, n_in, draws)
    got = Z.to_ints()
    assert len(got) == K * N
    for p, (x, d) in enumerate(zip(xs, draws)):
        want = ref.prove(5, A, B, O, x, d[0], d[1], lambda z_: bytes(32))["z"]
        assert got[p * N:(p + 1) * N] == want, p


# ---- 2. a K at which the batch picks another segment length than the single call ------------------------------------------
def test_k_aware_segmentation_gives_the_single_provers_z(vm, cs, crs, monkeypatch):
    """m = 1000: 4 tiles x 4 segments of CS_MIN_SEG.  The batched launch doubles the segment while tiles x segments x K
    is ABOVE CS_TARGET_WGS = 8192, so K = 512 (exactly 8192 workgroups) still runs the single call's 4 segments and
    K = 513 is the first batch that runs 2 segments of 512: the switch is at 513, not at 512, and K is set to it.
    Witnesses 0, K/2 and K-1 against the single prover under the same draws."""
    K, m = 513, 1000
    A, B, O, sc, x0, _ = make_batch(3513, 5, m, 2, 1)
    n_in = len(x0[0])
    N = n_in + 3 + 2 * m
    rng = np.random.default_rng(513)
    rows = rng.integers(0, 256, size=(K, n_in, 32), dtype=np.uint8)
    rows[:, :, 31] &= 0x0f
    rr = random.Random(514)
    draws = [[rr.randrange(1, ELL) for _ in range(3)] for _ in range(K)]
    assert cs._chunk_size(sc, n_in, K) == K                 # one chunk: all 513 in one launch sequence
    Z = cs._witnesses_on_device(sc, rows, n_in, draws)
    gens, gf = gens_for(crs, N), crs["gf"]
    for p in (0, K // 2, K - 1):
        x = [int.from_bytes(rows[p, i].tobytes(), "little") for i in range(n_in)]
        monkeypatch.setattr(cs, "prng", Draws(draws[p]))
        _, _, _, z, _ = cs.protocol_8_excl_pivot_prover(gens, sc, x, gf)
        assert Z[p * N:(p + 1) * N].to_ints() == z.to_ints(), p


# ---- 3. proof for proof ---------------------------------------------------------------------------------------------------
SMALL = [c for c in GPU_CASES if c[1] + 3 + 2 * c[2] + 1 <= 1 << 11]


@pytest.mark.parametrize("seed,n_x,m,n_out", SMALL)
def test_batch_equals_single_calls_proof_for_proof(vm, cs, crs, monkeypatch, seed, n_x, m, n_out):
    """N + 1 <= 2^11 < MASKS_ON_DEVICE_MIN: the pivot's masks come from its seeded prng"""
    K = 3
    A, B, O, sc, xs, _ = make_batch(seed, n_x, m, n_out, K)
    N = len(xs[0]) + 3 + 2 * m
    assert N + 1 <= 1 << 11 and N < vm.compressed_pivot.MASKS_ON_DEVICE_MIN
    gens, gf = gens_for(crs, N), crs["gf"]
    monkeypatch.setattr(cs, "prng", random.Random(seed))
    monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(seed + 1))
    singles = [cs.circuit_sat_prover(gens, sc, x, gf) for x in xs]
    # the single calls interleave their draws with the pivots'; the batch draws everything first, from each
    # generator in the same order
    monkeypatch.setattr(cs, "prng", random.Random(seed))
    monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(seed + 1))
    batch = cs.circuit_sat_prover_batch(gens, sc, xs, gf)
    assert len(batch) == K
    for got, want in zip(batch, singles):
        same_proof(got, want)
    assert vm.circuit_sat_verifier_batch(batch, gens, sc, gf) == [ALL_TRUE] * K
    if n_out:
        outs = list(batch[1]["outputs"])
        outs[0] = outs[0] + 1
        altered = [batch[0], dict(batch[1], outputs=outs), batch[2]]
        verdicts = vm.circuit_sat_verifier_batch(altered, gens, sc, gf)
        assert verdicts[0] == ALL_TRUE and verdicts[2] == ALL_TRUE
        assert verdicts[1]["L_wellformed_from_Cfgh_forms"] is False


# ---- 4. depth: one launch per level, not per level and witness -----------------------------------------------------------
def test_chain_circuit_costs_one_launch_per_level_for_all_witnesses(vm, cs, crs, monkeypatch):
    """x^(m+1) as a product chain (depth = m) on K = 4 inputs"""
    m, K = 30, 4
    A = [({0 if i == 0 else 1 + i - 1: 1}, 0) for i in range(m)]
    B = [({0: 1}, 0) for _ in range(m)]
    O = [({1 + m - 1: 1}, 0)]
    sc = sparse(1, A, B, O)
    assert len(sc.level_ptr) == m + 1
    bases = [3, 5, ELL - 2, 7]
    xs = [sc.pad([v]) for v in bases]
    ctx = sc.device()["ctx"]
    calls = []
    real = ctx.cs_triples_batch

    def counting(*a, **kw):
        calls.append(a[12] if len(a) > 12 else kw.get("check", 0))          # check: 0 when left out
        return real(*a, **kw)
    monkeypatch.setattr(ctx, "cs_triples_batch", counting)
    monkeypatch.setattr(cs, "prng", Draws(range(11, 11 + 3 * K)))
    res = cs.protocol_8_excl_pivot_prover_batch(gens_for(crs, len(xs[0]) + 3 + 2 * m), sc, xs, crs["gf"])
    # the levels, and the one values-only launch for the outputs
    assert calls.count(0) == len(sc.level_ptr) - 1 and calls.count(2) == 1 and len(calls) == len(sc.level_ptr)
    for p, ((proof, zc, L, z, gamma), v) in enumerate(zip(res, bases)):
        assert [int(o) % ELL for o in proof["outputs"]] == [pow(v, m + 1, ELL)]
        assert gamma == 13 + 3 * p
        assert z.to_ints() == ref.prove(1, A, B, O, xs[p], 11 + 3 * p, 12 + 3 * p, lambda z_: wire_of(zc))["z"]
        assert int(L(z)) % ELL == 0


# ---- 5. gamma_witnesses ---------------------------------------------------------------------------------------------------
def test_gamma_witnesses_are_checked_in_one_launch(vm, cs, crs, monkeypatch):
    K, m = 3, 65
    A, B, O, sc, xs, draws = make_batch(3565, 5, m, 2, K)
    N = len(xs[0]) + 3 + 2 * m
    gens, gf = gens_for(crs, N), crs["gf"]
    gammas = [ref.triples(5, A, B, x)[2] for x in xs]
    monkeypatch.setattr(cs, "prng", Draws(flat(draws)))
    computed = cs.protocol_8_excl_pivot_prover_batch(gens, sc, xs, gf)
    ctx = sc.device()["ctx"]
    calls = []
    real = ctx.cs_triples_batch
    monkeypatch.setattr(ctx, "cs_triples_batch", lambda *a, **kw: calls.append(a) or real(*a, **kw))
    monkeypatch.setattr(cs, "prng", Draws(flat(draws)))
    given = cs.protocol_8_excl_pivot_prover_batch(gens, sc, xs, gf, gamma_witnesses=gammas)
    assert len(calls) == 2                                   # the check and the outputs
    for (p1, zc1, _, z1, g1), (p2, zc2, _, z2, g2) in zip(computed, given):
        assert z1.to_ints() == z2.to_ints() and zc1 == zc2 and g1 == g2
        same_proof(p2, p1)
    monkeypatch.setattr(cs, "prng", random.Random(5))      # the draws come before the first launch, the check included
    gammas[1][7] = (gammas[1][7] + 1) % ELL
    gammas[1][40] = (gammas[1][40] + 1) % ELL
    gammas[2][5] = (gammas[2][5] + 1) % ELL
    with pytest.raises(ValueError, match=r"gamma_witnesses\[1\]: multiplication gate 7 "):
        cs.protocol_8_excl_pivot_prover_batch(gens, sc, xs, gf, gamma_witnesses=gammas)
    with pytest.raises(ValueError, match="gamma_witnesses: 3 lists of 65 gate outputs"):
        cs.protocol_8_excl_pivot_prover_batch(gens, sc, xs, gf, gamma_witnesses=gammas[:2])


# ---- 6. inputs that are bytes or on the device already ---------------------------------------------------------------------
def test_array_and_device_inputs_give_the_list_forms_proofs(vm, cs, crs, monkeypatch):
    K, m = 3, 64
    A, B, O, sc, xs, draws = make_batch(3664, 5, m, 2, K)
    xs[0][0] = -3                                           # a list may hold any int; the other forms hold its residue
    n_in = len(xs[0])
    gens, gf = gens_for(crs, n_in + 3 + 2 * m), crs["gf"]

    def run(inputs, **kw):
        monkeypatch.setattr(cs, "prng", random.Random(64))
        monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(65))
        return cs.circuit_sat_prover_batch(gens, sc, inputs, gf, **kw)

    want = run(xs)
    arr = np.stack([vm.sparse.residue_array(x, ELL) for x in xs])
    assert arr.shape == (K, n_in, 32)
    on_device = vm.ScalarVector.from_array(arr.reshape(K * n_in, 32))
    for got in (run(arr), run(on_device, n_in=n_in), run(tuple(tuple(x) for x in xs))):
        assert len(got) == K
        for g, w in zip(got, want):
            same_proof(g, w)
    # a value above l in the array is reduced, as an int in a list is
    big = arr.copy()
    big[0, 1] = np.frombuffer((int.from_bytes(arr[0, 1].tobytes(), "little") + ELL).to_bytes(32, "little"), np.uint8)
    for g, w in zip(run(big), want):
        same_proof(g, w)
    assert cs.circuit_sat_prover_batch(gens, sc, [], gf) == []
    assert cs.circuit_sat_prover_batch(gens, sc, np.zeros((0, n_in, 32), np.uint8), gf) == []
    assert cs.protocol_8_excl_pivot_prover_batch(gens, sc, on_device[:0], gf, n_in=n_in) == []
    with pytest.raises(ValueError, match="same number of inputs"):
        cs.circuit_sat_prover_batch(gens, sc, [xs[0], xs[1][:-1]], gf)
    with pytest.raises(ValueError, match="the circuit has 5 inputs, 4 given"):
        cs.circuit_sat_prover_batch(gens, sc, [x[:4] for x in xs], gf)
    with pytest.raises(ValueError, match="n_in="):
        cs.circuit_sat_prover_batch(gens, sc, on_device, gf)
    with pytest.raises(ValueError, match="not a multiple"):
        cs.circuit_sat_prover_batch(gens, sc, on_device, gf, n_in=n_in + 1)


# ---- 7. a first challenge on an interpolation node ------------------------------------------------------------------------
def test_challenge_on_a_node_names_the_witness_before_any_forms_launch(vm, cs, crs, monkeypatch):
    K, m = 3, 64
    A, B, O, sc, xs, draws = make_batch(3764, 5, m, 2, K)
    gens, gf = gens_for(crs, len(xs[0]) + 3 + 2 * m), crs["gf"]
    launched = []
    real_forms = cs._Forms
    monkeypatch.setattr(cs, "_Forms", lambda *a: launched.append(a) or real_forms(*a))
    real_challenge = cs.first_challenge
    for node in (0, m, 2 * m):
        seen = []

        def challenge(digest, order, node=node, seen=seen):
            seen.append(digest)
            return node if len(seen) == 2 else real_challenge(digest, order)        # witness 1 of 3
        monkeypatch.setattr(cs, "first_challenge", challenge)
        with pytest.raises(cs.ChallengeOnNode, match=f"witness 1: the first challenge {node} is an interpolation node"):
            cs.circuit_sat_prover_batch(gens, sc, xs, gf)
        assert len(seen) == K and launched == []
    monkeypatch.setattr(cs, "first_challenge", real_challenge)
    assert len(cs.protocol_8_excl_pivot_prover_batch(gens, sc, xs, gf)) == K and len(launched) == K


# ---- 8. chunks ------------------------------------------------------------------------------------------------------------
def test_a_chunk_boundary_changes_no_value(vm, cs, crs, monkeypatch):
    K, m = 5, 258
    A, B, O, sc, xs, draws = make_batch(3858, 5, m, 2, K)
    n_in = len(xs[0])
    gens, gf = gens_for(crs, n_in + 3 + 2 * m), crs["gf"]

    def run():
        monkeypatch.setattr(cs, "prng", random.Random(58))
        monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(59))
        return cs.circuit_sat_prover_batch(gens, sc, xs, gf)

    assert cs._chunk_size(sc, n_in, K) == K
    whole = run()
    two, three = cs._batch_bytes(sc, n_in, 2), cs._batch_bytes(sc, n_in, 3)
    assert two < three
    monkeypatch.setattr(cs, "BATCH_BUDGET_BYTES", (two + three) // 2)
    assert cs._chunk_size(sc, n_in, K) == 2
    starts = []
    real = cs._prove_chunk
    monkeypatch.setattr(cs, "_prove_chunk", lambda *a: starts.append((a[-1], len(a[4]))) or real(*a))
    split = run()
    assert starts == [(0, 2), (2, 2), (4, 1)]
    assert len(split) == K
    for got, want in zip(split, whole):
        same_proof(got, want)
    # a budget below one witness still proves one at a time
    monkeypatch.setattr(cs, "BATCH_BUDGET_BYTES", 1)
    assert cs._chunk_size(sc, n_in, K) == 1


# ---- 9. the paths that are host list code -----------------------------------------------------------------------------------
def test_reference_transcript_and_plain_pivot_fall_back_to_the_single_prover(vm, cs):
    case = next(c for c in FIXTURE if c["name"] == "padded")
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    sc = cs.SparseCircuit.from_circuit(ref.circuit_from_fixture(case, gf))
    x = [ref.untyped(v, gf) for v in case["x_typed"]]
    xs = [x, [v + 1 for v in x]]
    rng = random.Random(78)
    gens = {"g": vm.PointVector.fixed_base(group.generator, [int(e, 16) for e in case["gen_exponents"]]),
            "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ELL))}
    for choice, transcript in (("compressed", "reference"), ("pivot", "reference"), ("pivot", None)):
        proofs = cs.circuit_sat_prover_batch(gens, sc, xs, gf, choice, transcript=transcript)
        assert len(proofs) == 2
        for proof in proofs:
            assert cs.circuit_sat_verifier(proof, gens, sc, gf, choice, transcript=transcript) == ALL_TRUE
    with pytest.raises(NotImplementedError, match="BN-256"):
        cs.circuit_sat_prover_batch(gens, sc, xs, gf, "koe")
    assert vm.circuit_sat_prover_batch is cs.circuit_sat_prover_batch
    assert vm.protocol_8_excl_pivot_prover_batch is cs.protocol_8_excl_pivot_prover_batch
