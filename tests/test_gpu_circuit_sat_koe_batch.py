"""The batch Protocol 8 prover over BN-256 (circuit_sat_gpu.circuit_sat_prover_batch with a knowledge-of-exponent pp and
PivotChoice.koe; knowledge_of_exponent.restriction_argument_prover_batch / opening_linear_form_prover_batch): K witnesses
of one circuit, every stage once for all of them.  The contract is that the batch returns exactly what K
circuit_sat_prover calls return under the same draws, so the yardsticks are the single prover - existing code - and,
independently of every kernel, the CPU restatement tests/p8_field_ref.py with the trapdoor's exponents times the
generators (oracle/bn256_ref.py).  Every comparison is byte for byte.

Circuits are (seed, n_x, m, n_out); the draws (r_a, r_b, gamma per witness, witness after witness) are replayed through
circuit_sat_gpu.prng."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import p8_field_ref as fref
from tests import p8_ref as ref_l

pytestmark = pytest.mark.gpu

N_ORDER = fref.BN_N
F = fref.P8(N_ORDER)
ALL_TRUE = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True,
            "pivot_verification": {"restriction_arg_check": True, "PRQ_check": True}}
SMALL = (103, 5, 3, 2)                      # N = 14
M65 = (165, 5, 65, 2)                       # the first m past a 64-lane boundary
EDGES = [(7, 4, 0, 1), (8, 6, 9, 0), M65]   # m = 0, no outputs, m = 65
K_MAX = 17                                  # crosses msm_rows' group of 16


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
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    return cs, vm.knowledge_of_exponent


@pytest.fixture(autouse=True)
def restore_prngs(mods):
    cs, koe = mods
    saved = cs.prng, koe.prng
    yield
    cs.prng, koe.prng = saved


def setup(vm, koe, n_z, seed):
    """(pp for vectors of n_z scalars, its trapdoor)"""
    rng = random.Random(5000 + seed)
    g_exp, alpha, s = rng.randrange(1, N_ORDER), rng.randrange(N_ORDER), rng.randrange(N_ORDER)
    koe.prng = Replay([g_exp, alpha, s])
    pp = koe.trusted_setup(vm.pynocchio.BN256Point(bn.G1), vm.pynocchio.BN256TwistPoint(bn.G2), n_z, N_ORDER)
    assert koe.prng.draws == []
    return pp, fref.KoeTrapdoor(g_exp, alpha, s)


def flat(draws):
    return [v for d in draws for v in d]


def proof_bytes(proof):
    """every value of a proof as canonical bytes: P, pi (commitment and pivot), Q, y1..y3, outputs, L"""
    parts = [proof["z_commitment"][k].to_bytes() for k in ("P", "pi")]
    parts += [proof["pivot_proof"][k].to_bytes() for k in ("P", "pi", "Q")]
    parts += [(int(proof[k]) % N_ORDER).to_bytes(32, "little") for k in ("y1", "y2", "y3")]
    parts += [(int(v) % N_ORDER).to_bytes(32, "little") for v in proof["outputs"]]
    parts += [v.to_bytes(32, "little") for v in proof["L"].coeffs.to_ints()]
    parts.append((int(proof["L"].constant) % N_ORDER).to_bytes(32, "little"))
    return b"".join(parts)


def assert_same(got, want):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w) and sorted(g["pivot_proof"]) == ["P", "Q", "pi"], p
        assert type(g["y1"]) is type(w["y1"]) and type(g["L"].constant) is type(w["L"].constant), p
        assert proof_bytes(g) == proof_bytes(w), p


_MADE = {}


def make_case(vm, mods, case, K):
    """circuit, K inputs, pp, K draws and the K single proofs under those draws (the yardstick), once per (case, K);
    a smaller K of the same case is a prefix of the larger one's inputs and draws"""
    if (case, K) in _MADE:
        return _MADE[case, K]
    cs, koe = mods
    seed, n_x, m, n_out = case
    rng = random.Random(seed)
    A, B, O = F.random_circuit(rng, n_x, m, n_out)
    sc = cs.SparseCircuit(n_x, fref.to_csr(A), fref.to_csr(B), fref.to_csr(O), order=N_ORDER)
    n_z = n_x + 3 + 2 * m
    pp, trap = setup(vm, koe, n_z, seed)
    rng = random.Random(seed + 77)
    xs = [[rng.randrange(N_ORDER) for _ in range(n_x)] for _ in range(K)]
    xs[-1][0] = N_ORDER - 1
    draws = [[rng.randrange(1, N_ORDER) for _ in range(3)] for _ in range(K)]
    gf = vm.GF(N_ORDER)
    singles = []
    for x, d in zip(xs, draws):
        cs.prng = Replay(d)
        singles.append(cs.circuit_sat_prover(pp, sc, x, gf, vm.PivotChoice.koe))
        assert cs.prng.draws == []
    _MADE[case, K] = SimpleNamespace(A=A, B=B, O=O, xs=xs, sc=sc, pp=pp, trap=trap, draws=draws, gf=gf, singles=singles,
                                     n_z=n_z, n_x=n_x, m=m)
    return _MADE[case, K]


def prefix(c, K):
    return SimpleNamespace(**{**vars(c), "xs": c.xs[:K], "draws": c.draws[:K], "singles": c.singles[:K]})


def run_batch(vm, cs, c, xs=None, **kw):
    cs.prng = Replay(flat(c.draws))
    proofs = cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs if xs is None else xs, c.gf, vm.PivotChoice.koe, **kw)
    assert cs.prng.draws == []
    return proofs


# ---- 1. equality with K single calls; 4. the proofs verify -----------------------------------------------------------------
_BATCHES = {}


def small_batch(vm, mods, K):
    if K not in _BATCHES:
        c = prefix(make_case(vm, mods, SMALL, K_MAX), K)
        _BATCHES[K] = (c, run_batch(vm, mods[0], c))
    return _BATCHES[K]


@pytest.mark.parametrize("K", [1, 2, K_MAX])
def test_batch_equals_single_calls_byte_for_byte(vm, mods, K):
    c, batch = small_batch(vm, mods, K)
    assert len(batch) == K and len(batch[0]["L"].coeffs) == 14
    assert_same(batch, c.singles)
    # the pivot's P and pi ARE the commitment's
    for proof in batch:
        assert all(proof["pivot_proof"][k].to_bytes() == proof["z_commitment"][k].to_bytes() for k in ("P", "pi"))
    # distinct witnesses, distinct proofs: no row was proved twice
    assert len({proof_bytes(p) for p in batch}) == K


def test_every_proof_verifies_alone_and_together(vm, mods):
    cs, _ = mods
    c, batch = small_batch(vm, mods, K_MAX)
    for proof in batch:
        assert cs.circuit_sat_verifier(proof, c.pp, c.sc, c.gf, vm.PivotChoice.koe) == ALL_TRUE
    assert cs.circuit_sat_verifier_batch(batch, c.pp, c.sc, c.gf) == [ALL_TRUE] * K_MAX
    # the proof of x_1 presented beside the outputs of another input: exactly that position fails
    assert [int(v) for v in batch[1]["outputs"]] != [int(v) for v in batch[5]["outputs"]]
    swapped = list(batch)
    swapped[1] = dict(batch[1], outputs=batch[5]["outputs"])
    verdicts = cs.circuit_sat_verifier_batch(swapped, c.pp, c.sc, c.gf)
    assert verdicts[1] == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": False}
    assert [v for i, v in enumerate(verdicts) if i != 1] == [ALL_TRUE] * (K_MAX - 1)


# ---- 2. the CPU restatement ----------------------------------------------------------------------------------------------------
def test_first_and_last_witness_are_the_cpu_restatements(vm, mods):
    cs, _ = mods
    K = 3
    c, batch = small_batch(vm, mods, K)
    for p in (0, K - 1):
        proof, (r_a, r_b, gamma) = batch[p], c.draws[p]

        def commit(z, gamma=gamma):
            P_exp, pi_exp = c.trap.commitment(z, gamma)
            return bn.g1_to_bytes(bn.E1.mul(P_exp, bn.G1)), bn.g2_to_bytes(bn.E2.mul(pi_exp, bn.G2))
        want = F.prove_koe(c.n_x, c.A, c.B, c.O, c.xs[p], r_a, r_b, commit)
        assert [int(proof[k]) % N_ORDER for k in ("y1", "y2", "y3")] == want["y"], p
        assert [int(v) % N_ORDER for v in proof["outputs"]] == want["outputs"], p
        assert proof["L"].coeffs.to_ints() == want["L"] and int(proof["L"].constant) % N_ORDER == want["L_const"], p
        P_bytes, pi_bytes = commit(want["z"])
        Q_exp, u = c.trap.opening_by_evaluation(want["L"], want["z"], gamma)
        assert (u + want["L_const"]) % N_ORDER == 0
        assert proof["z_commitment"]["P"].to_bytes() == P_bytes == proof["pivot_proof"]["P"].to_bytes(), p
        assert proof["z_commitment"]["pi"].to_bytes() == pi_bytes == proof["pivot_proof"]["pi"].to_bytes(), p
        assert proof["pivot_proof"]["Q"].to_bytes() == bn.g1_to_bytes(bn.E1.mul(Q_exp, bn.G1)), p


# ---- 3. edge circuits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGES, ids=[f"nx{c[1]}_m{c[2]}_out{c[3]}" for c in EDGES])
def test_edge_circuits(vm, mods, case):
    c = make_case(vm, mods, case, 3)
    batch = run_batch(vm, mods[0], c)
    assert len(batch[0]["L"].coeffs) == c.n_z
    assert_same(batch, c.singles)


# ---- 5. chunks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", ["protocol_8", "opening"])
def test_a_chunk_boundary_changes_no_byte(vm, mods, monkeypatch, layer):
    cs, koe = mods
    K = 5
    c = prefix(make_case(vm, mods, SMALL, K_MAX), K)
    ctx = c.sc.device()["ctx"]
    sizes = []
    if layer == "protocol_8":
        two, three = cs._batch_bytes(c.sc, c.n_x, 2), cs._batch_bytes(c.sc, c.n_x, 3)
        assert two < three
        monkeypatch.setattr(cs, "BATCH_BUDGET_BYTES", two)
        assert cs._chunk_size(c.sc, c.n_x, K) == 2
        real = cs._prove_chunk
        monkeypatch.setattr(cs, "_prove_chunk", lambda *a: sizes.append(len(a[4])) or real(*a))
    else:
        two, three = koe.prove_batch_bytes(c.n_z, 2), koe.prove_batch_bytes(c.n_z, 3)
        assert two < three
        monkeypatch.setattr(koe, "PROVE_BATCH_BUDGET_BYTES", two)
        assert koe.prove_chunk_size(c.n_z, K) == 2
        real = ctx.bn256_koe_split_batch
        monkeypatch.setattr(ctx, "bn256_koe_split_batch", lambda *a: sizes.append(a[3]) or real(*a))
    split = run_batch(vm, cs, c)
    assert sizes == [2, 2, 1]
    assert_same(split, c.singles)


# ---- 6. modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["poly_product", "cs_extension"])
def test_ntt_modes_give_the_default_modes_bytes(vm, mods, mode):
    c = make_case(vm, mods, M65, 3)
    default = run_batch(vm, mods[0], c)
    with getattr(vm.device, mode)("ntt"):
        under = run_batch(vm, mods[0], c)
    assert [proof_bytes(p) for p in under] == [proof_bytes(p) for p in default]
    assert_same(under, c.singles)


# ---- 7. input shapes ---------------------------------------------------------------------------------------------------------
def test_lists_an_array_and_a_device_vector_give_the_same_proofs(vm, mods):
    cs, _ = mods
    K = 3
    c = prefix(make_case(vm, mods, SMALL, K_MAX), K)
    arr = np.stack([np.frombuffer(b"".join(v.to_bytes(32, "little") for v in x), np.uint8).reshape(-1, 32) for x in c.xs])
    assert arr.shape == (K, c.n_x, 32)
    on_device = vm.device.BnScalarVector.from_array(arr.reshape(-1, 32))
    assert_same(run_batch(vm, cs, c, arr), c.singles)
    assert_same(run_batch(vm, cs, c, on_device, n_in=c.n_x), c.singles)
    # a word above the order stands for its residue, in the array as in a list
    big = arr.copy()
    v = c.xs[0][1] + N_ORDER
    assert v < 1 << 256
    big[0, 1] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    assert_same(run_batch(vm, cs, c, big), c.singles)
    with pytest.raises(ValueError, match="n_in="):
        run_batch(vm, cs, c, on_device)
    with pytest.raises(ValueError, match="BnScalarVector"):
        run_batch(vm, cs, c, vm.ScalarVector.from_ints([1] * (K * c.n_x)), n_in=c.n_x)
    # the layer below returns the single call's tuple per witness, z a BnScalarVector of N scalars
    cs.prng = Replay(flat(c.draws))
    res = cs.protocol_8_excl_pivot_prover_batch(c.pp, c.sc, c.xs, c.gf)
    assert len(res) == K
    for (proof, zc, L, z, gamma), d, single in zip(res, c.draws, c.singles):
        assert gamma == d[2] and type(z).__name__ == "BnScalarVector" and len(z) == c.n_z and "pivot_proof" not in proof
        assert zc["P"].to_bytes() == single["z_commitment"]["P"].to_bytes()
        assert L.coeffs.to_ints() == single["L"].coeffs.to_ints()
        assert L.coeffs.dot(z) == (-int(L.constant)) % N_ORDER            # L(z) = 0


# ---- 8. gamma_witnesses --------------------------------------------------------------------------------------------------------
def test_gamma_witnesses_are_checked_per_witness(vm, mods):
    cs, _ = mods
    K = 3
    c = prefix(make_case(vm, mods, SMALL, K_MAX), K)
    gammas = [list(F.triples(c.n_x, c.A, c.B, x)[2]) for x in c.xs]
    assert_same(run_batch(vm, cs, c, gamma_witnesses=gammas), c.singles)
    gammas[1][2] = (gammas[1][2] + 1) % N_ORDER
    cs.prng = Replay(flat(c.draws))
    with pytest.raises(ValueError, match=r"gamma_witnesses\[1\]: multiplication gate 2 is not the product"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs, c.gf, "koe", gamma_witnesses=gammas)
    cs.prng = Replay(flat(c.draws))
    with pytest.raises(ValueError, match="gamma_witnesses: 3 lists of 3 gate outputs"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs, c.gf, "koe", gamma_witnesses=gammas[:2])


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_are_the_single_provers(vm, mods):
    cs, koe = mods
    K = 2
    c = prefix(make_case(vm, mods, SMALL, K_MAX), K)
    with pytest.raises(NotImplementedError, match="only the compact transcript is built"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs, c.gf, "koe", transcript="reference")
    with pytest.raises(NotImplementedError, match="only the compact transcript is built"):
        cs.protocol_8_excl_pivot_prover_batch(c.pp, c.sc, c.xs, c.gf, transcript="reference")
    short, _ = setup(vm, koe, c.n_z - 1, 1)
    cs.prng = Replay(flat(c.draws))
    with pytest.raises(AssertionError, match=r"Requirement does not hold: 2\*len\(x\)-1 <= number of generators"):
        cs.circuit_sat_prover_batch(short, c.sc, c.xs, c.gf, "koe")
    long, _ = setup(vm, koe, c.n_z + 1, 2)
    cs.prng = Replay(flat(c.draws))
    with pytest.raises(AssertionError):
        cs.circuit_sat_prover_batch(long, c.sc, c.xs, c.gf, "koe")
    over_l = cs.SparseCircuit(5, fref.to_csr(c.A), fref.to_csr(c.B), fref.to_csr(c.O))
    with pytest.raises(ValueError, match="circuit's order"):
        cs.circuit_sat_prover_batch(c.pp, over_l, c.xs, c.gf, "koe")
    with pytest.raises(ValueError, match="gf.order"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs, vm.GF(fref.ELL), "koe")
    with pytest.raises(ValueError, match="goes with PivotChoice.koe"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs, c.gf, "compressed")
    with pytest.raises(ValueError, match="the circuit has 5 inputs, 4 given"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, [x[:4] for x in c.xs], c.gf, "koe")
    cs.prng = Replay([])
    assert cs.circuit_sat_prover_batch(c.pp, c.sc, [], c.gf, "koe") == []
    assert cs.circuit_sat_prover_batch(c.pp, c.sc, np.zeros((0, 5, 32), np.uint8), c.gf, "koe") == []
    assert cs.protocol_8_excl_pivot_prover_batch(c.pp, c.sc, [], c.gf) == []


def test_challenge_on_a_node_names_the_witness(vm, mods, monkeypatch):
    cs, _ = mods
    K = 3
    c = prefix(make_case(vm, mods, SMALL, K_MAX), K)
    real, seen = cs.first_challenge, []

    def challenge(digest, order):
        seen.append(digest)
        return 2 * c.m if len(seen) == 2 else real(digest, order)
    monkeypatch.setattr(cs, "first_challenge", challenge)
    cs.prng = Replay(flat(c.draws))
    with pytest.raises(cs.ChallengeOnNode, match="witness 1: the first challenge 6 is an interpolation node"):
        cs.circuit_sat_prover_batch(c.pp, c.sc, c.xs, c.gf, "koe")


# ---- 10. the Ed25519 batch is what it was --------------------------------------------------------------------------------------
def test_ed25519_batch_still_equals_single_calls(vm, mods, monkeypatch):
    from verifiable_mpc_amd import wire
    cs, _ = mods
    ELL, K, seed = ref_l.ELL, 3, 4021
    rng = random.Random(seed)
    A, B, O = ref_l.random_circuit(rng, 5, 3, 2)
    sc = ref_l.sparse(5, A, B, O)
    xs = [sc.pad([rng.randrange(ELL) for _ in range(5)]) for _ in range(K)]
    N = len(xs[0]) + 3 + 2 * 3
    group = vm.EllipticCurve("Ed25519", "projective")
    gens = {"g": vm.PointVector.fixed_base(group.generator, [rng.randrange(1, ELL) for _ in range(N)]),
            "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ELL))}
    gf = vm.GF(group.order)

    def under_seeds(fn):
        monkeypatch.setattr(cs, "prng", random.Random(seed))
        monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(seed + 1))
        return fn()
    singles = under_seeds(lambda: [cs.circuit_sat_prover(gens, sc, x, gf) for x in xs])
    batch = under_seeds(lambda: cs.circuit_sat_prover_batch(gens, sc, xs, gf))
    assert len(batch) == K
    for got, want in zip(batch, singles):
        assert list(got) == list(want)
        assert wire.compress_point(got["z_commitment"]) == wire.compress_point(want["z_commitment"])
        assert [int(got[k]) % ELL for k in ("y1", "y2", "y3")] == [int(want[k]) % ELL for k in ("y1", "y2", "y3")]
        assert [int(o) % ELL for o in got["outputs"]] == [int(o) % ELL for o in want["outputs"]]
        assert type(got["L"].coeffs).__name__ == "ScalarVector"
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
                assert wire.compress_point(gp[k]) == wire.compress_point(wp[k]), k
    assert vm.circuit_sat_verifier_batch(batch, gens, sc, gf) == \
        [{"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True, "pivot_verification": True}] * K
