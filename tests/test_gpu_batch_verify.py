"""protocol_5_verifier_batch and its two callers against the single verifiers: the same answers, element for element -
with one N-term MSM for the whole batch (compact transcript, device forms), located bad proofs, and the fall-back loop
where a batch buys nothing."""
import random

import numpy as np
import pytest

from tests import p8_ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
ELL = p8_ref.ELL
P25519 = 2**255 - 19
K_MAX = 5


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def crs(vm):
    rng = random.Random(1717)
    group = vm.EllipticCurve("Ed25519", "projective")
    g = vm.PointVector.fixed_base(group.generator, [rng.randrange(1, ELL) for _ in range(63)], keep_proj=False)
    return {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ELL)),
            "gf": vm.GF(group.order)}


def gens_for(crs, n):
    return {"g": crs["g"][:n], "h": crs["h"], "k": crs["k"]}


def make_statements(vm, gens, gf, n, count, seed, transcript="compact"):
    """`count` statements (P, L, y, proof) over one CRS, each with its own x, L and P"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        x = vm.ScalarVector.from_ints([rng.randrange(ELL) for _ in range(n)])
        L = vm.pivot.LinearForm(vm.ScalarVector.from_ints([rng.randrange(ELL) for _ in range(n)]))
        gamma = rng.randrange(1, ELL)
        P = vm.pivot.vector_commitment(x, gamma, gens["g"], gens["h"])
        y = gf(L(x))
        out.append((P, L, y, vm.compressed_pivot.protocol_5_prover(gens, P, L, y, x, gamma, gf, transcript=transcript)))
    return out


@pytest.fixture(scope="module")
def proved(vm, crs):
    """five valid compact statements per n + 1 in {4, 16, 64}, made once and never changed (the tests copy what they alter)"""
    return {n: (gens_for(crs, n), make_statements(vm, gens_for(crs, n), crs["gf"], n, K_MAX, 9000 + n)) for n in (3, 15, 63)}


def singles(vm, gens, statements, gf, transcript="compact"):
    return [vm.compressed_pivot.protocol_5_verifier(gens, P, L, y, proof, gf, transcript=transcript)
            for P, L, y, proof in statements]


def batch(vm, gens, statements, gf, **kw):
    return vm.protocol_5_verifier_batch(gens, statements, gf, transcript=kw.pop("transcript", "compact"), **kw)


def count_kernel_calls(vm, monkeypatch):
    calls = []
    real = vm._native.Context.fr_batch_products
    monkeypatch.setattr(vm._native.Context, "fr_batch_products", lambda self, K, *a: calls.append(K) or real(self, K, *a))
    return calls


@pytest.mark.parametrize("n", [3, 15, 63])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_valid_proofs_one_combined_check(vm, crs, proved, monkeypatch, n, K):
    gens, statements = proved[n]
    statements = statements[:K]
    calls = count_kernel_calls(vm, monkeypatch)
    assert batch(vm, gens, statements, crs["gf"]) == [True] * K
    assert calls == [K]                                  # one combined check, no bisection
    assert singles(vm, gens, statements, crs["gf"]) == [True] * K
    # fixed weights: the weight must enter u, Gamma and Q alike
    weights = ([ELL - 1, 1 << 128, 1] + [7] * K)[:K]
    assert batch(vm, gens, statements, crs["gf"], weights=weights) == [True] * K


def tampered(vm, statements, i, kind):
    P, L, y, proof = statements[i]
    proof = dict(proof)
    if kind == "z_prime":
        proof["z_prime"] = [proof["z_prime"][0] + 1, proof["z_prime"][1]]
    elif kind == "swap":
        proof["A1"], proof["B1"] = proof["B1"], proof["A1"]
    elif kind == "t":
        proof["t"] = proof["t"] + 1
    elif kind == "y":
        y = y + 1
    elif kind == "P":
        P = statements[(i + 1) % len(statements)][0]
    elif kind == "small_order":
        two = vm.Ed25519Point.from_affine_bytes((0).to_bytes(32, "little") + (P25519 - 1).to_bytes(32, "little"))
        proof["A"] = vm.Ed25519Point.operation(proof["A"], two)             # (0, -1) has order 2
    elif kind == "fewer_rounds":
        last = max(int(key[1:]) for key in proof if key[0] == "A" and key[1:].isdigit())
        del proof["A" + str(last)], proof["B" + str(last)]
    elif kind == "more_rounds":
        last = max(int(key[1:]) for key in proof if key[0] == "A" and key[1:].isdigit())
        proof["A" + str(last + 1)], proof["B" + str(last + 1)] = proof["A0"], proof["B0"]
    else:
        raise ValueError(kind)
    return statements[:i] + [(P, L, y, proof)] + statements[i + 1:]


@pytest.mark.parametrize("kind", ["z_prime", "swap", "t", "y", "P", "small_order"])
@pytest.mark.parametrize("n,K,i", [(15, 5, 3), (63, 2, 0)])
def test_one_bad_proof_is_located(vm, crs, proved, kind, n, K, i):
    gens, statements = proved[n]
    bad = tampered(vm, statements[:K], i, kind)
    want = [j != i for j in range(K)]
    assert batch(vm, gens, bad, crs["gf"]) == want
    assert singles(vm, gens, bad, crs["gf"]) == want


@pytest.mark.parametrize("kind", ["fewer_rounds", "more_rounds"])
def test_wrong_round_count_is_false_and_leaves_the_batch(vm, crs, proved, monkeypatch, kind):
    gens, statements = proved[15]
    bad = tampered(vm, statements, 2, kind)
    calls = count_kernel_calls(vm, monkeypatch)
    assert batch(vm, gens, bad, crs["gf"]) == [True, True, False, True, True]
    assert calls == [4]                                  # removed before anything was combined


def test_small_order_point_leaves_the_batch(vm, crs, proved, monkeypatch):
    gens, statements = proved[15]
    bad = tampered(vm, statements, 0, "small_order")
    calls = count_kernel_calls(vm, monkeypatch)
    assert batch(vm, gens, bad, crs["gf"]) == [False, True, True, True, True]
    assert calls == [4]


def test_two_bad_proofs_among_five(vm, crs, proved, monkeypatch):
    gens, statements = proved[15]
    bad = tampered(vm, tampered(vm, statements, 1, "t"), 4, "z_prime")
    calls = count_kernel_calls(vm, monkeypatch)
    assert batch(vm, gens, bad, crs["gf"]) == [True, False, True, True, False]
    assert len(calls) <= 7 and calls[0] == 5            # bisection: 5 -> (2 | 3) -> singles
    assert batch(vm, gens, bad, crs["gf"], weights=[3, ELL - 1, 1 << 128, 1, 2]) == [True, False, True, True, False]


def test_weights_are_checked(vm, crs, proved):
    gens, statements = proved[3]
    with pytest.raises(ValueError, match="zero weight"):
        batch(vm, gens, statements[:2], crs["gf"], weights=[1, 0])
    with pytest.raises(ValueError, match="zero weight"):
        batch(vm, gens, statements[:2], crs["gf"], weights=[ELL, 1])
    with pytest.raises(ValueError, match="weights"):
        batch(vm, gens, statements[:2], crs["gf"], weights=[1])
    assert batch(vm, gens, [], crs["gf"]) == []


def test_shapes_without_a_batch_fall_back_to_the_loop(vm, crs, monkeypatch):
    gf = crs["gf"]
    calls = count_kernel_calls(vm, monkeypatch)
    # N = 2
    gens = gens_for(crs, 1)
    statements = make_statements(vm, gens, gf, 1, 2, 41)
    statements[1] = (statements[1][0], statements[1][1], statements[1][2] + 1, statements[1][3])
    assert batch(vm, gens, statements, gf) == singles(vm, gens, statements, gf) == [True, False]
    # the reference transcript at n = 3 (its text prints the generators' projective representatives)
    gens = dict(gens_for(crs, 3), g=vm.PointVector.fixed_base(crs["h"], [5, 7, 11], keep_proj=True))
    statements = make_statements(vm, gens, gf, 3, 2, 43, transcript="reference")
    statements[0] = (statements[0][0], statements[0][1], statements[0][2] + 1, statements[0][3])
    assert batch(vm, gens, statements, gf, transcript="reference") == \
        singles(vm, gens, statements, gf, transcript="reference") == [False, True]
    assert calls == []


# ---- the callers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,n", [(3, 7), (5, 15)])
def test_nullity_batch(vm, crs, capsys, s, n):
    nullity, gf = vm.nullity, crs["gf"]
    rng = random.Random(100 * s + n)
    gens = gens_for(crs, n)
    items = []
    for _ in range(3):
        x = [rng.randrange(1, ELL) for _ in range(n)]
        rows = []
        for _ in range(s):                              # forms that vanish at x
            row = [rng.randrange(ELL) for _ in range(n - 1)]
            rows.append(row + [-sum(a * b for a, b in zip(row, x)) * pow(x[-1], -1, ELL) % ELL])
        fm = vm.FormMatrix(np.frombuffer(b"".join(v.to_bytes(32, "little") for row in rows for v in row),
                                         np.uint8).reshape(s, n, 32).copy())
        xs = vm.ScalarVector.from_ints(x)
        gamma = rng.randrange(1, ELL)
        P = vm.pivot.vector_commitment(xs, gamma, gens["g"], gens["h"])
        proof, L, y, rho = nullity.prove_nullity_compressed(gens, P, fm, xs, gamma, gf)
        items.append((P, L, fm, rho, y, proof))
    assert nullity.verify_nullity_compressed_batch(gens, items, gf) == [True, True, True]
    P, L, fm, rho, y, proof = items[1]
    items[1] = (P, L, fm, (rho + 1) % ELL, y, proof)
    want = [nullity.verify_nullity_compressed(gens, *item, gf) for item in items]
    assert want == [True, False, True]
    assert vm.verify_nullity_compressed_batch(gens, items, gf) == want
    capsys.readouterr()


def test_circuit_sat_batch(vm, crs, monkeypatch):
    cs = vm.circuit_sat_gpu
    gf = crs["gf"]
    case = next(c for c in load_golden("p8_circuits.json")["cases"] if c["name"] == "padded")
    sc = cs.SparseCircuit.from_circuit(p8_ref.circuit_from_fixture(case, gf))
    rng = random.Random(88)
    xs = [sc.pad([rng.randrange(ELL) for _ in range(sc.n_x)]) for _ in range(3)]
    gens = gens_for(crs, len(xs[0]) + 3 + 2 * sc.m)
    proofs = [cs.circuit_sat_prover(gens, sc, x, gf, transcript="compact") for x in xs]
    all_true = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True, "pivot_verification": True}
    assert vm.circuit_sat_verifier_batch(proofs, gens, sc, gf, transcript="compact") == [all_true] * 3
    proofs[1] = dict(proofs[1], y3=proofs[1]["y3"] + 1)
    calls = count_kernel_calls(vm, monkeypatch)
    got = vm.circuit_sat_verifier_batch(proofs, gens, sc, gf, transcript="compact")
    assert got == [cs.circuit_sat_verifier(p, gens, sc, gf, transcript="compact") for p in proofs]
    assert got == [all_true, {"y1*y2=y3": False}, all_true]
    assert calls == [2]                                  # the altered proof never entered the batch
