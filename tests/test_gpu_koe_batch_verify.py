"""Batch verification of knowledge-of-exponent proofs: knowledge_of_exponent.
opening_linear_form_verifier_batch and the knowledge-of-exponent route of circuit_sat_gpu.circuit_sat_verifier_batch.

The contract is "the list of the single verifier's dicts", so the single verifiers are the reference (computed once per
pp and shared); what they themselves answer on honest and tampered proofs is the business of tests/test_gpu_koe.py and
tests/test_gpu_circuit_sat_koe.py.  The pp comes from setup_under with a fixed trapdoor."""
import random

import pytest

from oracle import bn256_ref as bn
from tests import test_gpu_circuit_sat_koe as cskoe

pytestmark = pytest.mark.gpu
N = bn.N
OK = {"restriction_arg_check": True, "PRQ_check": True}
K_MAX = 17


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def koe(vm):
    return vm.knowledge_of_exponent


@pytest.fixture(scope="module")
def mods(vm):
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    return cs, vm.knowledge_of_exponent


_OPENINGS = {}


def openings(vm, koe, n):
    """pp for forms of length n, K_MAX honest openings (coefficients, proof, u) and the single verifier's answers"""
    if n not in _OPENINGS:
        rng = random.Random(4000 + n)
        P = vm.pynocchio
        pp = koe.setup_under(P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2), n, rng.randrange(1, N), rng.randrange(1, N),
                             rng.randrange(1, N))
        items = []
        for _ in range(K_MAX):
            coeffs = [rng.randrange(N) for _ in range(n)]
            x, gamma = [rng.randrange(N) for _ in range(n)], rng.randrange(N)
            proof, u = koe.opening_linear_form_prover(vm.pivot.LinearForm(coeffs), x, gamma, pp)
            items.append((coeffs, proof, int(u)))
        singles = [koe.opening_linear_form_verifier(vm.pivot.LinearForm(c), pp, p, u) for c, p, u in items]
        assert singles == [OK] * K_MAX
        _OPENINGS[n] = (pp, items, singles)
    return _OPENINGS[n]


def forms(vm, items, kind):
    if kind == "device":
        return [vm.pivot.LinearForm(vm.device.BnScalarVector.from_ints(c)) for c, _, _ in items]
    return [vm.pivot.LinearForm(c) for c, _, _ in items]


@pytest.mark.parametrize("kind", ["device", "lists"])
@pytest.mark.parametrize("n", [8, 65])
@pytest.mark.parametrize("K", [1, 2, 17])
def test_batch_is_the_list_of_single_verifications(vm, koe, K, n, kind):
    pp, items, singles = openings(vm, koe, n)
    got = koe.opening_linear_form_verifier_batch(forms(vm, items[:K], kind), pp, [p for _, p, _ in items[:K]],
                                                 [u for _, _, u in items[:K]])
    assert got == singles[:K]


def test_mixed_device_and_list_forms_and_an_affine_form(vm, koe):
    pp, items, _ = openings(vm, koe, 8)
    sub = items[:4]
    Ls = forms(vm, sub[:2], "device") + forms(vm, sub[2:3], "lists") + [vm.pivot.AffineForm(sub[3][0], 5)]
    us = [u for _, _, u in sub[:3]] + [sub[3][2] + 5]
    proofs = [p for _, p, _ in sub]
    want = [koe.opening_linear_form_verifier(L, pp, p, u) for L, p, u in zip(Ls, proofs, us)]
    assert want == [OK] * 4
    assert koe.opening_linear_form_verifier_batch(Ls, pp, proofs, us) == want


def test_each_tampering_turns_its_own_check_at_its_own_index(vm, koe):
    pp, items, _ = openings(vm, koe, 8)
    K = 5
    Ls, proofs, us = forms(vm, items[:K], "lists"), [p for _, p, _ in items[:K]], [u for _, _, u in items[:K]]

    def both(proofs, us):
        got = koe.opening_linear_form_verifier_batch(Ls, pp, proofs, us)
        assert got == [koe.opening_linear_form_verifier(L, pp, p, u) for L, p, u in zip(Ls, proofs, us)]
        return got
    # one wrong u
    got = both(proofs, us[:2] + [us[2] + 1] + us[3:])
    assert got == [OK, OK, dict(OK, PRQ_check=False), OK, OK]
    # a pi taken from another proof
    got = both([proofs[0], dict(proofs[1], pi=proofs[4]["pi"])] + proofs[2:], us)
    assert got == [OK, dict(OK, restriction_arg_check=False), OK, OK, OK]
    # two proofs with their Q swapped
    swapped = list(proofs)
    swapped[1], swapped[3] = dict(proofs[1], Q=proofs[3]["Q"]), dict(proofs[3], Q=proofs[1]["Q"])
    got = both(swapped, us)
    assert got == [OK, dict(OK, PRQ_check=False), OK, dict(OK, PRQ_check=False), OK]


def test_empty_batch_mixed_lengths_and_a_point_off_its_curve(vm, koe):
    pp, items, _ = openings(vm, koe, 8)
    assert koe.opening_linear_form_verifier_batch([], pp, [], []) == []
    Ls, proofs, us = forms(vm, items[:5], "lists"), [p for _, p, _ in items[:5]], [u for _, _, u in items[:5]]
    short = vm.pivot.LinearForm(items[1][0][:7])
    with pytest.raises(ValueError, match="length"):
        koe.opening_linear_form_verifier_batch([Ls[0], short] + Ls[2:], pp, proofs, us)
    bad = list(proofs)
    bad[3] = dict(proofs[3], Q=vm.pynocchio.BN256Point((5, 7)))
    with pytest.raises(ValueError, match=r"proof 3: Q is not on the") as ei:
        koe.opening_linear_form_verifier_batch(Ls, pp, bad, us)
    # the single verifier's message, prefixed with the index
    with pytest.raises(ValueError) as single:
        koe.opening_linear_form_verifier(Ls[3], pp, bad[3], us[3])
    assert str(ei.value) == f"proof 3: {single.value}"


def count_pairing_launches(vm, monkeypatch):
    calls = []
    ctx_cls = vm._native.Context
    real = ctx_cls.bn256_pairing_product

    def counted(self, *args, **kw):
        calls.append(args[2])               # the number of pairs
        return real(self, *args, **kw)
    monkeypatch.setattr(ctx_cls, "bn256_pairing_product", counted)
    return calls


def test_opening_batch_is_one_pairing_launch(vm, koe, monkeypatch):
    pp, items, singles = openings(vm, koe, 8)
    Ls, proofs, us = forms(vm, items, "device"), [p for _, p, _ in items], [u for _, _, u in items]
    calls = count_pairing_launches(vm, monkeypatch)
    assert koe.opening_linear_form_verifier_batch(Ls, pp, proofs, us) == singles
    assert calls == [5 * K_MAX]
    # ... also when the rows budget cuts the sums R into chunks of three rows
    monkeypatch.setattr(koe, "BATCH_ROWS_BUDGET_BYTES", 3 * 32 * 8)
    del calls[:]
    assert koe.opening_linear_form_verifier_batch(Ls, pp, proofs, us) == singles
    assert calls == [5 * K_MAX]


# ---- the circuit batch ---------------------------------------------------------------------------------------------------
CIRCUIT_CASES = [(7, 4, 0, 1), (103, 5, 3, 2), (165, 5, 65, 2)]
_BATCHES = {}


def circuit_batch(vm, mods, case, monkeypatch):
    """five proofs of the case's circuit under its pp - honest; y3 altered; a coefficient of L altered; the pivot proof's
    P another point than the commitment's; another proof's Q - and the single verifier's answers"""
    cs, koe = mods
    c = cskoe.make_case(vm, mods, case)
    if case not in _BATCHES:
        rng = random.Random(case[0])
        monkeypatch.setattr(cs, "prng", random.Random(900 + case[0]))
        made = [c.proof] + [cs.circuit_sat_prover(c.pp, c.sc, [rng.randrange(N) for _ in range(case[1])], c.gf, "koe")
                            for _ in range(4)]
        co = made[2]["L"].coeffs.to_ints()
        co[len(co) // 2] = (co[len(co) // 2] + 1) % N
        pv = made[3]["pivot_proof"]
        proofs = [made[0],
                  cskoe.tampered(made[1], y3=made[1]["y3"] + 1),
                  cskoe.tampered(made[2], L=vm.pivot.AffineForm(type(made[2]["L"].coeffs).from_ints(co),
                                                                made[2]["L"].constant)),
                  cskoe.tampered(made[3], pivot_proof={**pv, "P": vm.pynocchio.BN256Point(bn.E1.add(pv["P"].coords,
                                                                                                    pv["P"].coords))}),
                  cskoe.tampered(made[4], pivot_proof={**made[4]["pivot_proof"], "Q": made[0]["pivot_proof"]["Q"]})]
        singles = [cs.circuit_sat_verifier(p, c.pp, c.sc, c.gf, vm.PivotChoice.koe) for p in proofs]
        assert singles[0] == cskoe.ALL_TRUE
        assert singles[1] == {"y1*y2=y3": False}
        assert singles[2] == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": False}
        assert singles[3]["pivot_verification"]["restriction_arg_check"] is False
        assert singles[4] == {**cskoe.ALL_TRUE, "pivot_verification": {"restriction_arg_check": True, "PRQ_check": False}}
        _BATCHES[case] = (proofs, singles)
    return (c,) + _BATCHES[case]


@pytest.mark.parametrize("case", CIRCUIT_CASES, ids=[f"nx{c[1]}_m{c[2]}_out{c[3]}" for c in CIRCUIT_CASES])
def test_circuit_batch_is_the_list_of_single_verifications(vm, mods, monkeypatch, case):
    cs, koe = mods
    c, proofs, singles = circuit_batch(vm, mods, case, monkeypatch)
    calls = count_pairing_launches(vm, monkeypatch)
    assert cs.circuit_sat_verifier_batch(proofs, c.pp, c.sc, c.gf) == singles
    assert calls == [15]                    # three of the five proofs get as far as the opening: one launch
    assert vm.circuit_sat_verifier_batch(proofs, c.pp, c.sc, c.gf, pivot_choice=vm.PivotChoice.koe) == singles
    assert cs.circuit_sat_verifier_batch([], c.pp, c.sc, c.gf) == []
    # chunks of 2, 2 and 1 proofs: the same answers, one launch per chunk
    monkeypatch.setattr(cs, "KOE_VERIFY_BUDGET_BYTES", 2 * 32 * c.n_z)
    del calls[:]
    assert cs.circuit_sat_verifier_batch(proofs, c.pp, c.sc, c.gf) == singles
    assert calls == [5, 5, 5]


def test_pivot_choice_and_generators_go_together(vm, mods, monkeypatch):
    cs, koe = mods
    c = cskoe.make_case(vm, mods, cskoe.SMALL)
    with pytest.raises(ValueError, match="goes with PivotChoice.koe") as batch:
        cs.circuit_sat_verifier_batch([c.proof], c.pp, c.sc, c.gf, pivot_choice="compressed")
    with pytest.raises(ValueError) as single:
        cs.circuit_sat_verifier(c.proof, c.pp, c.sc, c.gf, "compressed")
    assert str(batch.value) == str(single.value)
    # Ed25519 generators: "koe" is refused as by the single verifier, None is the call without the keyword
    from tests import test_gpu_circuit_sat_batch as csb
    group = vm.EllipticCurve("Ed25519", "projective")
    rng = random.Random(17)
    n_x, m, K = 4, 3, 2
    A, B, O, sc, xs, _ = csb.make_batch(23, n_x, m, 1, K)
    n_z = len(xs[0]) + 3 + 2 * m
    exps = [rng.randrange(1, group.order) for _ in range(n_z)]
    gens = {"g": vm.PointVector.fixed_base(group.generator, exps), "h": group.generator,
            "k": vm.Ed25519Point.repeat(group.generator, 0x1234567)}
    gf = vm.GF(group.order)
    monkeypatch.setattr(cs, "prng", random.Random(1))
    monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(2))
    proofs = [cs.circuit_sat_prover(gens, sc, x, gf) for x in xs]
    with pytest.raises(NotImplementedError, match="takes a pp") as batch:
        cs.circuit_sat_verifier_batch(proofs, gens, sc, gf, pivot_choice="koe")
    with pytest.raises(NotImplementedError) as single:
        cs.circuit_sat_verifier(proofs[0], gens, sc, gf, "koe")
    assert str(batch.value) == str(single.value)
    plain = cs.circuit_sat_verifier_batch(proofs, gens, sc, gf)
    assert plain == [csb.ALL_TRUE] * K
    assert cs.circuit_sat_verifier_batch(proofs, gens, sc, gf, pivot_choice=None) == plain
    assert cs.circuit_sat_verifier_batch(proofs, gens, sc, gf, pivot_choice="compressed") == plain
