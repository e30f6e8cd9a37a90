"""Protocol 8 over BN-256 with the knowledge-of-exponent pivot, end to end (circuit_sat_gpu over a SparseCircuit of the
BN-256 order, knowledge_of_exponent on device operands), against tests/p8_field_ref.py: the scalars of the proof
against the CPU restatement, its three points against the trapdoor's exponents times the generators
(oracle/bn256_ref.py, independent of the kernels), the verifier on honest and on tampered proofs.

All draws are replayed: the setup's (g_exp, alpha, s) through knowledge_of_exponent.prng, the prover's (r_a, r_b, gamma)
through circuit_sat_gpu.prng.  N = n_in + 3 + 2m is never padded: (5, 3, 2) gives N = 14."""
import random
from types import SimpleNamespace

import pytest

from oracle import bn256_ref as bn
from tests import p8_field_ref as fref

pytestmark = pytest.mark.gpu

N_ORDER = fref.BN_N
F = fref.P8(N_ORDER)
ALL_TRUE = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True,
            "pivot_verification": {"restriction_arg_check": True, "PRQ_check": True}}
# (seed, n_x, m, n_out)
CASES = [(7, 4, 0, 1), (8, 6, 9, 0)] + [(100 + m, 5, m, 2) for m in (1, 2, 3, 63, 64, 65, 1000)]
SMALL = (103, 5, 3, 2)


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


def g1_point(vm):
    return vm.pynocchio.BN256Point(bn.G1)


def g2_point(vm):
    return vm.pynocchio.BN256TwistPoint(bn.G2)


def setup(vm, koe, n_z, seed):
    """(pp for vectors of n_z scalars, its trapdoor)"""
    rng = random.Random(5000 + seed)
    g_exp, alpha, s = rng.randrange(1, N_ORDER), rng.randrange(N_ORDER), rng.randrange(N_ORDER)
    koe.prng = Replay([g_exp, alpha, s])
    pp = koe.trusted_setup(g1_point(vm), g2_point(vm), n_z, N_ORDER)
    assert koe.prng.draws == []
    return pp, fref.KoeTrapdoor(g_exp, alpha, s)


def g1_bytes(e):
    return bn.g1_to_bytes(bn.E1.mul(e, bn.G1))


def g2_bytes(e):
    return bn.g2_to_bytes(bn.E2.mul(e, bn.G2))


_MADE = {}


def make_case(vm, mods, case):
    """circuit, inputs, pp, the proof of the default modes and the restatement's values, once per case"""
    if case in _MADE:
        return _MADE[case]
    cs, koe = mods
    seed, n_x, m, n_out = case
    rng = random.Random(seed)
    A, B, O = F.random_circuit(rng, n_x, m, n_out)
    x = [rng.randrange(N_ORDER) for _ in range(n_x)]
    sc = cs.SparseCircuit(n_x, fref.to_csr(A), fref.to_csr(B), fref.to_csr(O), order=N_ORDER)
    n_z = n_x + 3 + 2 * m
    pp, trap = setup(vm, koe, n_z, seed)
    draws = [rng.randrange(1, N_ORDER) for _ in range(3)]          # r_a, r_b, gamma
    gf = vm.GF(N_ORDER)
    cs.prng = Replay(draws)
    proof = cs.circuit_sat_prover(pp, sc, x, gf, vm.PivotChoice.koe)
    assert cs.prng.draws == []

    def commit(z):
        P_exp, pi_exp = trap.commitment(z, draws[2])
        return g1_bytes(P_exp), g2_bytes(pi_exp)
    want = F.prove_koe(n_x, A, B, O, x, draws[0], draws[1], commit)
    _MADE[case] = SimpleNamespace(A=A, B=B, O=O, x=x, sc=sc, pp=pp, trap=trap, draws=draws, gf=gf, proof=proof, want=want,
                                  n_z=n_z)
    return _MADE[case]


def proof_bytes(proof):
    """every value of a proof as canonical bytes"""
    parts = [proof["z_commitment"][k].to_bytes() for k in ("P", "pi")]
    parts += [proof["pivot_proof"][k].to_bytes() for k in ("P", "pi", "Q")]
    parts += [(int(proof[k]) % N_ORDER).to_bytes(32, "little") for k in ("y1", "y2", "y3")]
    parts += [(int(v) % N_ORDER).to_bytes(32, "little") for v in proof["outputs"]]
    parts += [v.to_bytes(32, "little") for v in proof["L"].coeffs.to_ints()]
    parts.append((int(proof["L"].constant) % N_ORDER).to_bytes(32, "little"))
    return b"".join(parts)


@pytest.mark.parametrize("case", CASES, ids=[f"nx{c[1]}_m{c[2]}_out{c[3]}" for c in CASES])
def test_proof_is_the_restatements_and_verifies(vm, mods, case):
    cs, koe = mods
    c = make_case(vm, mods, case)
    proof, want = c.proof, c.want
    n_x, m = case[1], case[2]
    assert len(proof["L"].coeffs) == c.n_z == n_x + 3 + 2 * m           # no padding
    assert len(c.pp["pp_lhs"]) == 2 * c.n_z
    assert isinstance(proof["z_commitment"], dict) and sorted(proof["pivot_proof"]) == ["P", "Q", "pi"]
    # the scalars
    assert [int(proof[k]) % N_ORDER for k in ("y1", "y2", "y3")] == want["y"]
    assert [int(v) % N_ORDER for v in proof["outputs"]] == want["outputs"]
    assert proof["L"].coeffs.to_ints() == want["L"]
    assert int(proof["L"].constant) % N_ORDER == want["L_const"]
    # both challenges, from the proof's own bytes
    zc = proof["z_commitment"]
    digest = cs._first_digest(zc, c.sc, n_x)
    assert c.sc.digest == F.circuit_digest(n_x, c.A, c.B, c.O)
    assert cs.first_challenge(digest, N_ORDER) == want["c"] == \
        F.koe_first_challenge(zc["P"].to_bytes(), zc["pi"].to_bytes(), c.sc.digest, n_x)[0]
    assert cs._second_challenge(digest, want["y"], want["outputs"], N_ORDER, cs._Koe.second_tag) == want["rho"]
    # the points: the trapdoor's exponents times the generators
    P_exp, pi_exp = c.trap.commitment(want["z"], c.draws[2])
    Q_exp, u = c.trap.opening_by_evaluation(want["L"], want["z"], c.draws[2])
    assert (u + want["L_const"]) % N_ORDER == 0                         # L(z) = 0: what the pivot opens to
    assert zc["P"].to_bytes() == g1_bytes(P_exp) == proof["pivot_proof"]["P"].to_bytes()
    assert zc["pi"].to_bytes() == g2_bytes(pi_exp) == proof["pivot_proof"]["pi"].to_bytes()
    assert proof["pivot_proof"]["Q"].to_bytes() == g1_bytes(Q_exp)
    assert c.trap.restriction_check(P_exp, pi_exp) and c.trap.prq_check(want["L"], P_exp, Q_exp, u)
    # and the verifier
    assert cs.circuit_sat_verifier(proof, c.pp, c.sc, c.gf, vm.PivotChoice.koe) == ALL_TRUE


def test_z_on_the_device_is_the_restatements(vm, mods):
    cs, _ = mods
    c = make_case(vm, mods, SMALL)
    cs.prng = Replay(c.draws[:2])
    z = cs._witness_on_device(c.sc, c.x, N_ORDER)
    assert type(z).__name__ == "BnScalarVector" and z.to_ints() == c.want["z"] and len(z) == 14


def test_pivot_part_is_three_points_of_256_bytes(vm, mods):
    c = make_case(vm, mods, (1100, 5, 1000, 2))
    assert sum(len(c.proof["pivot_proof"][k].to_bytes()) for k in ("P", "pi", "Q")) == 256


def tampered(proof, **changes):
    out = dict(proof)
    out.update(changes)
    return out


def test_tampering_turns_exactly_its_own_key(vm, mods):
    cs, koe = mods
    c = make_case(vm, mods, SMALL)
    proof, gf, P = c.proof, c.gf, vm.pynocchio
    verify = lambda p: cs.circuit_sat_verifier(p, c.pp, c.sc, gf, "koe")           # noqa: E731
    assert verify(proof) == ALL_TRUE
    # y3: the product check, and nothing after it is run
    assert verify(tampered(proof, y3=proof["y3"] + 1)) == {"y1*y2=y3": False}
    # an output, a coefficient of L, the constant of L: L is no longer the forms' combination
    not_L = {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": False}
    assert verify(tampered(proof, outputs=[proof["outputs"][0] + 1, proof["outputs"][1]])) == not_L
    for pos in (0, 7, 13):
        co = proof["L"].coeffs.to_ints()
        co[pos] = (co[pos] + 1) % N_ORDER
        bad_L = vm.pivot.AffineForm(type(proof["L"].coeffs).from_ints(co), proof["L"].constant)
        assert verify(tampered(proof, L=bad_L)) == not_L, pos
    assert verify(tampered(proof, L=vm.pivot.AffineForm(proof["L"].coeffs, proof["L"].constant + 1))) == not_L
    # the three points of the pivot, one at a time, each replaced by another point of its group
    pv = proof["pivot_proof"]
    twice = lambda pt: P.BN256Point(bn.E1.add(pt.coords, pt.coords))               # noqa: E731
    pi2 = bn.E2.add(*[((pv["pi"].coords[0], pv["pi"].coords[1]), (pv["pi"].coords[2], pv["pi"].coords[3]))] * 2)
    pi2 = P.BN256TwistPoint((*pi2[0], *pi2[1]))
    got = verify(tampered(proof, pivot_proof={**pv, "P": twice(pv["P"])}))
    assert {k: v for k, v in got.items() if k != "pivot_verification"} == {k: True for k in list(ALL_TRUE)[:2]}
    assert got["pivot_verification"]["restriction_arg_check"] is False
    got = verify(tampered(proof, pivot_proof={**pv, "pi": pi2}))
    assert got["pivot_verification"] == {"restriction_arg_check": False, "PRQ_check": True}
    got = verify(tampered(proof, pivot_proof={**pv, "Q": twice(pv["Q"])}))
    assert got == {**ALL_TRUE, "pivot_verification": {"restriction_arg_check": True, "PRQ_check": False}}
    # the commitment itself: another first challenge, another L
    assert verify(tampered(proof, z_commitment={"P": twice(pv["P"]), "pi": pv["pi"]})) == not_L


def test_pp_of_the_wrong_length(vm, mods):
    cs, koe = mods
    c = make_case(vm, mods, SMALL)
    short, _ = setup(vm, koe, c.n_z - 1, 1)
    cs.prng = Replay(c.draws)
    with pytest.raises(AssertionError, match=r"Requirement does not hold: 2\*len\(x\)-1 <= number of generators"):
        cs.circuit_sat_prover(short, c.sc, c.x, c.gf, "koe")
    long, _ = setup(vm, koe, c.n_z + 1, 2)
    cs.prng = Replay(c.draws)
    with pytest.raises(AssertionError):
        cs.circuit_sat_prover(long, c.sc, c.x, c.gf, "koe")


def test_gamma_witness_is_checked(vm, mods):
    cs, _ = mods
    c = make_case(vm, mods, SMALL)
    gamma = list(c.want["gamma"])
    cs.prng = Replay(c.draws)
    assert proof_bytes(cs.circuit_sat_prover(c.pp, c.sc, c.x, c.gf, "koe", gamma_witness=gamma)) == proof_bytes(c.proof)
    gamma[1] = (gamma[1] + 1) % N_ORDER
    cs.prng = Replay(c.draws)
    with pytest.raises(ValueError, match="multiplication gate 1 is not the product"):
        cs.circuit_sat_prover(c.pp, c.sc, c.x, c.gf, "koe", gamma_witness=gamma)


@pytest.mark.parametrize("case", [SMALL, (165, 5, 65, 2)], ids=["m3", "m65"])
def test_ntt_modes_give_the_same_proof_bytes(vm, mods, case):
    cs, _ = mods
    c = make_case(vm, mods, case)
    cs.prng = Replay(c.draws)
    with vm.device.cs_extension("ntt"), vm.device.poly_product("ntt"):
        proof = cs.circuit_sat_prover(c.pp, c.sc, c.x, c.gf, "koe")
        assert cs.circuit_sat_verifier(proof, c.pp, c.sc, c.gf, "koe") == ALL_TRUE
    assert proof_bytes(proof) == proof_bytes(c.proof)


def test_fields_and_generators_must_go_together(vm, mods):
    cs, _ = mods
    c = make_case(vm, mods, SMALL)
    over_l = cs.SparseCircuit(5, fref.to_csr(c.A), fref.to_csr(c.B), fref.to_csr(c.O))
    assert over_l.digest != c.sc.digest
    with pytest.raises(ValueError, match="circuit's order"):
        cs.circuit_sat_prover(c.pp, over_l, c.x, c.gf, "koe")
    with pytest.raises(ValueError, match="gf.order"):
        cs.circuit_sat_prover(c.pp, c.sc, c.x, vm.GF(fref.ELL), "koe")
    with pytest.raises(ValueError, match="goes with PivotChoice.koe"):
        cs.circuit_sat_prover(c.pp, c.sc, c.x, c.gf, "compressed")
    with pytest.raises(ValueError, match="circuit's order"):
        cs.circuit_sat_verifier(c.proof, c.pp, over_l, c.gf, "koe")
    with pytest.raises(NotImplementedError, match="compact transcript"):
        cs.circuit_sat_prover(c.pp, c.sc, c.x, c.gf, "koe", transcript="reference")
    with pytest.raises(NotImplementedError, match="compact transcript"):
        cs.circuit_sat_verifier(c.proof, c.pp, c.sc, c.gf, "koe", transcript="reference")
    with pytest.raises(ValueError, match="order is neither"):
        cs.SparseCircuit(5, fref.to_csr(c.A), fref.to_csr(c.B), order=97)


@pytest.mark.parametrize("as_groups", [False, True], ids=["points", "groups"])
def test_create_generators_yields_a_pp_the_prover_accepts(vm, mods, as_groups):
    cs, koe = mods
    c = make_case(vm, mods, SMALL)
    g1, g2 = g1_point(vm), g2_point(vm)
    group = [SimpleNamespace(generator=g1, order=N_ORDER), SimpleNamespace(generator=g2, order=N_ORDER)] if as_groups \
        else [g1, g2]
    koe.prng = random.Random(11)
    pp = vm.create_generators(c.n_z, vm.PivotChoice.koe, group)
    assert sorted(pp) == ["pp_lhs", "pp_rhs"] and len(pp["pp_lhs"]) == len(pp["pp_rhs"]) == 2 * c.n_z
    cs.prng = random.Random(12)
    proof = vm.circuit_sat_prover(pp, c.sc, c.x, c.gf, vm.PivotChoice.koe)
    assert vm.circuit_sat_verifier(proof, pp, c.sc, c.gf, vm.PivotChoice.koe) == ALL_TRUE
    # and a proof made under one pp fails the pivot under another
    got = cs.circuit_sat_verifier(proof, c.pp, c.sc, c.gf, "koe")
    assert got["L_wellformed_from_Cfgh_forms"] is True and got["pivot_verification"]["restriction_arg_check"] is False
