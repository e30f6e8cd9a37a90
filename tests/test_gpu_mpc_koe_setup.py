"""The jointly made pp of the knowledge-of-exponent pivot: knowledge_of_exponent.update_setup, one
party's pass over a pp through vmpc_bn256_scale_points_dev, and mpc_koe.koe_trusted_setup, M passes in M exchanges.

The defining identity is checked on bytes: a pass under (a', b', c') over trusted_setup's pp under (a, b, c) IS
trusted_setup's pp under (a a', b b', c c').  A few points of every pp are also compared with the trapdoor's exponents
times the generators on Python ints (oracle/bn256_ref.py, tests/mpc_koe_ref.py), independently of every kernel."""
import asyncio
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import mpc_koe_ref as mref
from tests import p8_field_ref as fref

pytestmark = pytest.mark.gpu
N = fref.BN_N
F = fref.P8(N)


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
    from verifiable_mpc_amd import circuit_sat_gpu, knowledge_of_exponent, mpc_ac20, mpc_koe
    return SimpleNamespace(cs=circuit_sat_gpu, koe=knowledge_of_exponent, mpc_ac20=mpc_ac20, mk=mpc_koe)


def generators(vm):
    return vm.pynocchio.BN256Point(bn.G1), vm.pynocchio.BN256TwistPoint(bn.G2)


def groups(vm):
    g1, g2 = generators(vm)
    return [SimpleNamespace(generator=g1), SimpleNamespace(generator=g2)]


def setup_under(vm, koe, monkeypatch, n, trapdoor):
    monkeypatch.setattr(koe, "prng", Replay(trapdoor))
    pp = koe.trusted_setup(*generators(vm), n, N)
    assert koe.prng.draws == []
    return pp


def pp_bytes(pp):
    return pp["pp_lhs"].rows().tobytes(), pp["pp_rhs"].rows().tobytes()


def check_points(pp, trap, at):
    """elements `at` of both sides against the trapdoor's exponents times the generators"""
    lhs, rhs = pp["pp_lhs"].rows(), pp["pp_rhs"].rows()
    for i in at:
        assert lhs[i].tobytes() == bn.g1_to_bytes(bn.E1.mul(trap.lhs_exp(i), bn.G1)), i
        assert rhs[i].tobytes() == bn.g2_to_bytes(bn.E2.mul(trap.rhs_exp(i), bn.G2)), i


def draws(seed, count):
    rng = random.Random(seed)
    return [tuple(rng.randrange(1, N) for _ in range(3)) for _ in range(count)]


class Parties:
    """M mpc_koe runtimes in one process on one hub that counts every party's exchanges"""

    def __init__(self, mods, M, t, seed=1):
        calls = self.calls = [0] * M

        class CountingHub(mods.mpc_ac20.LocalHub):
            async def exchange(self, pid, tag, value):
                calls[pid] += 1
                return await super().exchange(pid, tag, value)
        self.M, self.hub = M, CountingHub(M)
        self.rts = [mods.mk.Runtime(p, M, t, random.Random(seed * 100 + p), self.hub) for p in range(M)]

    def run(self, fn, return_exceptions=False):
        async def everybody():
            return await asyncio.gather(*[fn(p, rt) for p, rt in enumerate(self.rts)], return_exceptions=return_exceptions)
        loop = asyncio.new_event_loop()
        try:
            return loop.run_until_complete(everybody())
        finally:
            loop.close()


def _three(rng):
    return tuple(rng.randrange(1, N) for _ in range(3))


# ---- update_setup ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 33, 129])
def test_a_pass_over_a_pp_is_the_pp_under_the_product_trapdoor(vm, mods, monkeypatch, n):
    first, second = draws(60 + n, 2)
    pp = setup_under(vm, mods.koe, monkeypatch, n, first)
    passed = mods.koe.update_setup(pp, *second)
    assert len(passed["pp_lhs"]) == len(passed["pp_rhs"]) == 2 * n
    product = tuple(a * b % N for a, b in zip(first, second))
    assert pp_bytes(passed) == pp_bytes(setup_under(vm, mods.koe, monkeypatch, n, product))
    trap = mref.joint_trapdoor([first, second])
    assert (trap.g_exp, trap.alpha, trap.s) == product
    check_points(passed, trap, [0, 1, 2 * n - 1])
    assert pp_bytes(pp) != pp_bytes(passed)                            # the input is left as it was
    check_points(pp, mref.joint_trapdoor([first]), [0, 2 * n - 1])


def test_a_pass_takes_lists_and_validates_them(vm, mods, monkeypatch):
    first, second = draws(71, 2)
    pp = setup_under(vm, mods.koe, monkeypatch, 5, first)
    as_lists = {"pp_lhs": list(pp["pp_lhs"]), "pp_rhs": list(pp["pp_rhs"])}
    assert pp_bytes(mods.koe.update_setup(as_lists, *second)) == pp_bytes(mods.koe.update_setup(pp, *second))
    x, y = bn.E1.mul(5, bn.G1)
    off_g1 = vm.pynocchio.BN256Point((x, (y + 1) % bn.P))
    with pytest.raises(ValueError, match="pp_lhs"):
        mods.koe.update_setup({"pp_lhs": as_lists["pp_lhs"][:3] + [off_g1], "pp_rhs": as_lists["pp_rhs"]}, *second)
    (x0, x1), (y0, y1) = bn.E2.mul(5, bn.G2)
    off_g2 = vm.pynocchio.BN256TwistPoint(((x0, x1), ((y0 + 1) % bn.P, y1)))
    with pytest.raises(ValueError, match="pp_rhs"):
        mods.koe.update_setup({"pp_lhs": as_lists["pp_lhs"], "pp_rhs": [off_g2] + as_lists["pp_rhs"][1:]}, *second)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_zero_factor_is_refused(vm, mods, monkeypatch, which):
    pp = setup_under(vm, mods.koe, monkeypatch, 5, draws(72, 1)[0])
    for zero in (0, N):
        factors = [3, 5, 7]
        factors[which] = zero
        with pytest.raises(ValueError, match=("g_exp", "alpha", "z")[which]):
            mods.koe.update_setup(pp, *factors)


# ---- koe_trusted_setup -----------------------------------------------------------------------------------------------------
def test_one_party_is_trusted_setup_under_its_draws(vm, mods, monkeypatch):
    ps = Parties(mods, 1, 0)
    pps = ps.run(lambda p, rt: mods.mk.koe_trusted_setup(groups(vm), None, 7, rt=rt))
    assert ps.calls == [1] and ps.rts[0].exchanges == 1
    mine = _three(random.Random(100))
    assert pp_bytes(pps[0]) == pp_bytes(setup_under(vm, mods.koe, monkeypatch, 7, mine))
    assert isinstance(pps[0]["pp_lhs"], mods.koe.PPVector) and len(pps[0]["pp_rhs"]) == 14


@pytest.fixture(scope="module")
def joint(vm, mods):
    """the M = 3 setup for vectors of 14 scalars, made once: (parties, every party's pp, every party's draws)"""
    ps = Parties(mods, 3, 1, seed=4)
    pps = ps.run(lambda p, rt: mods.mk.koe_trusted_setup(groups(vm), None, 14, rt=rt))
    return ps, pps, [_three(random.Random(400 + p)) for p in range(3)]


def test_three_parties_make_the_pp_of_the_product_trapdoor(vm, mods, monkeypatch, joint):
    ps, pps, all_draws = joint
    assert ps.calls == [3, 3, 3] and [rt.exchanges for rt in ps.rts] == [3, 3, 3]
    assert pp_bytes(pps[1]) == pp_bytes(pps[0]) and pp_bytes(pps[2]) == pp_bytes(pps[0])      # every party the same bytes
    trap = mref.joint_trapdoor(all_draws)
    assert pp_bytes(pps[0]) == pp_bytes(setup_under(vm, mods.koe, monkeypatch, 14, (trap.g_exp, trap.alpha, trap.s)))
    check_points(pps[0], trap, [0, 27])
    assert all(isinstance(pp[k], mods.koe.PPVector) and len(pp[k]) == 28 for pp in pps for k in ("pp_lhs", "pp_rhs"))


def test_a_single_prover_proves_under_the_joint_pp(vm, mods, joint):
    """N = 5 + 3 + 2 * 3 = 14: circuit_sat_prover / circuit_sat_verifier as they are, under a pp nobody has the trapdoor of"""
    _, pps, _ = joint
    rng = random.Random(103)
    A, B, O = F.random_circuit(rng, 5, 3, 2)
    x = [rng.randrange(N) for _ in range(5)]
    sc = mods.cs.SparseCircuit(5, fref.to_csr(A), fref.to_csr(B), fref.to_csr(O), order=N)
    gf = vm.GF(N)
    proof = mods.cs.circuit_sat_prover(pps[0], sc, x, gf, vm.PivotChoice.koe)
    assert mods.cs.circuit_sat_verifier(proof, pps[2], sc, gf, vm.PivotChoice.koe) == {
        "y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True,
        "pivot_verification": {"restriction_arg_check": True, "PRQ_check": True}}


@pytest.mark.parametrize("what", ["lhs off the curve", "rhs off the curve", "lhs at infinity", "rhs at infinity", "short"])
def test_a_bad_contribution_is_refused_by_every_party(vm, mods, monkeypatch, what):
    """party 0's pp is altered on its way out: the receivers - party 0 itself included - refuse it with ValueError"""
    real = mods.koe.setup_under

    def tampered(*args):
        pp = real(*args)
        side = "pp_lhs" if "lhs" in what else "pp_rhs"
        rows = pp[side].rows().copy()
        if "curve" in what:
            rows[2, 0] ^= 1                                           # x of element 2: no longer on the curve
        elif "infinity" in what:
            rows[3] = 0
        else:
            rows = rows[:-1]
        pp[side] = SimpleNamespace(rows=lambda: rows)
        return pp
    monkeypatch.setattr(mods.koe, "setup_under", tampered)
    ps = Parties(mods, 3, 1, seed=5)
    res = ps.run(lambda p, rt: mods.mk.koe_trusted_setup(groups(vm), None, 5, rt=rt), True)
    assert len(res) == 3 and all(isinstance(r, ValueError) and "koe_trusted_setup" in str(r) for r in res), res
    assert ps.calls == [1, 1, 1]                                      # refused after the first exchange, nothing passed on
