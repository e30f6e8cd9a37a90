"""Every BN-256 entry point that takes points from outside, fed a malformed encoding in each point operand in turn.
The compute kernels do not validate (include/vmpc.h); each entry below relies on vmpc_bn256_validate_dev in front of
them, and a gate that lets one of these through is a soundness or malleability gap, not a wrong number.

Three malformed kinds, from tests/bn256_encodings.py (Q is that module's valid point):
    off        Q with the low bit of its LAST residue flipped (y, and y.im on the twist): canonical, off the curve
    alias      Q with r + P in its last residue: other bytes for the point Q
    inf-alias  P in every residue: other bytes for the point at infinity, and NOT the all-zero bytes
The points are built with from_bytes or as byte arrays; the constructors reduce mod P and would hide two of the kinds.
What each gate is held to is what its docstring and include/vmpc.h promise: the exception type, the error code, the
named element or proof index; the byte-level entries must leave the output buffer as it was.  Every case is paired with
the same call with Q in that operand, which must go through, so that a gate refusing everything does not pass.

Gates: the host one-shots vmpc_bn256_g1_msm / g2_msm and vmpc_bn256_lincomb_batch; pynocchio.msm, pairing,
pairing_product, verify (each proof element, each verification-key element the verifier reads), verify_batch,
PreparedKey (from a dict and from a device array), compute_proof over a dict; knowledge_of_exponent's pp from lists,
trusted_setup's bases and the two verifiers' proof points; trinocchio.recombine_points; mpc_koe.koe_trusted_setup.

NOT covered: subgroup membership of twist points (the twist's cofactor is not 1; neither the reference nor these gates
check it).

30 tests; with tests/test_gpu_bn256_validate.py 54 tests in 6 s on an MI355X, most of it context and fixture setup.  No
gate let anything through.  Each of these value-only mutations makes tests of this file fail (the numbering is that of
tests/test_gpu_bn256_validate.py, which lists its own):
  1. Fp29x2Ops::raw_canonical looks at its first residue only (14 tests): the twist case of test_host_msm_one_shots,
     test_host_lincomb_one_shot, test_msm and test_key_vector_from_a_device_array; test_pairing_and_pairing_product,
     test_prepared_key_and_dict_key, test_koe_trusted_setup_bases, test_recombine_points; the kind "alias" of
     test_verify_names_the_malformed_proof_element, .._key_element, test_verify_batch_names_the_proof,
     test_koe_pp_from_lists, test_koe_verifiers_proof_points and test_joint_setup_..[alias-pp_rhs].
  2. gk_validate asks raw_canonical of x only (19 tests): those of 1. in both groups, with
     test_joint_setup_..[alias-pp_lhs].
  3. gk_validate stores 1 in place of its atomicAdd: none (every gate asks only whether the count is zero).
  4. fp_raw_is_canonical answers true on equality: none (P in every residue is also off the curve).
  5. BN256Point.from_bytes reduces mod P (16 tests): every test that builds an "alias" or "inf-alias" point object -
     test_msm, test_pairing_and_pairing_product, the three verify tests, test_prepared_key_and_dict_key,
     test_koe_pp_from_lists, test_koe_trusted_setup_bases, test_koe_verifiers_proof_points, test_recombine_points.
  6. mpc_koe._received_side without its bn256_validate call: the six malformed cases of
     test_joint_setup_refuses_a_malformed_contribution."""
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import bn256_encodings as enc
from tests.conftest import load_golden
from tests.test_gpu_bn256_pairing import instance
from tests.test_gpu_mpc_koe_setup import Parties, Replay, groups

pytestmark = pytest.mark.gpu
N = bn.N
KINDS = list(enc.KINDS)
FILL = 0xA5


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def pn(vm):
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def nat(vm):
    from verifiable_mpc_amd import _native
    return _native


@pytest.fixture(scope="module")
def mods(vm):
    from verifiable_mpc_amd import circuit_sat_gpu, knowledge_of_exponent, mpc_ac20, mpc_koe, trinocchio
    return SimpleNamespace(cs=circuit_sat_gpu, koe=knowledge_of_exponent, mpc_ac20=mpc_ac20, mk=mpc_koe, tn=trinocchio)


@pytest.fixture(scope="module")
def fx():
    return load_golden("bn256_pairing.json")


def cls_of(pn, group):
    return pn.BN256Point if group == 1 else pn.BN256TwistPoint


def bad_point(pn, group, kind):
    """the malformed point as an object whose to_bytes() is the malformed encoding, bit for bit"""
    raw = enc.malformed_bytes(group, kind)
    pt = cls_of(pn, group).from_bytes(raw)
    assert pt.to_bytes() == raw and pt.coords == enc.malformed(group, kind)
    return pt


def q_point(pn, group):
    pt = cls_of(pn, group).from_bytes(enc.q_bytes(group))
    assert pt.coords == enc.q_residues(group)
    return pt


def multiples(group, ks):
    E, G = enc.CURVES[group]
    return [E.mul(k, G) for k in ks]


def to_bytes(group, pt):
    return enc.encode(enc.flat(group, pt))


def rows_array(group, raws):
    return np.frombuffer(b"".join(raws), np.uint8).reshape(len(raws), enc.WIDTH[group]).copy()


def small_scalars(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


# ---- the host one-shots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_host_msm_one_shots(nat, group):
    """vmpc_bn256_g1_msm / g2_msm: the bad point first, in the middle and last of 5 -> VMPC_E_NOTONCURVE, out untouched"""
    lib = nat.load_library()
    fn = lib.vmpc_bn256_g1_msm if group == 1 else lib.vmpc_bn256_g2_msm
    E, G = enc.CURVES[group]
    width = enc.WIDTH[group]
    pts, ks = multiples(group, [3, 5, 7, 11, 13]), [2, 3, 4, 5, 6]
    sc = small_scalars(ks)
    _, q = enc.valid_point(group)
    for pos in (0, 2, 4):
        raws = [to_bytes(group, p) for p in pts]
        raws[pos] = enc.q_bytes(group)
        out, d_pts = np.full(width, FILL, np.uint8), rows_array(group, raws)
        assert fn(nat._np_ptr(sc), nat._np_ptr(d_pts), 5, nat._np_ptr(out)) == 0, pos
        want = E.msm(ks, pts[:pos] + [q] + pts[pos + 1:])
        assert out.tobytes() == to_bytes(group, want), pos
        for kind in KINDS:
            raws[pos] = enc.malformed_bytes(group, kind)
            out, d_pts = np.full(width, FILL, np.uint8), rows_array(group, raws)
            rc = fn(nat._np_ptr(sc), nat._np_ptr(d_pts), 5, nat._np_ptr(out))
            assert rc == nat.E_NOTONCURVE, (pos, kind, rc)
            assert (out == FILL).all(), (pos, kind)


@pytest.mark.parametrize("group", [1, 2])
def test_host_lincomb_one_shot(nat, group):
    """vmpc_bn256_lincomb_batch over a batch of 65: a bad base (the last of three) and a bad row point (lane 64)"""
    lib = nat.load_library()
    E, G = enc.CURVES[group]
    width, batch = enc.WIDTH[group], 65
    _, q = enc.valid_point(group)
    b0, b1 = multiples(group, [3, 5])
    row = E.mul(7, G)
    sc = small_scalars([v for b in range(batch) for v in (b + 1, 2, 3)])

    def call(bases, rows):
        out = np.full(batch * width, FILL, np.uint8)
        d_bases, d_rows = rows_array(group, bases), rows_array(group, rows)      # named: alive across the call
        rc = lib.vmpc_bn256_lincomb_batch(group, nat._np_ptr(d_bases), 3, nat._np_ptr(sc), nat._np_ptr(d_rows), 1, batch,
                                          0, nat._np_ptr(out))
        return rc, out

    good_bases = [to_bytes(group, b0), to_bytes(group, b1), enc.q_bytes(group)]
    good_rows = [to_bytes(group, row)] * 64 + [enc.q_bytes(group)]
    rc, out = call(good_bases, good_rows)
    assert rc == 0
    for b, r in ((0, row), (63, row), (64, q)):
        want = E.add(E.msm([b + 1, 2, 3], [b0, b1, q]), r)
        assert out[width * b:width * (b + 1)].tobytes() == to_bytes(group, want), b
    for kind in KINDS:
        bad = enc.malformed_bytes(group, kind)
        rc, out = call(good_bases[:2] + [bad], good_rows)
        assert rc == nat.E_NOTONCURVE and (out == FILL).all(), ("base", kind, rc)
        rc, out = call(good_bases, good_rows[:64] + [bad])
        assert rc == nat.E_NOTONCURVE and (out == FILL).all(), ("row point", kind, rc)


# ---- pynocchio.msm, pairing, pairing_product -----------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_msm(pn, nat, group):
    E, G = enc.CURVES[group]
    cls = cls_of(pn, group)
    pts, ks = multiples(group, [3, 5, 7, 11]), [9, 8, 7, 6, 5]
    _, q = enc.valid_point(group)
    objs = [cls.from_bytes(to_bytes(group, p)) for p in pts]
    got = pn.msm(ks, objs[:2] + [q_point(pn, group)] + objs[2:])
    assert got.to_bytes() == to_bytes(group, E.msm(ks, pts[:2] + [q] + pts[2:]))
    for kind in KINDS:
        with pytest.raises(nat.VmpcError) as e:
            pn.msm(ks, objs[:2] + [bad_point(pn, group, kind)] + objs[2:])
        assert e.value.code == nat.E_NOTONCURVE and "pynocchio.msm" in str(e.value), kind


def test_pairing_and_pairing_product(pn):
    q1, q2 = q_point(pn, 1), q_point(pn, 2)
    _, o1 = enc.valid_point(1)
    neg_q1 = pn.BN256Point.from_bytes(to_bytes(1, bn.E1.neg(o1)))
    g1s = [pn.BN256Point(p) for p in multiples(1, [3, 5])]
    g2s = [pn.BN256TwistPoint(enc.flat(2, p)) for p in multiples(2, [3, 5])]
    assert not pn.pairing(q1, q2).is_one()
    # the second product, pairs 2 and 3: e(Q1, Q2) e(-Q1, Q2) == 1
    gts, ones = pn.pairing_product(g1s + [q1, neg_q1], g2s + [q2, q2], [0, 2, 4])
    assert ones == [False, True] and gts[1].is_one()
    for kind in KINDS:
        b1, b2 = bad_point(pn, 1, kind), bad_point(pn, 2, kind)
        with pytest.raises(ValueError, match="pairing: first argument"):
            pn.pairing(b1, q2)
        with pytest.raises(ValueError, match="pairing: second argument"):
            pn.pairing(q1, b2)
        with pytest.raises(ValueError, match="pairing_product: G1 points"):
            pn.pairing_product(g1s + [q1, b1], g2s + [q2, q2], [0, 2, 4])
        with pytest.raises(ValueError, match="pairing_product: twist points"):
            pn.pairing_product(g1s + [q1, neg_q1], g2s + [b2, q2], [0, 2, 4])


# ---- pynocchio.verify / verify_batch ---------------------------------------------------------------------------------------
def verikey_names(Q):
    io = list(Q.indices_io)
    return (["r_v*v0*g1"] + [f"r_v*v{i}*g1" for i in io] + ["r_w*w0*g2"] + [f"r_w*w{i}*g2" for i in io] +
            [f"r_y*y{i}*g1" for i in io] + ["alpha_w*g1", "beta*gamma*g1", "g2", "r_y*t*g2", "alpha_v*g2", "alpha_y*g2",
                                           "gamma*g2", "beta*gamma*g2"])


def group_of(name):
    return 2 if name.endswith("g2") else 1


def test_verify_with_q_in_each_operand_goes_through(pn, fx):
    """the control of the two tests below: a VALID foreign point in any operand is no error - the checks just fail"""
    Q, verikey, _, proof, c = instance(pn, fx)
    assert all(pn.verify(Q, verikey, proof, c).values())
    for name in proof:
        res = pn.verify(Q, verikey, dict(proof, **{name: q_point(pn, group_of(name))}), c)
        assert set(res) == {"H", "V", "W", "Y", "Z"} and not all(res.values()), name
    for name in verikey_names(Q):
        res = pn.verify(Q, dict(verikey, **{name: q_point(pn, group_of(name))}), proof, c)
        assert set(res) == {"H", "V", "W", "Y", "Z"}, name


@pytest.mark.parametrize("kind", KINDS)
def test_verify_names_the_malformed_proof_element(pn, fx, kind):
    Q, verikey, _, proof, c = instance(pn, fx)
    assert len(proof) == 8
    for name in proof:
        bad = dict(proof, **{name: bad_point(pn, group_of(name), kind)})
        with pytest.raises(ValueError, match="proof 0: " + re.escape(repr(name))):
            pn.verify(Q, verikey, bad, c)


@pytest.mark.parametrize("kind", KINDS)
def test_verify_names_the_malformed_key_element(pn, fx, kind):
    Q, verikey, _, proof, c = instance(pn, fx)
    names = verikey_names(Q)
    assert set(names) <= set(verikey) and len(names) == 16
    for name in names:
        bad = dict(verikey, **{name: bad_point(pn, group_of(name), kind)})
        with pytest.raises(ValueError, match=re.escape(f"verikey[{name!r}]")):
            pn.verify(Q, bad, proof, c)


@pytest.mark.parametrize("kind", KINDS)
def test_verify_batch_names_the_proof(pn, fx, kind):
    Q, verikey, _, proof, c = instance(pn, fx)
    for name in ("h*g1", "r_w*w_mid*g2"):
        bad = dict(proof, **{name: bad_point(pn, group_of(name), kind)})
        ok = dict(proof, **{name: q_point(pn, group_of(name))})
        for at in (0, 2, 4):
            proofs = [proof] * 5
            proofs[at] = ok
            res = pn.verify_batch(Q, verikey, proofs, [c] * 5)
            assert [all(r.values()) for r in res] == [j != at for j in range(5)]
            proofs[at] = bad
            with pytest.raises(ValueError, match=f"proof {at}: " + re.escape(repr(name))):
                pn.verify_batch(Q, verikey, proofs, [c] * 5)
    # two malformed proofs: the first is named
    proofs = [proof, dict(proof, **{"h*g1": bad_point(pn, 1, kind)}), proof, dict(proof, **{"h*g1": bad_point(pn, 1, kind)}),
              proof]
    with pytest.raises(ValueError, match="proof 1: "):
        pn.verify_batch(Q, verikey, proofs, [c] * 5)


# ---- the prover's keys -------------------------------------------------------------------------------------------------------
def _h_and_deltas(fx):
    case = fx["pinocchio"]

    class H:
        coeffs = [int(v, 16) for v in case["h"]]

        def __len__(self):
            return len(self.coeffs)

    class D:
        v, w, y = (int(x, 16) for x in case["deltas"])
    return H(), D


KEY_ELEMENTS = ["r_v*alpha_v*v5*g1", "r_w*w5*g2", "s^3*g1", "r_y*beta*t*g1"]


def test_prepared_key_and_dict_key(pn, nat, fx):
    Q, verikey, evalkey, proof, c = instance(pn, fx)
    h, D = _h_and_deltas(fx)
    assert set(KEY_ELEMENTS) <= set(evalkey)
    for name in KEY_ELEMENTS:
        ok = dict(evalkey, **{name: q_point(pn, group_of(name))})
        assert set(pn.compute_proof(Q, c, h, ok, D)) == set(proof), name
        assert set(pn.compute_proof(Q, c, h, pn.PreparedKey(Q, ok), D)) == set(proof), name
        for kind in KINDS:
            bad = dict(evalkey, **{name: bad_point(pn, group_of(name), kind)})
            with pytest.raises(nat.VmpcError) as e:
                pn.PreparedKey(Q, bad)
            assert e.value.code == nat.E_NOTONCURVE and "pynocchio.PreparedKey" in str(e.value), (name, kind)
            with pytest.raises(nat.VmpcError) as e:
                pn.compute_proof(Q, c, h, bad, D)
            assert e.value.code == nat.E_NOTONCURVE and "pynocchio.msm" in str(e.value), (name, kind)


@pytest.mark.parametrize("group", [1, 2])
def test_key_vector_from_a_device_array(vm, pn, nat, group):
    """the array path of a prepared key (PreparedKey.synthetic / generate hand device arrays to _KeyVector.from_device)"""
    ctx = vm.get_context()
    raws = [to_bytes(group, p) for p in multiples(group, [3, 5, 7, 11, 13, 17, 19, 23, 29])]
    raws[6] = enc.q_bytes(group)
    vec = pn._KeyVector.from_device(ctx, group, ctx.upload(rows_array(group, raws)), len(raws))
    assert vec.n == len(raws) and vec.group == group
    for kind in KINDS:
        raws[6] = enc.malformed_bytes(group, kind)
        with pytest.raises(nat.VmpcError) as e:
            pn._KeyVector.from_device(ctx, group, ctx.upload(rows_array(group, raws)), len(raws))
        assert e.value.code == nat.E_NOTONCURVE, kind


# ---- knowledge_of_exponent ------------------------------------------------------------------------------------------------------
KOE_N = 3


@pytest.fixture()
def koe_case(vm, pn, mods, monkeypatch):
    """a pp for vectors of 3 scalars under a known trapdoor, as PPVectors and as lists, and an opening that verifies"""
    koe = mods.koe
    rng = random.Random(77)
    trapdoor = [rng.randrange(1, N) for _ in range(3)]
    monkeypatch.setattr(koe, "prng", Replay(trapdoor))
    pp = koe.trusted_setup(pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2), KOE_N, N)
    lists = {"pp_lhs": list(pp["pp_lhs"]), "pp_rhs": list(pp["pp_rhs"])}
    L = vm.pivot.LinearForm([rng.randrange(N) for _ in range(KOE_N)])
    x, gamma = [rng.randrange(N) for _ in range(KOE_N)], rng.randrange(N)
    proof, u = koe.opening_linear_form_prover(L, x, gamma, pp)
    ok = {"restriction_arg_check": True, "PRQ_check": True}
    assert koe.opening_linear_form_verifier(L, pp, proof, u) == ok == koe.opening_linear_form_verifier(L, lists, proof, u)
    return SimpleNamespace(koe=koe, pp=pp, lists=lists, L=L, x=x, gamma=gamma, proof=proof, u=u, trapdoor=trapdoor)


def with_point(lists, side, at, pt):
    out = {k: list(v) for k, v in lists.items()}
    out[side][at] = pt
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_koe_pp_from_lists(pn, koe_case, kind):
    """a pp that arrives as lists is validated wherever it is taken: ValueError naming the side"""
    k, koe = koe_case, koe_case.koe
    for side, group in (("pp_lhs", 1), ("pp_rhs", 2)):
        bad, ok = bad_point(pn, group, kind), q_point(pn, group)
        # update_setup reads every point: the last one
        assert len(koe.update_setup(with_point(k.lists, side, 2 * KOE_N - 1, ok), 3, 5, 7)[side]) == 2 * KOE_N
        with pytest.raises(ValueError, match=side):
            koe.update_setup(with_point(k.lists, side, 2 * KOE_N - 1, bad), 3, 5, 7)
        # the prover's commitment reads points 0 .. n
        P, pi = koe.restriction_argument_prover(range(KOE_N), k.x, k.gamma, with_point(k.lists, side, KOE_N, ok))
        assert P.coords is not None and pi.coords is not None
        with pytest.raises(ValueError, match=side):
            koe.restriction_argument_prover(range(KOE_N), k.x, k.gamma, with_point(k.lists, side, KOE_N, bad))
        # the verifiers read point 0 of either side
        assert koe.restriction_argument_verifier(k.proof["P"], k.proof["pi"], with_point(k.lists, side, 0, ok)) is False
        with pytest.raises(ValueError, match=side):
            koe.restriction_argument_verifier(k.proof["P"], k.proof["pi"], with_point(k.lists, side, 0, bad))
        with pytest.raises(ValueError, match=side):
            koe.opening_linear_form_verifier(k.L, with_point(k.lists, side, 0, bad), k.proof, k.u)
    # .. and the opening's verifier points 0 .. n of pp_rhs
    res = koe.opening_linear_form_verifier(k.L, with_point(k.lists, "pp_rhs", KOE_N, q_point(pn, 2)), k.proof, k.u)
    assert res == {"restriction_arg_check": True, "PRQ_check": False}
    with pytest.raises(ValueError, match="pp_rhs"):
        koe.opening_linear_form_verifier(k.L, with_point(k.lists, "pp_rhs", KOE_N, bad_point(pn, 2, kind)), k.proof, k.u)


def test_koe_trusted_setup_bases(pn, mods, monkeypatch):
    koe = mods.koe
    g1, g2 = pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2)
    g_exp, alpha, z = 11, 13, 17
    monkeypatch.setattr(koe, "prng", Replay([g_exp, alpha, z]))
    pp = koe.trusted_setup(q_point(pn, 1), q_point(pn, 2), KOE_N, N)
    k1, k2 = enc.valid_point(1)[0], enc.valid_point(2)[0]
    assert pp["pp_lhs"][0].to_bytes() == to_bytes(1, bn.E1.mul(k1 * g_exp * z, bn.G1))
    assert pp["pp_rhs"][1].to_bytes() == to_bytes(2, bn.E2.mul(k2 * g_exp * alpha * z * z, bn.G2))
    for kind in KINDS:
        monkeypatch.setattr(koe, "prng", Replay([g_exp, alpha, z]))
        with pytest.raises(ValueError, match="trusted_setup: generator 1"):
            koe.trusted_setup(bad_point(pn, 1, kind), g2, KOE_N, N)
        monkeypatch.setattr(koe, "prng", Replay([g_exp, alpha, z]))
        with pytest.raises(ValueError, match="trusted_setup: generator 2"):
            koe.trusted_setup(g1, bad_point(pn, 2, kind), KOE_N, N)


@pytest.mark.parametrize("kind", KINDS)
def test_koe_verifiers_proof_points(pn, koe_case, kind):
    """P, pi and Q: the module promises ValueError for a point not on its curve, not a False check"""
    k, koe = koe_case, koe_case.koe
    b1, b2, q1, q2 = bad_point(pn, 1, kind), bad_point(pn, 2, kind), q_point(pn, 1), q_point(pn, 2)
    assert koe.restriction_argument_verifier(k.proof["P"], k.proof["pi"], k.pp) is True
    assert koe.restriction_argument_verifier(q1, k.proof["pi"], k.pp) is False
    assert koe.restriction_argument_verifier(k.proof["P"], q2, k.pp) is False
    with pytest.raises(ValueError, match="^P is not on the BN-256 curve"):
        koe.restriction_argument_verifier(b1, k.proof["pi"], k.pp)
    with pytest.raises(ValueError, match="^pi is not on the BN-256 twist"):
        koe.restriction_argument_verifier(k.proof["P"], b2, k.pp)
    for name, bad, ok, curve in (("P", b1, q1, "curve"), ("pi", b2, q2, "twist"), ("Q", b1, q1, "curve")):
        res = koe.opening_linear_form_verifier(k.L, k.pp, dict(k.proof, **{name: ok}), k.u)
        assert set(res) == {"restriction_arg_check", "PRQ_check"} and not all(res.values()), name
        with pytest.raises(ValueError, match=f"^{name} is not on the BN-256 {curve}"):
            koe.opening_linear_form_verifier(k.L, k.pp, dict(k.proof, **{name: bad}), k.u)


# ---- trinocchio.recombine_points ---------------------------------------------------------------------------------------------------
def test_recombine_points(vm, pn, nat, mods):
    tn = mods.tn
    ctx = vm.get_context()
    rt = tn.Runtime(0, 3, 1, random.Random(1), tn.LocalHub(3), ctx=ctx)
    g1, g2 = pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2)
    q1, q2 = q_point(pn, 1), q_point(pn, 2)
    assert rt.recombine_points([[q1, g2, q2]] * 3, ctx) == [q1, g2, q2]                  # the weights sum to 1
    w = rt.weights
    got = rt.recombine_points([[g1, g2], [q1, g2], [g1, q2]], ctx)
    k1, k2 = enc.valid_point(1)[0], enc.valid_point(2)[0]
    assert got[0].to_bytes() == to_bytes(1, bn.E1.mul((w[0] + w[1] * k1 + w[2]) % N, bn.G1))
    assert got[1].to_bytes() == to_bytes(2, bn.E2.mul((w[0] + w[1] + w[2] * k2) % N, bn.G2))
    for kind in KINDS:
        for every in ([[g1, g2], [bad_point(pn, 1, kind), g2], [g1, g2]],
                      [[g1, g2], [g1, g2], [g1, bad_point(pn, 2, kind)]]):
            with pytest.raises(nat.VmpcError) as e:
                rt.recombine_points(every, ctx)
            assert e.value.code == nat.E_NOTONCURVE and "trinocchio.recombine_points" in str(e.value), kind


# ---- mpc_koe.koe_trusted_setup --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["pp_lhs", "pp_rhs"])
@pytest.mark.parametrize("kind", KINDS + ["Q"])
def test_joint_setup_refuses_a_malformed_contribution(vm, mods, monkeypatch, kind, side):
    """party 0's pp has one point replaced on its way out.  Every receiver - party 0 itself included - refuses the three
    malformed kinds, after the first exchange; "inf-alias" is the point of this case: the side has no all-zero point,
    so the search for the point at infinity passes it, and the curve gate must not.  With Q there (a point of the
    curve, if not of the pp) the setup goes through: this check does not refuse everything."""
    real = mods.koe.setup_under
    group = 1 if side == "pp_lhs" else 2
    raw = enc.q_bytes(group) if kind == "Q" else enc.malformed_bytes(group, kind)

    def tampered(*args):
        pp = real(*args)
        rows = pp[side].rows().copy()
        rows[2] = np.frombuffer(raw, np.uint8)
        assert rows.any(axis=1).all()
        pp[side] = SimpleNamespace(rows=lambda: rows)
        return pp
    monkeypatch.setattr(mods.koe, "setup_under", tampered)
    ps = Parties(mods, 3, 1, seed=6)
    res = ps.run(lambda p, rt: mods.mk.koe_trusted_setup(groups(vm), None, 5, rt=rt), True)
    assert len(res) == 3
    if kind == "Q":
        assert all(isinstance(r, dict) and len(r[side]) == 10 for r in res), res
        assert ps.calls == [3, 3, 3]
        return
    curve = "BN-256 curve" if group == 1 else "BN-256 twist"
    want = f"koe_trusted_setup: {side} as received holds a point not on the {curve}"
    assert all(isinstance(r, ValueError) and str(r) == want for r in res), res
    assert ps.calls == [1, 1, 1]                                      # refused after the first exchange, nothing passed on
