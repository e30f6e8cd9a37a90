"""GPU tests of the knowledge-of-exponent pivot over BN-256 (verifiable_mpc_amd/knowledge_of_exponent.py,
csrc/bn256_koe.hip over csrc/fr_bn.h): the polynomial product and the powers kernel against Python integers (exactly),
parity with the reference-made fixture (tests/golden/koe_bn256.json), the prover against the setup's trapdoor at
n = 2^10, 2^13 and 2^16 (oracle/bn256_ref.py, independent of the kernels), and the soundness of the verifier."""
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N = bn.N
TOP = (1 << 256) - 1
h2i = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def koe(vm):
    return vm.knowledge_of_exponent


@pytest.fixture(scope="module")
def fx():
    return load_golden("koe_bn256.json")


def to_arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)


def to_ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def poly_mul(koe, a, b):
    return to_ints(koe.fr_poly_mul(to_arr(a), to_arr(b)))


def coeff(a, b, k):
    return sum(a[i] * b[k - i] for i in range(max(0, k - len(b) + 1), min(len(a) - 1, k) + 1)) % N


def horner(c, r):
    acc = 0
    for v in reversed(c):
        acc = (acc * r + v) % N
    return acc


# ---- fr_poly_mul ----------------------------------------------------------------------------------------------------

def test_poly_mul_small_shapes_exact(koe):
    rng = random.Random(1)
    for na in range(1, 66):
        for nb in (1, 2, 63, 64, 65):
            a = [rng.randrange(N) for _ in range(na)]
            b = [rng.randrange(N) for _ in range(nb)]
            assert poly_mul(koe, a, b) == [coeff(a, b, k) for k in range(na + nb - 1)], (na, nb)


@pytest.mark.parametrize("log_n", [12, 14, 16])
def test_poly_mul_large_by_evaluation(koe, log_n):
    """a(r) b(r) == c(r) mod n at three random r: exact, a wrong product passes with probability ~ 2^17 / 2^256"""
    n = 1 << log_n
    rng = random.Random(log_n)
    a = [rng.randrange(N) for _ in range(n)]
    b = [rng.randrange(N) for _ in range(n)]
    c = poly_mul(koe, a, b)
    assert len(c) == 2 * n - 1 and all(v < N for v in c)
    for _ in range(3):
        r = rng.randrange(N)
        assert horner(a, r) * horner(b, r) % N == horner(c, r)
    for k in [0, 1, n - 1, n, 2 * n - 2] + [rng.randrange(2 * n - 1) for _ in range(16)]:
        assert c[k] == coeff(a, b, k), k


def test_poly_mul_worst_case_carries(koe):
    """(n-1)^2 = 1 mod n: 2^16 products of the largest residues overflow an accumulator that is one limb short"""
    n = 1 << 16
    c = poly_mul(koe, [N - 1] * n, [N - 1] * n)
    assert c == [min(k, 2 * n - 2 - k) + 1 for k in range(2 * n - 1)]


def test_poly_mul_unreduced_and_zero_inputs(koe):
    rng = random.Random(5)
    for na, nb in ((1, 1), (7, 300), (300, 7), (257, 513), (1000, 1000)):
        a = [rng.choice([rng.randrange(N, 1 << 256), TOP, N, N + 1, rng.randrange(1 << 256)]) for _ in range(na)]
        b = [rng.choice([rng.randrange(N, 1 << 256), TOP, N, 0, rng.randrange(1 << 256)]) for _ in range(nb)]
        ar, br = [v % N for v in a], [v % N for v in b]
        assert poly_mul(koe, a, b) == [coeff(ar, br, k) for k in range(na + nb - 1)], (na, nb)
    a = [rng.randrange(N) for _ in range(700)]
    assert poly_mul(koe, a, [0] * 300) == [0] * 999
    assert poly_mul(koe, [0] * 300, a) == [0] * 999
    assert poly_mul(koe, [N] * 5, a) == [0] * 704


def test_poly_mul_host_buffer_form(vm):
    rng = random.Random(6)
    a = [rng.randrange(1 << 256) for _ in range(130)]
    b = [rng.randrange(1 << 256) for _ in range(70)]
    got = to_ints(vm._native.bn256_fr_poly_mul(to_arr(a), to_arr(b)))
    assert got == [coeff([v % N for v in a], [v % N for v in b], k) for k in range(199)]


def test_poly_mul_above_the_cap_is_e_range_and_writes_nothing(vm):
    nat = vm._native
    ctx = vm.get_context()
    cap = nat.BN256_FR_POLY_MAX
    pattern = np.full(64, 0xA5, np.uint8)
    a, b, out = ctx.upload(to_arr([3, 4])), ctx.upload(to_arr([5])), ctx.upload(pattern)
    for na, nb in ((cap + 1, 1), (1, cap + 1), (cap + 1, cap + 1)):
        with pytest.raises(nat.VmpcError) as ei:
            ctx.bn256_fr_poly_mul(a.ptr, na, b.ptr, nb, out.ptr)
        assert ei.value.code == nat.E_RANGE
        ctx.sync()
        assert np.array_equal(ctx.download(out.ptr, 64), pattern)
    # at lengths it supports the same buffers are written
    ctx.bn256_fr_poly_mul(a.ptr, 2, b.ptr, 1, out.ptr)
    ctx.sync()
    assert to_ints(ctx.download(out.ptr, 64)) == [15, 20]
    # the host-buffer form refuses before it creates a context or reads a byte
    lib = nat.load_library()
    host_out = pattern.copy()
    rc = lib.vmpc_bn256_fr_poly_mul(nat._np_ptr(to_arr([3])), cap + 1, nat._np_ptr(to_arr([5])), 1, nat._np_ptr(host_out))
    assert rc == nat.E_RANGE and np.array_equal(host_out, pattern)


# ---- fr_powers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 2, 64, 1 << 16])
def test_fr_powers(vm, koe, count):
    ctx = vm.get_context()
    rng = random.Random(count)
    for z in (0, 1, N - 1, rng.randrange(N)):
        for scale in (0, 1, N - 1, rng.randrange(N)):
            buf = koe.fr_powers(z, scale, count)
            ctx.sync()
            got = to_ints(ctx.download(buf.ptr, 32 * count))
            want, v = [], scale
            for _ in range(count):
                v = v * z % N
                want.append(v)
            assert got == want, (z, scale)


# ---- parity with the reference-made fixture --------------------------------------------------------------------------

class Replay:
    """stands in for the module's prng: hands out the recorded draws in order"""

    def __init__(self, draws):
        self.draws = list(draws)

    def randrange(self, *args):
        return self.draws.pop(0)


class ForeignPoint:
    """an MPyC-style element: normalize() and indexable coordinates (twist coordinates are pairs)"""

    def __init__(self, coords):
        self.coords = coords

    def normalize(self):
        return self

    def __getitem__(self, k):
        return self.coords[k]


def g1c(v):
    return None if v is None else (h2i(v[0]), h2i(v[1]))


def g2c(v):
    return None if v is None else (h2i(v[0]), h2i(v[1]), h2i(v[2]), h2i(v[3]))


def seeded_setup(vm, koe, s, n=None):
    koe.prng = Replay([h2i(s["g_exp"]), h2i(s["alpha"]), h2i(s["z"])])
    P = vm.pynocchio
    pp = koe.trusted_setup(P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2), n or s["n"], N)
    assert koe.prng.draws == []
    return pp


def list_pp(vm, s, foreign=False):
    P = vm.pynocchio
    if foreign:
        return {"pp_lhs": [ForeignPoint(g1c(p)) for p in s["pp_lhs"]],
                "pp_rhs": [ForeignPoint(((c[0], c[1]), (c[2], c[3]))) for c in map(g2c, s["pp_rhs"])]}
    return {"pp_lhs": [P.BN256Point(g1c(p)) for p in s["pp_lhs"]],
            "pp_rhs": [P.BN256TwistPoint(g2c(p)) for p in s["pp_rhs"]]}


def form(vm, o):
    gf = vm.GF(N)
    coeffs = [gf(h2i(c)) for c in o["L"]]
    if h2i(o["constant"]):
        return vm.pivot.AffineForm(coeffs, gf(h2i(o["constant"])))
    return vm.pivot.LinearForm(coeffs)


def test_trusted_setup_matches_reference_point_for_point(vm, koe, fx):
    for s in fx["setups"]:
        pp = seeded_setup(vm, koe, s)
        assert len(pp["pp_lhs"]) == len(pp["pp_rhs"]) == 2 * s["n"]
        assert [p.coords for p in pp["pp_lhs"]] == [g1c(p) for p in s["pp_lhs"]]
        assert [p.coords for p in pp["pp_rhs"]] == [g2c(p) for p in s["pp_rhs"]]
        assert pp["pp_lhs"][0].coords == pp["pp_lhs"][-2 * s["n"]].coords == g1c(s["pp_lhs"][0])
        assert isinstance(pp["pp_lhs"][1], vm.pynocchio.BN256Point)
        assert isinstance(pp["pp_rhs"][1], vm.pynocchio.BN256TwistPoint)


@pytest.mark.parametrize("pp_kind", ["device", "lists", "foreign"])
def test_prover_and_verifier_match_reference(vm, koe, fx, pp_kind):
    gf = vm.GF(N)
    for s in fx["setups"]:
        pp = seeded_setup(vm, koe, s) if pp_kind == "device" else list_pp(vm, s, pp_kind == "foreign")
        for o in s["openings"]:
            L = form(vm, o)
            x, gamma = [gf(h2i(v)) for v in o["x"]], gf(h2i(o["gamma"]))
            proof, u = koe.opening_linear_form_prover(L, x, gamma, pp)
            assert proof["P"].coords == g1c(o["P"]), o["name"]
            assert proof["pi"].coords == g2c(o["pi"]), o["name"]
            assert proof["Q"].coords == g1c(o["Q"]), o["name"]
            assert int(u) % N == h2i(o["u"]) and u == L(x)
            assert koe.opening_linear_form_verifier(L, pp, proof, u) == o["verification"]
        for r in s["restrictions"]:
            x, gamma = [h2i(v) for v in r["x"]], h2i(r["gamma"])
            P, pi = koe.restriction_argument_prover(r["S"], x, gamma, pp)
            assert P.coords == g1c(r["P"]) and pi.coords == g2c(r["pi"])
            assert koe.restriction_argument_verifier(P, pi, pp) is r["verification"]
            # a range is a subset too
            P2, pi2 = koe.restriction_argument_prover(range(len(x)), x, gamma, pp)
            assert koe.restriction_argument_verifier(P2, pi2, pp) is True and P2 != P


def test_zero_witness_gives_identity_proof_that_verifies(vm, koe, fx):
    s = fx["setups"][3]
    pp = seeded_setup(vm, koe, s)
    L = form(vm, s["openings"][0])
    proof, u = koe.opening_linear_form_prover(L, [0] * 4, 0, pp)
    assert proof["P"].coords is None and proof["pi"].coords is None and proof["Q"].coords is None and int(u) == 0
    assert koe.opening_linear_form_verifier(L, pp, proof, u) == {"restriction_arg_check": True, "PRQ_check": True}


# ---- the prover against the trapdoor, at size ------------------------------------------------------------------------

@pytest.mark.parametrize("log_n", [10, 13, 16])
def test_prover_against_trapdoor(vm, koe, log_n):
    n = 1 << log_n
    rng = random.Random(100 + log_n)
    g_exp, alpha, z = rng.randrange(1, N), rng.randrange(N), rng.randrange(N)
    pp = seeded_setup(vm, koe, {"g_exp": hex(g_exp), "alpha": hex(alpha), "z": hex(z)}, n)
    x = [rng.randrange(N) for _ in range(n)]
    gamma = rng.randrange(N)
    coeffs = [rng.randrange(N) for _ in range(n)]
    proof, u = koe.opening_linear_form_prover(vm.pivot.LinearForm(coeffs), x, gamma, pp)
    assert int(u) % N == sum(c * v for c, v in zip(coeffs, x)) % N
    zp = [1]
    for _ in range(n + 1):
        zp.append(zp[-1] * z % N)
    a_z = (gamma + sum(v * zp[i + 1] for i, v in enumerate(x))) % N
    b_z = sum(coeffs[n - 1 - j] * zp[j] for j in range(n)) % N
    commit = g_exp * z % N * a_z % N
    assert proof["P"].coords == bn.E1.mul(commit, bn.G1)
    pi = bn.E2.mul(alpha * commit % N, bn.G2)
    assert proof["pi"].coords == (*pi[0], *pi[1])
    q = g_exp * z % N * ((a_z * b_z - int(u) * zp[n]) % N) % N
    assert proof["Q"].coords == bn.E1.neg(bn.E1.mul(q, bn.G1))
    if log_n == 10:
        assert koe.opening_linear_form_verifier(vm.pivot.LinearForm(coeffs), pp, proof, u) == \
            {"restriction_arg_check": True, "PRQ_check": True}


# ---- soundness of the verifier ---------------------------------------------------------------------------------------

def test_verifier_soundness(vm, koe, fx):
    P = vm.pynocchio
    s = fx["setups"][1]
    pp = seeded_setup(vm, koe, s)
    o = s["openings"][1]                                   # the affine form
    L = form(vm, o)
    gf = vm.GF(N)
    x, gamma = [gf(h2i(v)) for v in o["x"]], gf(h2i(o["gamma"]))
    proof, u = koe.opening_linear_form_prover(L, x, gamma, pp)
    ok = {"restriction_arg_check": True, "PRQ_check": True}
    assert koe.opening_linear_form_verifier(L, pp, proof, u) == ok
    other_g1 = P.BN256Point(bn.E1.mul(12345, bn.G1))
    t = bn.E2.mul(6789, bn.G2)
    other_g2 = P.BN256TwistPoint((*t[0], *t[1]))
    both, prq, restr = dict(ok, restriction_arg_check=False, PRQ_check=False), dict(ok, PRQ_check=False), \
        dict(ok, restriction_arg_check=False)
    assert koe.opening_linear_form_verifier(L, pp, dict(proof, P=other_g1), u) == both
    assert koe.opening_linear_form_verifier(L, pp, dict(proof, pi=other_g2), u) == restr
    assert koe.opening_linear_form_verifier(L, pp, dict(proof, Q=other_g1), u) == prq
    assert koe.opening_linear_form_verifier(L, pp, proof, u + 1) == prq
    bent = list(L.coeffs)
    bent[2] = bent[2] + 1
    assert koe.opening_linear_form_verifier(vm.pivot.AffineForm(bent, L.constant), pp, proof, u) == prq
    other_pp = seeded_setup(vm, koe, fx["setups"][3], s["n"])
    assert koe.opening_linear_form_verifier(L, other_pp, proof, u) == both
    assert koe.restriction_argument_verifier(proof["P"], proof["pi"], pp) is True
    assert koe.restriction_argument_verifier(other_g1, proof["pi"], pp) is False
    for name, bad in (("P", P.BN256Point((1, 1))), ("pi", P.BN256TwistPoint((1, 2, 3, 4))), ("Q", P.BN256Point((5, 7)))):
        with pytest.raises(ValueError, match=name):
            koe.opening_linear_form_verifier(L, pp, dict(proof, **{name: bad}), u)
    with pytest.raises(ValueError, match="pp_lhs"):
        lists = list_pp(vm, s)
        lists["pp_lhs"][0] = P.BN256Point((1, 1))
        koe.opening_linear_form_verifier(L, lists, proof, u)
