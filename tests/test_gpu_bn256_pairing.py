"""GPU parity of the BN-256 optimal-ate pairing and the Pinocchio verifier (csrc/bn256_pairing.hip,
verifiable_mpc_amd/pynocchio.py pairing / verify / verify_batch) against the reference-made fixture
(tests/golden/bn256_pairing.json) and the Python restatement (tests/bn256_pairing_ref.py)."""
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import bn256_pairing_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
h2i = lambda s: int(s, 16)

# which checks read which proof element (trinocchio/pynocchio.py:276-325)
READS = {
    "r_v*v_mid*g1": {"H", "V", "Z"},
    "r_w*w_mid*g2": {"H", "W", "Z"},
    "r_y*y_mid*g1": {"H", "Y", "Z"},
    "h*g1": {"H"},
    "r_v*alpha_v*v_mid*g1": {"V"},
    "r_w*alpha_w*w_mid*g1": {"W"},
    "r_y*alpha_y*y_mid*g1": {"Y"},
    "r_v*beta*v_mid+r_w*beta*w_mid+r_y*beta*y_mid*g1": {"Z"},
}


@pytest.fixture(scope="module")
def pn():
    import verifiable_mpc_amd as v
    v.get_context()
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def fx():
    return load_golden("bn256_pairing.json")


def g1_pt(pn, v):
    return pn.BN256Point(None if v is None else tuple(v))


def g2_pt(pn, v):
    return pn.BN256TwistPoint(None if v is None else (v[0][0], v[0][1], v[1][0], v[1][1]))


def as_ref(gt):
    return tuple(gt.coeffs)


def instance(pn, fx):
    case = fx["pinocchio"]

    def mk(v, name):
        cls = pn.BN256TwistPoint if name.endswith("g2") else pn.BN256Point
        return cls(None if v is None else [h2i(x) for x in v])

    class Q:
        indices_io = case["indices_io"]
        indices_mid = case["indices_mid"]
    verikey = {k: mk(v, k) for k, v in case["verikey"].items()}
    evalkey = {k: mk(v, k) for k, v in case["evalkey"].items()}
    proof = {k: mk(v, k) for k, v in case["proof"].items()}
    return Q, verikey, evalkey, proof, [h2i(v) for v in case["c"]]


def doubled(pn, pt):
    if pt.group == 1:
        return pn.BN256Point(bn.E1.add(pt.coords, pt.coords))
    c = pt.coords
    q = ((c[0], c[1]), (c[2], c[3]))
    return pn.BN256TwistPoint(bn.E2.add(q, q))


def test_pairing_matches_reference_fixture(pn, fx):
    for case in fx["pairing"]:
        a = pn.BN256Point(None if case["g1"] is None else [h2i(v) for v in case["g1"]])
        b = pn.BN256TwistPoint(None if case["g2"] is None else [h2i(v) for v in case["g2"]])
        got = pn.pairing(a, b)
        assert got.coeffs == tuple(h2i(v) for v in case["gt"]), case["name"]
        assert got.is_one() == (case["g1"] is None or case["g2"] is None)


def test_pairing_matches_restatement_on_random_points(pn):
    rng = random.Random(31)
    for _ in range(3):
        p, q = bn.E1.mul(rng.randrange(1, bn.N), bn.G1), bn.E2.mul(rng.randrange(1, bn.N), bn.G2)
        got = pn.pairing(g1_pt(pn, p), g2_pt(pn, q))
        assert as_ref(got) == R.pairing(p, q)
        assert hash(got) == hash(pn.GT(got.coeffs)) and got == pn.GT(got.coeffs)


@pytest.mark.parametrize("n", [1, 13, 4097])
def test_pairing_batches(pn, n):
    """vmpc_bn256_pairing_dev over n pairs (partial waves and blocks): e(k G1, G2) = e(G1, G2)^k"""
    from verifiable_mpc_amd.device import get_context
    ctx = get_context()
    rng = random.Random(n)
    k0 = rng.randrange(1, bn.N)
    inf_j = n // 2 if n > 2 else -1              # one point at infinity in the middle of the longer batches
    p = bn.E1.mul(k0, bn.G1)
    g1 = []
    for j in range(n):
        g1.append(bn.g1_to_bytes(p if j != inf_j else None))
        p = bn.E1.add(p, bn.G1)
    g1 = np.frombuffer(b"".join(g1), np.uint8).reshape(n, 64)
    g2 = np.tile(np.frombuffer(bn.g2_to_bytes(bn.G2), np.uint8), (n, 1))
    d1, d2, out = ctx.upload(g1), ctx.upload(g2), ctx.alloc(384 * n)
    ctx.bn256_pairing(d1.ptr, d2.ptr, n, out.ptr)
    ctx.sync()
    raw = ctx.download(out.ptr, 384 * n).tobytes()
    gts = [tuple(int.from_bytes(raw[384 * j + 32 * i:384 * j + 32 * i + 32], "little") for i in range(12))
           for j in range(n)]
    e = R.pairing(bn.G1, bn.G2)
    assert gts[0] == R.gt_pow(e, k0)
    if inf_j >= 0:
        assert gts[inf_j] == R.GT_ONE
    # consecutive multiples differ by a factor e (skipping the infinity entry); a sample checked absolutely
    for j in range(n - 1):
        if inf_j in (j, j + 1):
            continue
        assert gts[j + 1] == R.gt_mul(gts[j], e), j
    for j in {n - 1, n // 3}:
        if j != inf_j:
            assert gts[j] == R.gt_pow(e, k0 + j), j


def test_pairing_product_is_one(pn):
    rng = random.Random(3)
    a = rng.randrange(2, bn.N)
    P, Q = bn.E1.mul(rng.randrange(1, bn.N), bn.G1), bn.E2.mul(rng.randrange(1, bn.N), bn.G2)
    g1 = [g1_pt(pn, bn.E1.mul(a, P)), g1_pt(pn, bn.E1.neg(P)), g1_pt(pn, bn.E1.mul(a, P)), g1_pt(pn, bn.E1.neg(P))]
    g2 = [g2_pt(pn, Q), g2_pt(pn, bn.E2.mul(a, Q)), g2_pt(pn, Q), g2_pt(pn, bn.E2.mul(a + 1, Q))]
    gts, ones = pn.pairing_product(g1, g2, [0, 2, 4])
    assert ones == [True, False]
    assert gts[0].is_one() and not gts[1].is_one()


def test_pairing_product_lengths_and_offsets(pn):
    """products of 1..12 pairs at arbitrary offsets equal the single pairings multiplied by the restatement"""
    from verifiable_mpc_amd.device import get_context
    ctx = get_context()
    rng = random.Random(12)
    lengths = list(range(1, 13)) + [0, 3]
    rng.shuffle(lengths)
    n = sum(lengths)
    ks = [rng.randrange(1, bn.N) for _ in range(n)]
    # few distinct points keep the host side cheap: P_j = k_j G1 against a handful of twist multiples
    qs = [bn.E2.mul(rng.randrange(1, bn.N), bn.G2) for _ in range(3)]
    g1 = [g1_pt(pn, bn.E1.mul(k, bn.G1)) for k in ks]
    g2 = [g2_pt(pn, qs[j % 3]) for j in range(n)]
    offsets = np.cumsum([0] + lengths).tolist()
    gts, ones = pn.pairing_product(g1, g2, offsets)
    # singles on the GPU
    a1 = np.frombuffer(b"".join(p.to_bytes() for p in g1), np.uint8).reshape(n, 64)
    a2 = np.frombuffer(b"".join(q.to_bytes() for q in g2), np.uint8).reshape(n, 128)
    d1, d2, out = ctx.upload(a1), ctx.upload(a2), ctx.alloc(384 * n)
    ctx.bn256_pairing(d1.ptr, d2.ptr, n, out.ptr)
    ctx.sync()
    raw = ctx.download(out.ptr, 384 * n).tobytes()
    singles = [pn.GT.from_bytes(raw[384 * j:384 * j + 384]) for j in range(n)]
    # two singles pinned against the restatement, the rest by the products
    for j in (0, n - 1):
        assert as_ref(singles[j]) == R.pairing(bn.E1.mul(ks[j], bn.G1), qs[j % 3])
    for k, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        want = R.GT_ONE
        for j in range(lo, hi):
            want = R.gt_mul(want, as_ref(singles[j]))
        assert as_ref(gts[k]) == want, (k, lo, hi)
        assert ones[k] == (hi == lo)


def test_verify_fixture_proof(pn, fx):
    Q, verikey, _, proof, c = instance(pn, fx)
    res = pn.verify(Q, verikey, proof, c)
    assert list(res) == ["H", "V", "W", "Y", "Z"]
    assert res == {"H": True, "V": True, "W": True, "Y": True, "Z": True} == fx["pinocchio"]["verification"]
    assert all(type(v) is bool for v in res.values())


@pytest.mark.parametrize("name", sorted(READS))
def test_verify_tampered_element(pn, fx, name):
    Q, verikey, _, proof, c = instance(pn, fx)
    bad = dict(proof)
    bad[name] = doubled(pn, proof[name])
    res = pn.verify(Q, verikey, bad, c)
    assert {k for k, ok in res.items() if not ok} == READS[name]


def test_verify_proof_from_compute_proof(pn, fx):
    Q, verikey, evalkey, proof, c = instance(pn, fx)
    case = fx["pinocchio"]

    class H:
        coeffs = [h2i(v) for v in case["h"]]

        def __len__(self):
            return len(self.coeffs)

    class D:
        v, w, y = (h2i(x) for x in case["deltas"])
    mine = pn.compute_proof(Q, c, H(), evalkey, D)
    assert mine == proof
    assert all(pn.verify(Q, verikey, mine, c).values())
    key = pn.PreparedKey(Q, evalkey)
    assert all(pn.verify(Q, verikey, pn.compute_proof(Q, c, H(), key, D), c).values())


def test_verify_batch_matches_verify(pn, fx):
    Q, verikey, _, proof, c = instance(pn, fx)
    variants = [(proof, c)]
    for name in sorted(READS):
        bad = dict(proof)
        bad[name] = doubled(pn, proof[name])
        variants.append((bad, c))
    c_bad = list(c)
    c_bad[Q.indices_io[0]] += 1
    variants.append((proof, c_bad))
    single = [pn.verify(Q, verikey, p, cc) for p, cc in variants]
    assert single[-1]["H"] is False and all(v for k, v in single[-1].items() if k != "H")
    rng = random.Random(1000)
    picks = [0 if rng.random() < 0.5 else rng.randrange(len(variants)) for _ in range(1000)]
    got = pn.verify_batch(Q, verikey, [variants[i][0] for i in picks], [variants[i][1] for i in picks])
    assert got == [single[i] for i in picks]
    assert pn.verify_batch(Q, verikey, [], []) == []


def test_off_curve_point_raises(pn, fx):
    Q, verikey, _, proof, c = instance(pn, fx)
    bad = dict(proof)
    x, y = proof["h*g1"].coords
    bad["h*g1"] = pn.BN256Point((x, y + 1))
    with pytest.raises(ValueError, match="h\\*g1"):
        pn.verify(Q, verikey, bad, c)
    with pytest.raises(ValueError, match="proof 2"):
        pn.verify_batch(Q, verikey, [proof, proof, bad], [c, c, c])
    key = dict(verikey)
    x, y = verikey["alpha_w*g1"].coords
    key["alpha_w*g1"] = pn.BN256Point((x + 1, y))
    with pytest.raises(ValueError, match="alpha_w"):
        pn.verify(Q, key, proof, c)
    with pytest.raises(ValueError):
        pn.pairing(pn.BN256Point((1, 3)), pn.BN256TwistPoint(None))
