"""GPU key generation for Pinocchio (verifiable_mpc_amd/pynocchio.py Trapdoor .. PreparedKey.generate, R1CSQAP;
csrc/bn256_keygen.hip): parity with the reference-made fixture (tests/golden/pinocchio_keygen.json), proofs over
generated keys, exact key vectors at scale against bn256_fixed_base of the restated exponents (tests/keygen_ref.py)
and the oracle, and edges.  Every comparison is exact."""
import random
import types

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import keygen_ref as K
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N = K.N
h2i = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def pn():
    import verifiable_mpc_amd as v
    v.get_context()
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def ctx(pn):
    from verifiable_mpc_amd import get_context
    return get_context()


@pytest.fixture(scope="module")
def fx():
    return load_golden("pinocchio_keygen.json")["cases"]


class _Poly:
    def __init__(self, coeffs):
        self.coeffs = coeffs

    def __len__(self):
        return len(self.coeffs)


class DenseQAP:
    """the reference QAP's attributes, rebuilt from the fixture's coefficients"""

    def __init__(self, case):
        q = case["qap"]
        self.v = [_Poly([h2i(c) for c in p]) for p in q["v"]]
        self.w = [_Poly([h2i(c) for c in p]) for p in q["w"]]
        self.y = [_Poly([h2i(c) for c in p]) for p in q["y"]]
        self.t = _Poly([h2i(c) for c in q["t"]])
        self.d, self.m, self.out_ix = case["d"], case["m"], case["out_ix"]
        self.indices = range(self.m + 1)
        self.indices_io_and_0 = range(0, self.out_ix + 1)
        self.indices_io = range(1, self.out_ix + 1)
        self.indices_mid = range(self.out_ix + 1, self.m + 1)


def _qaps(pn, case):
    r = case["r1cs"]
    return {"dense": DenseQAP(case), "r1cs": pn.R1CSQAP(r["V"], r["W"], r["Y"], case["out_ix"], m=case["m"])}


def _gen(pn, td):
    return pn.Generators(td, pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2))


def _enc(pt):
    if pt.coords is None:
        return None
    return [format(v, "x") for v in pt.coords]


def _from_enc(pn, name, enc):
    cls = pn.BN256TwistPoint if name.endswith("g2") else pn.BN256Point
    return cls(None if enc is None else [h2i(x) for x in enc])


def _coords(pt):
    """oracle point -> the coords tuple of a BN256Point / BN256TwistPoint"""
    if pt is None:
        return None
    return tuple(pt) if isinstance(pt[0], int) else (*pt[0], *pt[1])


def _seeded_td(pn, case):
    pn.prng = random.Random(case["seed"])
    try:
        return pn.Trapdoor(N)
    finally:
        pn.prng = random.SystemRandom()


def test_trapdoor_and_deltas_follow_the_reference_draws(pn, fx):
    for case in fx:
        td = _seeded_td(pn, case)
        for k, v in case["trapdoor"].items():
            assert getattr(td, k) == h2i(v), k
        pn.prng = random.Random(case["seed"])
        try:
            pn.Trapdoor(N)
            # the fixture's witness comes between Trapdoor and SampleDeltas without drawing
            dl = pn.SampleDeltas(N)
        finally:
            pn.prng = random.SystemRandom()
        assert [dl.v, dl.w, dl.y] == [h2i(x) for x in case["deltas"]]


@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_reference_parity(pn, fx, form):
    """generate_evalkey / generate_verikey == the reference's keys, names and order included"""
    for case in fx:
        td = _seeded_td(pn, case)
        qap = _qaps(pn, case)[form]
        gen = _gen(pn, td)
        for name, want in (("evalkey", case["evalkey"]), ("verikey", case["verikey"])):
            key = (pn.generate_evalkey if name == "evalkey" else pn.generate_verikey)(td, qap, gen)
            assert list(key) == [k for k, _ in want], (case["name"], form, name)
            for k, enc in want:
                assert _enc(key[k]) == enc, (case["name"], form, name, k)


def _proof_inputs(case):
    c = [h2i(x) for x in case["c"]]
    h = [h2i(x) for x in case["h"]]
    dv, dw, dy = (h2i(x) for x in case["deltas"])
    return c, h, types.SimpleNamespace(v=dv, w=dw, y=dy)


@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_generated_key_proves_and_verifies(pn, fx, form):
    for case in fx:
        td = _seeded_td(pn, case)
        qap = _qaps(pn, case)[form]
        gen = _gen(pn, td)
        key = pn.PreparedKey.generate(td, qap, gen)
        c, h, deltas = _proof_inputs(case)
        proof = pn.compute_proof(qap, c, h, key, deltas)
        for k, enc in case["proof"].items():
            assert _enc(proof[k]) == enc, (case["name"], form, k)
        verikey = pn.generate_verikey(td, qap, gen)
        assert pn.verify(qap, verikey, proof, c) == {k: True for k in "HVWYZ"}
        # the same against a key dict made by generate_evalkey, element by element
        key2 = pn.PreparedKey(qap, pn.generate_evalkey(td, qap, gen))
        proof2 = pn.compute_proof(qap, c, h, key2, deltas)
        assert {k: _enc(p) for k, p in proof2.items()} == {k: _enc(p) for k, p in proof.items()}


def test_tampered_trapdoor_fails_h(pn, fx):
    """a key made at s + 1 proves against a verification key made at s: the H check fails"""
    case = fx[1]
    td = _seeded_td(pn, case)
    bad = K.TD(td.r_v, td.r_w, (td.s + 1) % N, td.alpha_v, td.alpha_w, td.alpha_y, td.beta, td.gamma, td.r_y)
    for form, qap in _qaps(pn, case).items():
        key = pn.PreparedKey.generate(bad, qap, _gen(pn, bad))
        c, h, deltas = _proof_inputs(case)
        proof = pn.compute_proof(qap, c, h, key, deltas)
        vk = {k: _from_enc(pn, k, e) for k, e in case["verikey"]}
        got = pn.verify(qap, vk, proof, c)
        assert got["H"] is False, form


# ---- scale: synthetic R1CS, whole key vectors ---------------------------------------------------------------------

def _random_td(seed):
    r = random.Random(seed)
    return K.TD(*(r.randrange(N) for _ in range(8)))


def _download(ctx, group, buf, count):
    return ctx.download(buf.ptr, 64 * group * count).reshape(count, 64 * group)


def _fixed_base(ctx, group, exps):
    base = bn.g1_to_bytes(bn.G1) if group == 1 else bn.g2_to_bytes(bn.G2)
    db, de = ctx.upload(np.frombuffer(base, np.uint8)), ctx.upload(K.to_array(exps))
    out = ctx.alloc(64 * group * len(exps))
    ctx.bn256_fixed_base(group, db.ptr, de.ptr, len(exps), out.ptr)
    ctx.sync()
    return _download(ctx, group, out, len(exps))


@pytest.mark.parametrize("log_d", [12, 16, 18])
def test_scale_key_vectors_exact(pn, ctx, log_d):
    d = 1 << log_d
    V, W, Y, out_ix, m = K.synthetic_r1cs(d, seed=log_d)
    lens = np.bincount(np.concatenate([V[1], W[1]]), minlength=m + 1)
    assert lens[0] > d // 2 and lens[0] > 100 * np.median(lens[1:])       # the skewed wire-0 column
    qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
    td = _random_td(log_d)
    gen = _gen(pn, td)
    vecs = pn.evalkey_vectors(td, qap, gen)
    v, w, y, t = K.qap_at(K.csr_entries(V), K.csr_entries(W), K.csr_entries(Y), m + 1, d, td.s)
    mid = list(qap.indices_mid)
    ex = K.key_exponents(td, v, w, y, t, mid)
    ex["h*g1"] = [pow(td.s, i, N) for i in range(d + 1)]
    assert list(vecs) == list(K.ELEMENT_NAMES) + ["h*g1"]
    for name, (group, buf, count) in vecs.items():
        assert count == len(ex[name]), name
        got = _download(ctx, group, buf, count)
        want = _fixed_base(ctx, group, ex[name])
        assert np.array_equal(got, want), name
        if log_d == 16:
            E, G = (bn.E1, bn.G1) if group == 1 else (bn.E2, bn.G2)
            to_b = bn.g1_to_bytes if group == 1 else bn.g2_to_bytes
            cols = random.Random(name).sample(range(count - 3), 13) + [count - 3, count - 2, count - 1]
            for j in cols:
                assert got[j].tobytes() == to_b(E.mul(ex[name][j], G)), (name, j)


def test_h_zero_circuit_proves_at_2_16(pn, ctx):
    """rows x_j * one = y_j with y_j = x_j: p(x) = 0, h = 0, no deltas; a proof over the generated key verifies"""
    d = 1 << 16
    n_io = 4
    # wires: 0 one, 1..n_io io, then x_1..x_d, y_1..y_d
    x_w = n_io + 1 + np.arange(d)
    y_w = x_w + d
    ptr = np.arange(d + 1)
    ones = np.ones(d, np.int64)
    V, W, Y = (ptr, x_w, ones), (ptr, np.zeros(d, np.int64), ones), (ptr, y_w, ones)
    qap = pn.R1CSQAP(V, W, Y, n_io, m=n_io + 2 * d)
    rng = np.random.default_rng(5)
    c = np.zeros((qap.m + 1, 32), np.uint8)
    c[0, 0] = 1
    c[1:n_io + 1, :8] = rng.integers(0, 256, size=(n_io, 8), dtype=np.uint8)
    c[x_w, :31] = rng.integers(0, 256, size=(d, 31), dtype=np.uint8)
    c[y_w] = c[x_w]
    td = _random_td(99)
    gen = _gen(pn, td)
    key = pn.PreparedKey.generate(td, qap, gen)
    proof = pn.compute_proof(qap, c, [0], key)
    verikey = pn.generate_verikey(td, qap, gen)
    cl = [int.from_bytes(c[i].tobytes(), "little") for i in range(n_io + 1)]
    assert pn.verify(qap, verikey, proof, cl) == {k: True for k in "HVWYZ"}


# ---- edges ----------------------------------------------------------------------------------------------------------

def _vwyt(pn, ctx, qap, s):
    at = pn._QAPAtS(ctx, qap, s)
    ctx.sync()
    nw = len(qap.indices)
    raw = ctx.download(at.vwyt.ptr, 32 * (3 * nw + 1)).reshape(-1, 32)
    vals = [int.from_bytes(r.tobytes(), "little") for r in raw]
    return vals[:nw], vals[nw:2 * nw], vals[2 * nw:3 * nw], vals[3 * nw]


@pytest.mark.parametrize("which", ["0", "1", "d"])
def test_special_s_sparse_and_dense(pn, ctx, fx, which):
    for case in fx:
        d = case["d"]
        s = {"0": 0, "1": 1, "d": d}[which]
        r = case["r1cs"]
        want = K.qap_at(K.entries_of_rows(r["V"]), K.entries_of_rows(r["W"]), K.entries_of_rows(r["Y"]),
                        case["m"] + 1, d, s)
        for form, qap in _qaps(pn, case).items():
            assert _vwyt(pn, ctx, qap, s) == want, (case["name"], form, which)
    # and the basis itself on a longer range (several scan lanes), s inside it
    for d, s in ((1000, 0), (1000, 1), (1000, 1000), (1000, 517), (4097, 4097), (4097, 12345)):
        ell = ctx.alloc(32 * d)
        t = ctx.alloc(32)
        sb = ctx.upload(K.to_array([s]))
        ctx.bn256_qap_lagrange(sb.ptr, d, ell.ptr, t.ptr)
        ctx.sync()
        got = [int.from_bytes(r.tobytes(), "little") for r in ctx.download(ell.ptr, 32 * d).reshape(-1, 32)]
        want_ell, want_t = K.lagrange_at(s, d)
        assert got == want_ell, (d, s)
        assert int.from_bytes(ctx.download(t.ptr, 32).tobytes(), "little") == want_t


@pytest.mark.parametrize("d", [1, 63, 64, 65, 16383, 16384, 16385, 32769])
def test_lagrange_basis_at_scan_boundaries(ctx, d):
    """csrc/fr_scan.h over GF(n) with runs of KG_RUN = 64 elements, three sequences: d = 63, 64, 65 is a run one short
    of full, full and a second lane of one element; 16383 / 16384 give 256 lanes (one per scanning thread), 16385 gives
    257 (two per thread, 127 threads with none, the one that hands on the total among them), 32769 gives 513 (three per
    thread).  s on a node (16384: the last element of lane 255) turns the products to zero in the middle of a run."""
    rng = random.Random(6000 + d)
    ell, t = ctx.alloc(32 * (d + 1)), ctx.alloc(32)
    for s in [rng.randrange(d + 1, N), 0] + sorted({v for v in (1, 64, 65, 16384, d) if v <= d}):
        ctx.upload_into(ell.ptr, K.to_array([7] * (d + 1)))
        sb = ctx.upload(K.to_array([s]))
        ctx.bn256_qap_lagrange(sb.ptr, d, ell.ptr, t.ptr)
        ctx.sync()
        got = [int.from_bytes(r.tobytes(), "little") for r in ctx.download(ell.ptr, 32 * (d + 1)).reshape(-1, 32)]
        want_ell, want_t = K.lagrange_at(s, d)
        assert got == want_ell + [7], (d, s)
        assert int.from_bytes(ctx.download(t.ptr, 32).tobytes(), "little") == want_t, (d, s)


def _restated_evalkey(td, ents, n_cols, d, mid):
    v, w, y, t = K.qap_at(*ents, n_cols, d, td.s)
    out = {}
    for name, group, e in K.evalkey_exponents(td, v, w, y, t, mid, d):
        E, G = (bn.E1, bn.G1) if group == 1 else (bn.E2, bn.G2)
        out[name] = E.mul(e, G)
    return out


@pytest.mark.parametrize("layout", ["no_mid", "no_io"])
def test_circuit_without_mid_or_io(pn, layout):
    rng = random.Random(layout)
    d, m = 6, 5
    rows = [[[rng.randrange(-3, 4) for _ in range(m + 1)] for _ in range(d)] for _ in range(3)]
    out_ix = m if layout == "no_mid" else 0
    qap = pn.R1CSQAP(rows[0], rows[1], rows[2], out_ix, m=m)
    assert (len(qap.indices_mid) == 0) == (layout == "no_mid") and (len(qap.indices_io) == 0) == (layout == "no_io")
    td = _random_td(len(layout))
    key = pn.generate_evalkey(td, qap, _gen(pn, td))
    want = _restated_evalkey(td, [K.entries_of_rows(r) for r in rows], m + 1, d, list(qap.indices_mid))
    assert list(key) == list(want)
    for k in want:
        assert key[k].coords == _coords(want[k]), k


def test_off_curve_generator_raises(pn, fx):
    td = _random_td(3)
    bad1 = pn.BN256Point((1, 3))
    bad2 = pn.BN256TwistPoint((1, 2, 3, 4))
    with pytest.raises(ValueError):
        pn.Generators(td, bad1, pn.BN256TwistPoint(bn.G2))
    with pytest.raises(ValueError):
        pn.Generators(td, pn.BN256Point(bn.G1), bad2)
    qap = _qaps(pn, fx[0])["r1cs"]
    gen = types.SimpleNamespace(g1=bad1, g2=pn.BN256TwistPoint(bn.G2))
    with pytest.raises(ValueError):
        pn.generate_evalkey(td, qap, gen)
    with pytest.raises(ValueError):
        pn.PreparedKey.generate(td, qap, gen)
    with pytest.raises(ValueError):
        pn.generate_verikey(td, qap, types.SimpleNamespace(g1=pn.BN256Point(bn.G1), g2=bad2))


def test_d_above_cap_is_range(pn, ctx):
    from verifiable_mpc_amd import _native
    cap = 1 << 22
    with pytest.raises(_native.VmpcError) as ei:
        ctx.bn256_qap_lagrange(0, cap + 1, 0, 0)
    assert ei.value.code == _native.E_RANGE
    with pytest.raises(_native.VmpcError) as ei:
        ctx.bn256_qap_colsum(0, cap + 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert ei.value.code == _native.E_RANGE
    # the cap itself is accepted by the argument check (a null pointer is then VMPC_E_INVAL, not a range error)
    with pytest.raises(_native.VmpcError) as ei:
        ctx.bn256_qap_lagrange(0, cap, 0, 0)
    assert ei.value.code == _native.E_INVAL
