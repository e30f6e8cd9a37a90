"""The Pinocchio prover's h on the GPU (verifiable_mpc_amd/pynocchio.py compute_h, csrc/bn256_qap_h.hip): parity with
the reference-made fixture (tests/golden/pinocchio_keygen.json) for both QAP forms, proofs made from the computed h,
random satisfiable R1CS against the naive restatement (tests/h_ref.py), the defining identity h t = V W - Y at random
points at scale, violated witnesses, degenerate inputs, and the primitives through the C ABI.  Every comparison is
exact."""
import random
import types

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import h_ref as H
from tests import keygen_ref as K
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N = K.N
h2i = lambda s: int(s, 16)
ALL_TRUE = {k: True for k in "HVWYZ"}


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


def _deltas(vals):
    return types.SimpleNamespace(v=vals[0], w=vals[1], y=vals[2])


def _case_inputs(case):
    return [h2i(x) for x in case["c"]], _deltas([h2i(x) for x in case["deltas"]])


def _gen(pn, td):
    return pn.Generators(td, pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2))


def _seeded_td(pn, case):
    pn.prng = random.Random(case["seed"])
    try:
        return pn.Trapdoor(N)
    finally:
        pn.prng = random.SystemRandom()


def _enc(pt):
    return None if pt.coords is None else [format(v, "x") for v in pt.coords]


def _r1cs_qap(pn, built):
    V, W, Y, out_ix, m, c = built
    return pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), out_ix, m=m)


def to_ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


# ---- the fixture ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_fixture_parity(pn, fx, form):
    for case in fx:
        qap = _qaps(pn, case)[form]
        c, deltas = _case_inputs(case)
        h = pn.compute_h(qap, c, deltas)
        assert len(h) == case["d"] + 1
        assert h.coeffs == [h2i(x) for x in case["h"]], (case["name"], form)
        a, b, y = (H.row_values(case["r1cs"][k], c) for k in "VWY")
        h0 = pn.compute_h(qap, c)
        assert len(h0) == case["d"] - 1
        assert h0.coeffs == H.naive_h(a, b, y)[0], (case["name"], form)


@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_fixture_proof_from_computed_h(pn, fx, form):
    """generate -> compute_h -> compute_proof equals the fixture's proof point for point and verifies; the same through
    the evalkey dict"""
    for case in fx:
        td = _seeded_td(pn, case)
        qap = _qaps(pn, case)[form]
        gen = _gen(pn, td)
        c, deltas = _case_inputs(case)
        key = pn.PreparedKey.generate(td, qap, gen)
        h = pn.compute_h(qap, c, deltas)
        proof = pn.compute_proof(qap, c, h, key, deltas)
        for k, enc in case["proof"].items():
            assert _enc(proof[k]) == enc, (case["name"], form, k)
        verikey = pn.generate_verikey(td, qap, gen)
        assert pn.verify(qap, verikey, proof, c) == ALL_TRUE
        proof2 = pn.compute_proof(qap, c, pn.compute_h(qap, c, deltas), pn.generate_evalkey(td, qap, gen), deltas)
        assert {k: _enc(p) for k, p in proof2.items()} == dict(case["proof"].items())


# ---- random satisfiable R1CS against the naive restatement --------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_random_r1cs_against_restatement(pn, d):
    built = H.satisfiable_r1cs(d, seed=1000 + d)
    V, W, Y, out_ix, m, c = built
    qap = _r1cs_qap(pn, built)
    a, b, y = (H.csr_row_values(M, c) for M in (V, W, Y))
    rng = random.Random(d)
    dl = tuple(rng.randrange(N) for _ in range(3))
    if d <= 65:
        want0, want1 = H.naive_h(a, b, y)[0], H.naive_h(a, b, y, dl)[0]
    else:       # the naive route is cubic: above 65 the restated formula, itself checked against it on the CPU
        want0, want1 = H.moment_h(a, b), H.moment_h(a, b, dl)
    h0, h1 = pn.compute_h(qap, c), pn.compute_h(qap, c, _deltas(dl))
    assert len(h0) == max(d - 1, 0) and len(h1) == d + 1
    assert h0.coeffs == want0
    assert h1.coeffs == want1
    # the same witness as negative / oversized ints and as a uint8 array
    shifted = [x - N if i % 3 == 0 else x + N * (i % 5) for i, x in enumerate(c)]
    assert pn.compute_h(qap, shifted, _deltas(dl)).coeffs == want1
    assert pn.compute_h(qap, K.to_array(c), _deltas(dl)).coeffs == want1


def test_random_r1cs_small_d_uses_the_naive_route():
    """(the restatement used above 65 is the naive one below: both sides of the split are covered)"""
    a = [3, 5, 7]
    assert H.moment_h(a, a) == H.naive_h(a, a, [x * x % N for x in a])[0]


# ---- scale --------------------------------------------------------------------------------------------------------------

def _scale_circuit(d, seed, n_io=4):
    """V and W read two random input wires each (64-bit values), Y writes output wire j with value 1: satisfiable by
    c[out_j] = a_j b_j.  -> (V, W, Y CSR with int64 values, out_ix, m, witness (m + 1, 32) uint8, a, b, y as ints)"""
    rng = np.random.default_rng(seed)
    m = n_io + 2 * d
    c = [1] + [int(x) for x in rng.integers(1, 1 << 62, size=n_io + d)]
    c = [x * x * x % N for x in c]
    c[0] = 1
    ptr = np.arange(0, 2 * d + 1, 2)
    mats, vals_rows = [], []
    for _ in range(2):
        col = rng.integers(0, n_io + d + 1, size=2 * d)
        vals = rng.integers(-(1 << 62), 1 << 62, size=2 * d).astype(np.int64)
        mats.append((ptr, col, vals))
        cl, vl = col.tolist(), vals.tolist()
        vals_rows.append([(vl[2 * r] * c[cl[2 * r]] + vl[2 * r + 1] * c[cl[2 * r + 1]]) % N for r in range(d)])
    a, b = vals_rows
    y = [ai * bi % N for ai, bi in zip(a, b)]
    Y = (np.arange(d + 1), n_io + d + 1 + np.arange(d), np.ones(d, np.int64))
    c += y
    return mats[0], mats[1], Y, n_io, m, K.to_array(c), a, b, y


def _horner(coeffs, x):
    acc = 0
    for v in reversed(coeffs):
        acc = (acc * x + v) % N
    return acc


def _check_identity(d, a, b, y, h, dl, seed):
    rng = random.Random(seed)
    dv, dw, dy = dl if dl is not None else (0, 0, 0)
    for _ in range(2):
        x0 = rng.randrange(d + 1, N)
        ell, t0 = K.lagrange_at(x0, d)
        V0, W0, Y0 = (sum(v * l for v, l in zip(vals, ell)) % N for vals in (a, b, y))
        h0 = (_horner(h, x0) - dv * W0 - dw * V0 - dv * dw * t0 + dy) % N
        assert h0 * t0 % N == (V0 * W0 - Y0) % N


@pytest.mark.parametrize("log_d,zk", [(14, False), (14, True), (16, False), (16, True), (18, True)])
def test_scale_identity_at_random_points(pn, log_d, zk):
    """h(x0) t(x0) = V(x0) W(x0) - Y(x0) (plus the zero-knowledge terms) at two random x0, with V(x0) from the row values
    and the Lagrange basis - O(d) big-int work that shares nothing with the kernels - and the exact length"""
    d = 1 << log_d
    V, W, Y, out_ix, m, c, a, b, y = _scale_circuit(d, seed=log_d)
    qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
    dl = tuple(random.Random(log_d).randrange(N) for _ in range(3)) if zk else None
    h = pn.compute_h(qap, c, _deltas(dl) if zk else None)
    assert len(h) == (d + 1 if zk else d - 1) and len(h.coeffs) == len(h)
    assert any(h.coeffs)
    _check_identity(d, a, b, y, h.coeffs, dl, seed=log_d)


def test_verified_proof_with_nonzero_h_at_2_14(pn):
    d = 1 << 14
    V, W, Y, out_ix, m, c, a, b, y = _scale_circuit(d, seed=77)
    qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
    r = random.Random(14)
    td = K.TD(*(r.randrange(N) for _ in range(8)))
    gen = _gen(pn, td)
    key = pn.PreparedKey.generate(td, qap, gen)
    dl = _deltas([r.randrange(N) for _ in range(3)])
    h = pn.compute_h(qap, c, dl)
    proof = pn.compute_proof(qap, c, h, key, dl)
    verikey = pn.generate_verikey(td, qap, gen)
    cl = to_ints(c[:out_ix + 1])
    assert pn.verify(qap, verikey, proof, cl) == ALL_TRUE
    assert any(h.coeffs)
    proof2 = pn.compute_proof(qap, c, list(h.coeffs), key, dl)
    assert {k: _enc(p) for k, p in proof2.items()} == {k: _enc(p) for k, p in proof.items()}
    # and a wrong h does not verify
    bad = list(h.coeffs)
    bad[5] = (bad[5] + 1) % N
    assert pn.verify(qap, verikey, pn.compute_proof(qap, c, bad, key, dl), cl)["H"] is False


# ---- violated witnesses -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_violated_witness_raises_at_31(pn, fx, form):
    case = fx[1]
    assert case["d"] == 31
    qap = _qaps(pn, case)[form]
    c, deltas = _case_inputs(case)
    wire = list(qap.indices_mid)[len(qap.indices_mid) // 2]
    c[wire] = (c[wire] + 1) % N
    a, b, y = (H.row_values(case["r1cs"][k], c) for k in "VWY")
    first = min(j for j in range(31) if (a[j] * b[j] - y[j]) % N) + 1
    with pytest.raises(ValueError, match=rf"constraint {first} "):
        pn.compute_h(qap, c, deltas)


def test_violated_witness_raises_at_2_14(pn):
    d = 1 << 14
    V, W, Y, out_ix, m, c, a, b, y = _scale_circuit(d, seed=78)
    qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
    c = c.copy()
    # a mid input wire that a row in the middle of V reads
    wire = next(int(w) for w in V[1][d:] if w > out_ix)
    cv = (to_ints(c[wire:wire + 1])[0] + 1) % N
    c[wire] = np.frombuffer(cv.to_bytes(32, "little"), np.uint8)
    ci = to_ints(c)
    bad = []
    for M in (V, W):
        ptr, col, vals = M
        hit = np.nonzero(col == wire)[0]
        bad += (hit // 2).tolist()
    rows = sorted(set(bad))
    assert rows
    first = None
    for r in rows:
        ar = sum(int(V[2][e]) * ci[V[1][e]] for e in (2 * r, 2 * r + 1)) % N
        br = sum(int(W[2][e]) * ci[W[1][e]] for e in (2 * r, 2 * r + 1)) % N
        if (ar * br - y[r]) % N:
            first = r + 1
            break
    assert first is not None
    with pytest.raises(ValueError, match=rf"constraint {first} "):
        pn.compute_h(qap, c)


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"zero_a": True}, {"zero_b": True}])
def test_zero_rows(pn, kw):
    d = 70
    built = H.satisfiable_r1cs(d, seed=9, **kw)
    V, W, Y, out_ix, m, c = built
    qap = _r1cs_qap(pn, built)
    a, b, y = (H.csr_row_values(M, c) for M in (V, W, Y))
    assert pn.compute_h(qap, c).coeffs == [0] * (d - 1)
    dl = (5, 7, 11)
    assert pn.compute_h(qap, c, _deltas(dl)).coeffs == H.moment_h(a, b, dl) == H.naive_h(a, b, y, dl)[0]


def test_zero_deltas_given_keep_the_length(pn):
    d = 40
    built = H.satisfiable_r1cs(d, seed=10)
    qap = _r1cs_qap(pn, built)
    c = built[5]
    h0 = pn.compute_h(qap, c).coeffs
    hz = pn.compute_h(qap, c, _deltas((0, 0, 0)))
    assert len(hz) == d + 1 and hz.coeffs == h0 + [0, 0]


def test_witness_of_all_n_minus_1(pn):
    """every wire n - 1 (the constant wire included): rows x_j * x_j = 1 * y_j hold, (n-1)^2 = 1 = ... on wire values"""
    d = 66
    # row j: (w_a) * (w_b) = (1/(n-1)) * w_c, i.e. (n-1)(n-1) = (n-1)(n-1)
    ptr = list(range(d + 1))
    rng = random.Random(4)
    V = (ptr, [rng.randrange(0, d + 3) for _ in range(d)], [1] * d)
    W = (ptr, [rng.randrange(0, d + 3) for _ in range(d)], [1] * d)
    Y = (ptr, [rng.randrange(0, d + 3) for _ in range(d)], [N - 1] * d)
    c = [N - 1] * (d + 3)
    qap = pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), 2, m=d + 2)
    a = [N - 1] * d
    y = [1] * d
    dl = (N - 1, N - 1, N - 1)
    assert pn.compute_h(qap, c, _deltas(dl)).coeffs == H.naive_h(a, a, y, dl)[0]
    assert pn.compute_h(qap, c).coeffs == H.naive_h(a, a, y)[0]


def test_d_above_cap_raises(pn):
    from verifiable_mpc_amd import _native as nat
    qap = types.SimpleNamespace(d=nat.BN256_FR_POLY_MAX, indices=range(1))
    with pytest.raises(ValueError, match="cap"):
        pn.compute_h(qap, [1])


# ---- primitives through the C ABI ---------------------------------------------------------------------------------------

def _moments_ref(u, n_out):
    out, run = [], list(u)
    for k in range(n_out):
        out.append(sum(run) % N)
        run = [x * j % N for j, x in enumerate(run, 1)]
    return out


@pytest.mark.parametrize("d,n_out", [(1, 8), (64, 8), (65, 8), (4097, 8), (1 << 18, 8), (300, 300)])
def test_moments_primitive(ctx, d, n_out):
    rng = np.random.default_rng(d)
    rnd = rng.integers(0, 256, size=(d, 32), dtype=np.uint8)          # any 32-byte values: reduced on load
    top = K.to_array([N - 1] * d)
    du, dt = ctx.upload(rnd), ctx.upload(top)
    o0, o1, o2 = ctx.alloc(32 * n_out), ctx.alloc(32 * n_out), ctx.alloc(32 * n_out)
    ctx.bn256_qap_moments(du.ptr, dt.ptr, d, n_out, o0.ptr, o1.ptr)
    ctx.bn256_qap_moments(du.ptr, None, d, n_out, o2.ptr, None)
    ctx.sync()
    want0 = _moments_ref([x % N for x in to_ints(rnd)], n_out)
    assert to_ints(ctx.download(o0.ptr, 32 * n_out)) == want0
    assert to_ints(ctx.download(o2.ptr, 32 * n_out)) == want0
    assert to_ints(ctx.download(o1.ptr, 32 * n_out)) == _moments_ref([N - 1] * d, n_out)


def test_moments_deep_segment(ctx):
    """k far beyond the first segment: a segment's start power j^k0 by square-and-multiply"""
    d, n_out = 700, 1400
    u = [random.Random(6).randrange(N) for _ in range(d)]
    du, out = ctx.upload(K.to_array(u)), ctx.alloc(32 * n_out)
    ctx.bn256_qap_moments(du.ptr, None, d, n_out, out.ptr, None)
    ctx.sync()
    got = to_ints(ctx.download(out.ptr, 32 * n_out))
    for k in (0, 1, 511, 512, 513, 1023, 1024, 1399):
        assert got[k] == sum(x * pow(j, k, N) for j, x in enumerate(u, 1)) % N, k


def _weights(d):
    """w_j = (-1)^(d-j) (j-1)! (d-j)! for j = 1..d: factorials in Python"""
    fact = [1] * (d + 1)
    for k in range(1, d + 1):
        fact[k] = fact[k - 1] * k % N
    return [(-1) ** (d - j) * fact[j - 1] * fact[d - j] % N for j in range(1, d + 1)]


@pytest.mark.parametrize("d", [1, 63, 64, 65, 16383, 16384, 16385, 32769])
def test_weights_at_scan_boundaries(ctx, d):
    """csrc/fr_scan.h over GF(n) with runs of QH_RUN = 64 elements: d = 63, 64, 65 is a run one short of full, full
    and a second lane of one element; 16383 / 16384 give 256 lanes (one per scanning thread, the last run short at
    16383), 16385 gives 257 (two per thread, 127 threads with none, the one that inverts d! among them), 32769 gives 513
    (three per thread, 85 threads with none).  a random, b all n - 1."""
    rng = random.Random(8000 + d)
    a, b = [rng.randrange(N) for _ in range(d)], [N - 1] * d
    da, db = ctx.upload(K.to_array(a)), ctx.upload(K.to_array(b))
    ua, ub = ctx.upload(K.to_array([7] * (d + 1))), ctx.upload(K.to_array([7] * (d + 1)))
    ctx.bn256_qap_h_weights(da.ptr, db.ptr, d, ua.ptr, ub.ptr)
    inv_w = [pow(wj, -1, N) for wj in _weights(d)]
    ctx.sync()
    assert to_ints(ctx.download(ua.ptr, 32 * (d + 1))) == [x * f % N for x, f in zip(a, inv_w)] + [7]
    assert to_ints(ctx.download(ub.ptr, 32 * (d + 1))) == [x * f % N for x, f in zip(b, inv_w)] + [7]


def test_weights_check_and_horner_primitives(ctx):
    d = 130
    rng = random.Random(8)
    a, b = [rng.randrange(N) for _ in range(d)], [rng.randrange(N) for _ in range(d)]
    da, db = ctx.upload(K.to_array(a)), ctx.upload(K.to_array(b))
    ua, ub = ctx.alloc(32 * d), ctx.alloc(32 * d)
    ctx.bn256_qap_h_weights(da.ptr, db.ptr, d, ua.ptr, ub.ptr)
    w = _weights(d)
    ctx.sync()
    assert to_ints(ctx.download(ua.ptr, 32 * d)) == [x * pow(wj, -1, N) % N for x, wj in zip(a, w)]
    assert to_ints(ctx.download(ub.ptr, 32 * d)) == [x * pow(wj, -1, N) % N for x, wj in zip(b, w)]
    y = [x * z % N for x, z in zip(a, b)]
    bad = ctx.alloc(4)
    for spoil in ((), (77,), (100, 12)):
        yy = list(y)
        for i in spoil:
            yy[i] = (yy[i] + 1) % N
        dy = ctx.upload(K.to_array(yy))
        ctx.bn256_qap_check(da.ptr, db.ptr, dy.ptr, d, bad.ptr)
        ctx.sync()
        assert int(ctx.download(bad.ptr, 4).view("<u4")[0]) == (min(spoil) if spoil else 0xFFFFFFFF)
    coeffs = [[rng.randrange(N) for _ in range(9)] for _ in range(3)]
    dc, out = ctx.upload(K.to_array(sum(coeffs, []))), ctx.alloc(32 * 3 * d)
    ctx.bn256_qap_horner(dc.ptr, 9, 3, d, out.ptr)
    ctx.sync()
    assert to_ints(ctx.download(out.ptr, 32 * 3 * d)) == [_horner(p, j) for p in coeffs for j in range(1, d + 1)]


def _t_on_device(ctx, d):
    scratch, out = ctx.alloc(64 * (d + (d + 127) // 128)), ctx.alloc(32 * (d + 1))
    ctx.bn256_qap_t_coeffs(d, scratch.ptr, out.ptr)
    ctx.sync()
    return to_ints(ctx.download(out.ptr, 32 * (d + 1)))


def test_t_coefficients(ctx, fx):
    for case in fx:
        assert _t_on_device(ctx, case["d"]) == [h2i(x) for x in case["qap"]["t"]]
    for d in (1, 128, 129, 300, 1000):
        assert _t_on_device(ctx, d) == H.t_coeffs(d)
    d = 1 << 16
    t = _t_on_device(ctx, d)
    assert len(t) == d + 1 and t[d] == 1
    x0 = random.Random(16).randrange(N)
    want = 1
    for j in range(1, d + 1):
        want = want * (x0 - j) % N
    assert _horner(t, x0) == want


def test_cap_is_range_before_any_pointer(ctx):
    from verifiable_mpc_amd import _native as nat
    d = nat.BN256_FR_POLY_MAX
    calls = [lambda: ctx.bn256_qap_moments(0, 0, d, 8, 0, 0), lambda: ctx.bn256_qap_moments(0, 0, 8, d + 1, 0, 0),
             lambda: ctx.bn256_qap_h_weights(0, 0, d, 0, 0), lambda: ctx.bn256_qap_check(0, 0, 0, d, 0),
             lambda: ctx.bn256_qap_t_coeffs(d, 0, 0), lambda: ctx.bn256_qap_horner(0, 4, 1, d, 0),
             lambda: ctx.bn256_qap_h_combine(0, 0, 0, d, 0, 0, 0)]
    for call in calls:
        with pytest.raises(nat.VmpcError) as ei:
            call()
        assert ei.value.code == nat.E_RANGE
    with pytest.raises(nat.VmpcError) as ei:
        ctx.bn256_qap_moments(0, 0, d - 1, 8, 0, 0)       # at the cap: null pointers are the complaint
    assert ei.value.code == nat.E_INVAL
