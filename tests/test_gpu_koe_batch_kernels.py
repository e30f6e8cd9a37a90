"""The entries behind the batch Protocol 8 prover over BN-256, one at a time through the C ABI, against numpy and Python
integers: vmpc_bn256_koe_stage_batch_dev and vmpc_bn256_koe_split_batch_dev (csrc/bn256_koe.hip), the GF(n)
instantiations vmpc_bn256_fr_cs_triples_batch_dev / vmpc_bn256_fr_cs_extend_batch_dev (csrc/circuit_sat.hip) against
their single forms, and knowledge_of_exponent.opening_linear_form_prover_batch against K single openings.

Shapes: the staging kernel runs 256 lanes a workgroup over n + 1 lanes (n = 255, 256, 257: the gamma lane last of a
workgroup, first of the next, and one further), the split one lane per witness (K = 65: past one wave of 64).  PAT
fills what no kernel may write; it is a word above the order, so no kernel can produce it."""
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import p8_field_ref as fref

pytestmark = pytest.mark.gpu

N = fref.BN_N
F = fref.P8(N)
PAT_BYTE = 0xA5
PAT = int.from_bytes(bytes([PAT_BYTE]) * 32, "little")
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def ctx(vm):
    return vm.get_context()


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _ints(a):
    raw = a.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _pattern(ctx, n):
    return ctx.upload(np.full((max(n, 1), 32), PAT_BYTE, np.uint8))


def _get(ctx, buf, n):
    ctx.sync()
    return _ints(ctx.download(buf.ptr, 32 * n))


def _rows(rng, K, n, stride):
    """K rows of n scalars, `stride` apart, PAT between them -> (flat image, rows as residues).  Values: random
    residues, the largest one, and a word above the order (reduced when a kernel loads it)."""
    image, rows = [PAT] * (K * stride), []
    for p in range(K):
        raw = [rng.choice([rng.randrange(N), N - 1, rng.randrange(1 << 200) + N]) for _ in range(n)]
        image[p * stride:p * stride + n] = raw
        rows.append([v % N for v in raw])
    return image, rows


def test_pat_is_not_a_residue():
    assert N <= PAT < 1 << 256 and 2 * N > 1 << 256


# ---- koe_stage_batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("K", [1, 3])
def test_stage_batch(ctx, K, n):
    rng = random.Random(100 * n + K)
    xs, Ls, ls, rs = n + 3, n + 2, n + 5, n + 4             # strides above the rows
    x_img, x = _rows(rng, K, n, xs)
    L_img, L = _rows(rng, K, n, Ls)
    gammas = [rng.choice([rng.randrange(N), N - 1]) for _ in range(K)]
    d_x, d_L, d_g = ctx.upload(_bytes(x_img)), ctx.upload(_bytes(L_img)), ctx.upload(_bytes(gammas))
    want_lhs, want_rhs = [PAT] * (K * ls + 1), [PAT] * (K * rs + 1)
    for p in range(K):
        want_lhs[p * ls:p * ls + n + 1] = [gammas[p]] + x[p]
        want_rhs[p * rs:p * rs + n] = L[p][::-1]
    # both sides in one launch
    lhs, rhs = _pattern(ctx, K * ls + 1), _pattern(ctx, K * rs + 1)
    ctx.bn256_koe_stage_batch(d_x.ptr, xs, d_g.ptr, d_L.ptr, Ls, n, K, lhs.ptr, ls, rhs.ptr, rs)
    assert _get(ctx, lhs, K * ls + 1) == want_lhs
    assert _get(ctx, rhs, K * rs + 1) == want_rhs
    # x NULL: lhs (and the gammas) are not looked at; L NULL: rhs is not
    lhs, rhs = _pattern(ctx, K * ls + 1), _pattern(ctx, K * rs + 1)
    ctx.bn256_koe_stage_batch(None, xs, None, d_L.ptr, Ls, n, K, lhs.ptr, ls, rhs.ptr, rs)
    assert _get(ctx, lhs, K * ls + 1) == [PAT] * (K * ls + 1)
    assert _get(ctx, rhs, K * rs + 1) == want_rhs
    lhs, rhs = _pattern(ctx, K * ls + 1), _pattern(ctx, K * rs + 1)
    ctx.bn256_koe_stage_batch(d_x.ptr, xs, d_g.ptr, None, Ls, n, K, lhs.ptr, ls, None, rs)
    assert _get(ctx, lhs, K * ls + 1) == want_lhs
    assert _get(ctx, rhs, K * rs + 1) == [PAT] * (K * rs + 1)
    # every row is the single entry's
    for p in range(K):
        l1, r1 = _pattern(ctx, n + 2), _pattern(ctx, n + 1)
        ctx.bn256_koe_stage(d_x.ptr + 32 * p * xs, gammas[p], d_L.ptr + 32 * p * Ls, n, l1.ptr, r1.ptr)
        assert _get(ctx, l1, n + 2) == want_lhs[p * ls:p * ls + n + 1] + [PAT]
        assert _get(ctx, r1, n + 1) == want_rhs[p * rs:p * rs + n] + [PAT]
    # no witnesses: no launch
    lhs = _pattern(ctx, ls)
    ctx.bn256_koe_stage_batch(d_x.ptr, xs, d_g.ptr, None, Ls, n, 0, lhs.ptr, ls, None, rs)
    assert _get(ctx, lhs, ls) == [PAT] * ls


def test_stage_and_split_batch_range_errors(vm, ctx):
    nat = vm._native
    n, K = 4, 2
    buf = _pattern(ctx, 64)
    ok = dict(x=buf.ptr, xs=n, g=buf.ptr, L=buf.ptr, Ls=n, n=n, K=K, lhs=buf.ptr, ls=n + 1, rhs=buf.ptr, rs=n)

    def stage(**kw):
        a = {**ok, **kw}
        return ctx.bn256_koe_stage_batch(a["x"], a["xs"], a["g"], a["L"], a["Ls"], a["n"], a["K"], a["lhs"], a["ls"], a["rhs"],
                                         a["rs"])
    bad = [dict(ls=n), dict(xs=n - 1), dict(Ls=n - 1), dict(rs=n - 1), dict(xs=(1 << 31) + 1), dict(Ls=(1 << 31) + 1),
           dict(ls=(1 << 31) + 1), dict(rs=(1 << 31) + 1), dict(K=nat.BN256_QAP_MAX_WIT + 1),
           dict(n=nat.BN256_FR_POLY_MAX, xs=1 << 30, Ls=1 << 30, ls=1 << 30, rs=1 << 30)]
    for kw in bad:
        for ptrs in ({}, dict(x=None, L=None, lhs=None, rhs=None, g=None)):        # before any pointer is looked at
            with pytest.raises(nat.VmpcError) as ei:
                stage(**kw, **ptrs)
            assert ei.value.code == nat.E_RANGE, kw
    for kw in (dict(x=None, L=None), dict(lhs=None), dict(g=None), dict(rhs=None)):
        with pytest.raises(nat.VmpcError) as ei:
            stage(**kw)
        assert ei.value.code == nat.E_INVAL, kw
    for c_stride, n_, K_ in ((2 * n - 1, n, K), ((1 << 31) + 1, n, K), (2 * n, n, nat.BN256_QAP_MAX_WIT + 1),
                             (1 << 30, nat.BN256_FR_POLY_MAX, K)):
        with pytest.raises(nat.VmpcError) as ei:
            ctx.bn256_koe_split_batch(None, c_stride, n_, K_, None)
        assert ei.value.code == nat.E_RANGE
    with pytest.raises(nat.VmpcError) as ei:
        ctx.bn256_koe_split_batch(buf.ptr, 8, 0, K, buf.ptr)
    assert ei.value.code == nat.E_INVAL
    assert _get(ctx, buf, 64) == [PAT] * 64


# ---- koe_split_batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("K", [1, 65])
def test_split_batch(ctx, K, n):
    rng = random.Random(300 * n + K)
    stride = 2 * n + 3
    image, rows = _rows(rng, K, 2 * n, stride)
    c, u = ctx.upload(_bytes(image + [PAT])), _pattern(ctx, K + 1)
    ctx.bn256_koe_split_batch(c.ptr, stride, n, K, u.ptr)
    assert _get(ctx, u, K + 1) == [row[n] for row in rows] + [PAT]
    want = list(image) + [PAT]
    for p in range(K):
        want[p * stride + n] = 0
    assert _get(ctx, c, K * stride + 1) == want           # only the coefficient n of each row has changed
    ctx.bn256_koe_split_batch(c.ptr, stride, n, 0, u.ptr)
    assert _get(ctx, c, K * stride + 1) == want


# ---- the GF(n) batch entries of Protocol 8 against the single ones -----------------------------------------------------------
N_X, K_WIT = 5, 3


def _p8_case(vm, m):
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    rng = random.Random(7000 + m)
    A, B, _ = F.random_circuit(rng, N_X, m, 0)
    sc = cs.SparseCircuit(N_X, fref.to_csr(A), fref.to_csr(B), order=N)
    xs = [[rng.randrange(N) for _ in range(N_X - 1)] + [N - 1] for _ in range(K_WIT)]
    rs = [(rng.randrange(1, N), rng.randrange(1, N)) for _ in range(K_WIT)]
    return sc, A, B, xs, rs


def _single_z(ctx, sc, x, r, m, mode, vm):
    """z of one witness by the single GF(n) entries: (z, a, b) as ints"""
    d = sc.device()
    M, n_z, g_off = m + 1, N_X + 3 + 2 * m, N_X + 3
    z = ctx.upload(_bytes(x + [PAT] * (n_z - N_X)))
    a, b = ctx.upload(_bytes([PAT] * m + [r[0]])), ctx.upload(_bytes([PAT] * m + [r[1]]))
    for lv in range(len(sc.level_ptr) - 1):
        lo, hi = int(sc.level_ptr[lv]), int(sc.level_ptr[lv + 1])
        ctx.cs_triples(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, N_X, g_off, z.ptr, a.ptr, b.ptr, bn=True)
    with vm.device.cs_extension(mode):
        ctx.cs_extend(a.ptr, b.ptr, m, d["fact"].ptr, d["ifact"].ptr, z.ptr + 32 * N_X, bn=True)
    return _get(ctx, z, n_z), _get(ctx, a, M), _get(ctx, b, M)


@pytest.mark.parametrize("mode", ["direct", "ntt"])
@pytest.mark.parametrize("m", [0, 1, 2, 65])
def test_bn_triples_and_extend_batch_rows_are_the_single_entries(vm, ctx, m, mode):
    nat = vm._native
    sc, A, B, xs, rs = _p8_case(vm, m)
    d = sc.device()
    K, M, n_z, g_off = K_WIT, m + 1, N_X + 3 + 2 * m, N_X + 3
    zs, abs_ = n_z + 2, M + 3                               # strides above the rows
    z_img, a_img, b_img = [PAT] * (K * zs + 1), [PAT] * (K * abs_ + 1), [PAT] * (K * abs_ + 1)
    for p in range(K):
        z_img[p * zs:p * zs + N_X] = xs[p]
        a_img[p * abs_ + m], b_img[p * abs_ + m] = rs[p]
    Z, a, b = ctx.upload(_bytes(z_img)), ctx.upload(_bytes(a_img)), ctx.upload(_bytes(b_img))
    for lv in range(len(sc.level_ptr) - 1):
        lo, hi = int(sc.level_ptr[lv]), int(sc.level_ptr[lv + 1])
        ctx.cs_triples_batch(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, N_X, g_off, Z.ptr, zs, a.ptr,
                             b.ptr, abs_, K, bn=True)
    lib = nat.load_library()
    assert lib.vmpc_bn256_fr_cs_extend_batch_bytes(m, K) == lib.vmpc_fr_cs_extend_batch_bytes(m, K) > 0
    with vm.device.cs_extension(mode):
        need = ctx.cs_extend_batch_bytes(m, K, bn=True)
        assert need > 0 and need == ctx.cs_extend_batch_bytes(m, K)
        for attempt in range(2):                            # the second call finds the arena the first one left
            before = ctx.debug_arena_info()
            ctx.cs_extend_batch(a.ptr, b.ptr, abs_, m, d["fact"].ptr, d["ifact"].ptr, Z.ptr + 32 * N_X, zs, K, bn=True)
            ctx.sync()
            size, used, gen = ctx.debug_arena_info()
            assert 0 < used <= need <= size, (used, need, size)
        assert gen == before[2] and size == before[0], "the arena grew during a call it was large enough for"
    got_z, got_a, got_b = _get(ctx, Z, K * zs + 1), _get(ctx, a, K * abs_ + 1), _get(ctx, b, K * abs_ + 1)
    for p in range(K):
        z1, a1, b1 = _single_z(ctx, sc, xs[p], rs[p], m, mode, vm)
        assert got_z[p * zs:p * zs + n_z] == z1 and PAT not in z1, p
        assert z1[g_off:g_off + m] == F.triples(N_X, A, B, xs[p])[2], p
        assert got_a[p * abs_:p * abs_ + M] == a1 and got_b[p * abs_:p * abs_ + M] == b1, p
        assert got_z[p * zs + n_z:(p + 1) * zs] == [PAT] * (zs - n_z), p
        gap = [PAT] * (abs_ - M)
        assert got_a[p * abs_ + M:(p + 1) * abs_] == gap and got_b[p * abs_ + M:(p + 1) * abs_] == gap, p
    assert got_z[K * zs] == PAT and got_a[K * abs_] == PAT
    if mode == "ntt" or m == 0:
        return
    # check = 1: every witness names ITS smallest bad gate, and z stays the caller's
    spoil = {1: [m - 1], 2: [m - 1, m // 2]}
    image = list(got_z)
    for p, gates in spoil.items():
        for i in gates:
            image[p * zs + g_off + i] = (image[p * zs + g_off + i] + 1) % N
    Z2, bad = ctx.upload(_bytes(image)), ctx.upload(np.full(K, 7, np.uint32))
    ctx.cs_triples_batch(d["A"].csr(), d["B"].csr(), None, m, N_X, g_off, Z2.ptr, zs, a.ptr, b.ptr, abs_, K, 1, bad.ptr,
                         bn=True)
    ctx.sync()
    assert ctx.download(bad.ptr, 4 * K).view(np.uint32).tolist() == [NONE, m - 1, min(m - 1, m // 2)]
    assert _get(ctx, Z2, K * zs + 1) == image
    with pytest.raises(nat.VmpcError) as ei:
        ctx.cs_triples_batch(d["A"].csr(), d["B"].csr(), None, m, N_X, g_off, Z2.ptr, g_off + m - 1, a.ptr, b.ptr, abs_, K,
                             bn=True)
    assert ei.value.code == nat.E_RANGE
    with pytest.raises(nat.VmpcError) as ei:
        ctx.cs_extend_batch(a.ptr, b.ptr, m, m, d["fact"].ptr, d["ifact"].ptr, Z.ptr, zs, K, bn=True)
    assert ei.value.code == nat.E_RANGE


# ---- opening_linear_form_prover_batch alone ------------------------------------------------------------------------------------
class Replay:
    def __init__(self, draws):
        self.draws = list(draws)

    def randrange(self, *args):
        return self.draws.pop(0)


@pytest.fixture(scope="module")
def openings(vm):
    """n = 5, K = 3: pp, inputs, forms (the second with all-zero coefficients), gammas and the three single openings"""
    koe = vm.knowledge_of_exponent
    n, K = 5, 3
    rng = random.Random(515)
    saved = koe.prng
    koe.prng = Replay([rng.randrange(1, N), rng.randrange(N), rng.randrange(N)])
    try:
        pp = koe.trusted_setup(vm.pynocchio.BN256Point(bn.G1), vm.pynocchio.BN256TwistPoint(bn.G2), n, N)
    finally:
        koe.prng = saved
    gf = vm.GF(N)
    xs = [[rng.randrange(N) for _ in range(n)] for _ in range(K)]
    coeffs = [[rng.randrange(N) for _ in range(n)], [0] * n, [N - 1] * n]
    consts = [rng.randrange(N) for _ in range(K)]
    gammas = [rng.randrange(1, N) for _ in range(K)]
    Vec = vm.device.BnScalarVector
    X = Vec.from_ints([v for x in xs for v in x])
    Ls = [vm.pivot.AffineForm(Vec.from_ints(co), gf(k)) for co, k in zip(coeffs, consts)]
    singles = [koe.opening_linear_form_prover(L, X[p * n:(p + 1) * n], g, pp) for p, (L, g) in enumerate(zip(Ls, gammas))]
    return dict(n=n, K=K, pp=pp, gf=gf, xs=xs, coeffs=coeffs, consts=consts, gammas=gammas, X=X, Ls=Ls, singles=singles)


def _same_openings(got, want):
    assert len(got) == len(want)
    for p, ((gp, gu), (wp, wu)) in enumerate(zip(got, want)):
        assert list(gp) == list(wp) == ["P", "pi", "Q"], p
        assert (gp["Q"].coords is None) == (wp["Q"].coords is None), p
        for k in ("P", "pi", "Q"):
            assert type(gp[k]) is type(wp[k]) and gp[k].coords == wp[k].coords, (p, k)
            if wp[k].coords is not None:
                assert gp[k].to_bytes() == wp[k].to_bytes(), (p, k)
        assert type(gu) is type(wu) and int(gu) == int(wu), p


def test_opening_batch_equals_single_openings(vm, openings):
    o, koe = openings, vm.knowledge_of_exponent
    n, K = o["n"], o["K"]
    # the yardstick itself: u = L(x), and the all-zero form opens to its constant with Q at infinity
    for p, (proof, u) in enumerate(o["singles"]):
        assert int(u) == (sum(a * b for a, b in zip(o["coeffs"][p], o["xs"][p])) + o["consts"][p]) % N
    assert o["singles"][1][0]["Q"].coords is None and int(o["singles"][1][1]) == o["consts"][1]
    got = koe.opening_linear_form_prover_batch(o["Ls"], o["X"], o["gammas"], o["pp"])
    _same_openings(got, o["singles"])
    assert got[1][0]["Q"].coords is None and int(got[1][1]) == o["consts"][1]
    # rows further apart than their length
    wide = vm.device.BnScalarVector.from_ints([v for x in o["xs"] for v in x + [PAT % N, 1]])
    _same_openings(koe.opening_linear_form_prover_batch(o["Ls"], wide, o["gammas"], o["pp"], stride=n + 2, n=n), o["singles"])
    # the commitment first, its staged rows handed on
    pairs, lhs = koe.restriction_argument_prover_batch(o["X"], o["gammas"], o["pp"], return_lhs=True)
    assert [(P.to_bytes(), pi.to_bytes()) for P, pi in pairs] == \
        [(s[0]["P"].to_bytes(), s[0]["pi"].to_bytes()) for s in o["singles"]]
    assert [(P.to_bytes(), pi.to_bytes()) for P, pi in koe.restriction_argument_prover_batch(o["xs"], o["gammas"], o["pp"])] \
        == [(P.to_bytes(), pi.to_bytes()) for P, pi in pairs]
    got = koe.opening_linear_form_prover_batch(o["Ls"], None, o["gammas"], o["pp"], [P for P, _ in pairs],
                                               [pi for _, pi in pairs], lhs=lhs)
    _same_openings(got, o["singles"])
    assert koe.opening_linear_form_prover_batch([], o["X"][:0], [], o["pp"]) == []


def test_opening_batch_from_host_lists_and_a_pp_of_lists(vm, openings):
    o, koe = openings, vm.knowledge_of_exponent
    gf = o["gf"]
    host_Ls = [vm.pivot.AffineForm([gf(v) for v in co], gf(k)) for co, k in zip(o["coeffs"], o["consts"])]
    host_singles = [koe.opening_linear_form_prover(L, x, g, o["pp"]) for L, x, g in zip(host_Ls, o["xs"], o["gammas"])]
    _same_openings(host_singles, o["singles"])
    _same_openings(koe.opening_linear_form_prover_batch(host_Ls, o["xs"], o["gammas"], o["pp"]), host_singles)
    int_Ls = [vm.pivot.AffineForm(list(co), k) for co, k in zip(o["coeffs"], o["consts"])]
    int_singles = [koe.opening_linear_form_prover(L, x, g, o["pp"]) for L, x, g in zip(int_Ls, o["xs"], o["gammas"])]
    _same_openings(koe.opening_linear_form_prover_batch(int_Ls, o["xs"], o["gammas"], o["pp"]), int_singles)
    # a pp given as lists has no table: msm_rows runs its sums row by row
    listed = {"pp_lhs": list(o["pp"]["pp_lhs"]), "pp_rhs": list(o["pp"]["pp_rhs"])}
    _same_openings(koe.opening_linear_form_prover_batch(o["Ls"], o["X"], o["gammas"], listed), o["singles"])


def test_opening_batch_chunks(vm, openings, monkeypatch):
    o, koe = openings, vm.knowledge_of_exponent
    monkeypatch.setattr(koe, "PROVE_BATCH_BUDGET_BYTES", koe.prove_batch_bytes(o["n"], 2))
    assert koe.prove_chunk_size(o["n"], o["K"]) == 2
    _same_openings(koe.opening_linear_form_prover_batch(o["Ls"], o["X"], o["gammas"], o["pp"]), o["singles"])
    monkeypatch.setattr(koe, "PROVE_BATCH_BUDGET_BYTES", 32 * (o["n"] + 1))
    pairs = koe.restriction_argument_prover_batch(o["X"], o["gammas"], o["pp"])
    assert [P.to_bytes() for P, _ in pairs] == [s[0]["P"].to_bytes() for s in o["singles"]]
