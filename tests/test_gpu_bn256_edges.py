"""Edges of the BN-256 MSMs (csrc/bn256.hip, bn256_impl.h), of vmpc_bn256_lincomb_batch_dev and of whole Pinocchio
proofs at size, against oracle/bn256_ref.py.  Every check is exact group-element equality through the exponent
identity: points e_i G with known e_i, so that sum s_i (e_i G) = ((sum s_i e_i) mod N) G, the right-hand side by the
oracle's E.mul.  Points too many for the oracle to walk are made on the device by bn256_fixed_base (pinned by
test_gpu_bn256.py::test_fixed_base_batch_matches_oracle); 16 columns of every such vector are checked against the
oracle as well.  The scalar constructions and the planner facts they rely on are in tests/bn256_msm_inputs.py and are
checked on the CPU by tests/test_bn256_msm_inputs.py.

Covered: every window width c = 4 .. 16 on the variable-base path and each planner-chosen width at its natural size;
the extreme buckets of the c = 16 tables (padding columns, prefixes, the multi-key pass); skewed scalar vectors at
n = 2^16 whose heavy buckets take gk_finish's workgroup tree; coincidences (P + P, P - P) after the bucket stage in
both gk_reduce forms and in the window recombination; the lincomb batch kernel; the eight compute_proof elements at
n = 2^16 and 2^18, and the dict path at n = 2^12.

27 tests, 34 s on an MI355X (most of it the oracle's Python arithmetic).  Each of these value-only mutations of the
library makes some of them fail: gk_finish's LDS tree starting at stride MSM_BLOCK / 4 (14 tests), k_bnp_lincomb's
bit loop starting at 254 (the two lincomb tests), jac_add answering P + P with the point at infinity (19 tests)."""
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import bn256_msm_inputs as mi
from tests.test_gpu_bn256 import walk_points

pytestmark = pytest.mark.gpu
N = bn.N
GROUPS = {1: (bn.E1, bn.G1, bn.g1_to_bytes, bn.g1_from_bytes, 64),
          2: (bn.E2, bn.G2, bn.g2_to_bytes, bn.g2_from_bytes, 128)}


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as v
    return v.get_context()


def arr32(vals):
    from verifiable_mpc_amd import _native
    return _native.ints_to_array([int(v) for v in vals], 32)


def ints(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint8).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def dot(sc, ex):
    return sum(a * b for a, b in zip(sc, ex)) % N


class Oracle:
    """E.mul(k, G) per group, remembered: many checks share a value"""

    def __init__(self):
        self.memo = {}

    def __call__(self, grp, k):
        k %= N
        if (grp, k) not in self.memo:
            E, G = GROUPS[grp][:2]
            self.memo[(grp, k)] = E.mul(k, G)
        return self.memo[(grp, k)]


@pytest.fixture(scope="module")
def mul():
    return Oracle()


def device_points(ctx, grp, exps, rng, mul):
    """e_i G for a list of ints, made on the device; 16 of its columns compared with the oracle"""
    _, G, to_b, from_b, width = GROUPS[grp]
    n = len(exps)
    dg, de = ctx.upload(np.frombuffer(to_b(G), np.uint8)), ctx.upload(arr32(exps))
    dp = ctx.alloc(width * n)
    ctx.bn256_fixed_base(grp, dg.ptr, de.ptr, n, dp.ptr)
    check_columns(ctx, grp, dp, exps, rng, mul)
    return dp


def check_columns(ctx, grp, buf, exps, rng, mul):
    _, _, _, from_b, width = GROUPS[grp]
    n = len(exps)
    cols = sorted({0, n - 1} | {rng.randrange(n) for _ in range(14)})
    while len(cols) < min(16, n):
        cols = sorted(set(cols) | {rng.randrange(n)})
    ctx.sync()
    for i in cols:
        got = from_b(ctx.download(buf.ptr + width * i, width).tobytes())
        assert got == mul(grp, exps[i]), ("device-made column", i)


def host_points(grp, pts):
    to_b, width = GROUPS[grp][2], GROUPS[grp][4]
    return np.frombuffer(b"".join(to_b(p) for p in pts), np.uint8).reshape(len(pts), width)


def var_msm(ctx, grp, sc, dp, n, window=0):
    width = GROUPS[grp][4]
    ds, out = ctx.upload(sc if isinstance(sc, np.ndarray) else arr32(sc)), ctx.alloc(width)
    ctx.set_window(window)
    try:
        ctx.bn256_msm(grp, ds.ptr, dp.ptr, n, out.ptr)
        ctx.sync()
    finally:
        ctx.set_window(0)
    return ctx.download(out.ptr, width).tobytes()


def table_msm(ctx, grp, table, tn, ds, m):
    """(affine bytes, Jacobian bytes) of one single-key table pass"""
    width = GROUPS[grp][4]
    out, jac = ctx.alloc(width), ctx.alloc(3 * width // 2)
    ctx.bn256_table_msm(grp, table.ptr, tn, ds.ptr, m, out.ptr, jac.ptr)
    ctx.sync()
    return ctx.download(out.ptr, width).tobytes(), ctx.download(jac.ptr, 3 * width // 2).tobytes()


def multi_msm(ctx, grp, tables, tn, ds, m):
    jw = 3 * GROUPS[grp][4] // 2
    out = ctx.alloc(jw * len(tables))
    ctx.bn256_table_msm_multi(grp, [t.ptr for t in tables], tn, ds.ptr, m, out.ptr)
    ctx.sync()
    raw = ctx.download(out.ptr, jw * len(tables)).tobytes()
    return [raw[jw * k:jw * (k + 1)] for k in range(len(tables))]


def assert_jac(grp, raw, want, what):
    """Jacobian output: Z = 0 exactly for the point at infinity, otherwise the oracle's affine point"""
    from verifiable_mpc_amd import pynocchio as pn
    to_b, width = GROUPS[grp][2], GROUPS[grp][4]
    z_zero = not any(raw[width:])
    assert z_zero == (want is None), what
    assert pn._from_jacobian(grp, raw).to_bytes() == to_b(want), what


# ---- a. every window width --------------------------------------------------------------------------------------

@pytest.mark.parametrize("grp", [1, 2])
def test_every_window_width(ctx, mul, grp):
    """vmpc_ctx_set_window(c) for c = 4 .. 16 (4 runs as (5, 52)) over 300 distinct points; the scalars reach the
    last bucket of every window (E_c), the largest top digit (N - 1) and the bucket boundaries 2^(c-1) +- 1"""
    E, G, to_b, _, width = GROUPS[grp]
    rng = random.Random(700 + grp)
    exps, pts = walk_points(E, G, rng, 300)
    dp = ctx.upload(host_points(grp, pts))
    for c in range(4, 17):
        cc = mi.make_plan(300, c)[0]
        sc = mi.width_edge_scalars(cc, rng, 300)
        assert var_msm(ctx, grp, sc, dp, 300, window=c) == to_b(mul(grp, dot(sc, exps))), c


@pytest.mark.parametrize("grp", [1, 2])
@pytest.mark.parametrize("logn,c", [(11, 9), (14, 11), (15, 12), (16, 13), (19, 15)])
def test_planner_width_at_natural_size(ctx, mul, grp, logn, c):
    n = 1 << logn
    assert mi.make_plan(n)[0] == c
    to_b = GROUPS[grp][2]
    rng = random.Random(31 * logn + grp)
    exps = [rng.randrange(1, N) for _ in range(n)]
    dp = device_points(ctx, grp, exps, rng, mul)
    sc = mi.width_edge_scalars(c, rng, n)
    assert var_msm(ctx, grp, sc, dp, n) == to_b(mul(grp, dot(sc, exps)))


# ---- b. extreme buckets on the table path -----------------------------------------------------------------------

@pytest.mark.parametrize("grp", [1, 2])
@pytest.mark.parametrize("tn", [297, 303])
def test_table_extreme_buckets(ctx, mul, grp, tn):
    """c = 16 with 17 rows: E_16 (every row but the top one in the last bucket) and N - 1 in every column, then
    mixed; table_n = 1, 7 (mod 8) leaves padding columns in the stride; whole vector and a prefix m < table_n; the
    single-key pass (affine and Jacobian out) and the multi-key pass over two tables"""
    E, G, to_b, _, width = GROUPS[grp]
    rng = random.Random(tn * 3 + grp)
    keys = [walk_points(E, G, rng, tn) for _ in range(2)]
    dps = [ctx.upload(host_points(grp, pts)) for _, pts in keys]
    tables = [ctx.bn256_table_build(grp, dp.ptr, tn) for dp in dps]
    e16 = mi.extreme(16)
    mixed = [e16, N - 1, 0, 1, (1 << 15) - 1, 1 << 15, (1 << 15) + 1] * 8
    mixed += [rng.randrange(N) for _ in range(tn - len(mixed))]
    for name, sc in (("E_16", [e16] * tn), ("N-1", [N - 1] * tn), ("mixed", mixed)):
        ds = ctx.upload(arr32(sc))
        for m in (tn, tn - 5):
            wants = [mul(grp, dot(sc[:m], exps[:m])) for exps, _ in keys]
            aff, jac = table_msm(ctx, grp, tables[0], tn, ds, m)
            assert aff == to_b(wants[0]), (name, m)
            assert_jac(grp, jac, wants[0], (name, m))
            for k, raw in enumerate(multi_msm(ctx, grp, tables, tn, ds, m)):
                assert_jac(grp, raw, wants[k], (name, m, k))


# ---- c. skewed distributions at size ----------------------------------------------------------------------------

@pytest.mark.parametrize("grp", [1, 2])
def test_skewed_scalars_at_size(ctx, mul, grp):
    """n = 2^16 on the variable-base path (c = 13), the table path and the six-key pass.  Point vectors: distinct
    points (device-made), one point repeated in every column (equal partial sums meet in gk_finish's tree), P and -P
    alternating (heavy cases sum to the point at infinity: all-zero bytes, Z = 0), and a distinct vector with
    infinity columns in the six-key pass.  Scalar vectors: tests/bn256_msm_inputs.skewed_vectors."""
    E, G, to_b, _, width = GROUPS[grp]
    n = 1 << 16
    c = mi.make_plan(n)[0]
    rng = random.Random(90 + grp)
    ex_d = [rng.randrange(1, N) for _ in range(n)]
    ex_d2 = [rng.randrange(1, N) for _ in range(n)]
    d, d2 = device_points(ctx, grp, ex_d, rng, mul), device_points(ctx, grp, ex_d2, rng, mul)
    q, p = rng.randrange(1, N), rng.randrange(1, N)
    r = ctx.upload(np.tile(np.frombuffer(to_b(mul(grp, q)), np.uint8), n))
    a = ctx.upload(np.tile(np.frombuffer(to_b(mul(grp, p)) + to_b(E.neg(mul(grp, p))), np.uint8), n // 2))
    holes = [0, 1, n // 2, n - 3, n - 2, n - 1]
    dh = ctx.alloc(width * n)
    ctx.copy(dh.ptr, d2.ptr, width * n)
    for i in holes:
        ctx.upload_into(dh.ptr + width * i, np.zeros(width, np.uint8))
    ex_dh = list(ex_d2)
    for i in holes:
        ex_dh[i] = 0
    vecs = {"distinct": (d, ex_d), "repeated_point": (r, [q] * n), "alternating_point": (a, [p, N - p] * (n // 2)),
            "distinct_holes": (dh, ex_dh)}
    tables = {k: ctx.bn256_table_build(grp, v[0].ptr, n) for k, v in vecs.items()}
    multi = ["distinct", "repeated_point", "alternating_point", "distinct_holes", "repeated_point", "distinct"]
    var_sc = mi.skewed_vectors(n, c, 40 + grp)
    tab_sc = dict(var_sc, extreme=[mi.extreme(16)] * n)
    for sname in var_sc:
        for path, scs in (("var", var_sc), ("table", tab_sc)):
            sc = scs[sname]
            wants = {k: mul(grp, dot(sc, ex)) for k, (_, ex) in vecs.items()}
            if sname in mi.HEAVY:
                assert wants["alternating_point"] is None
            if path == "var":
                for k in ("distinct", "repeated_point", "alternating_point"):
                    assert var_msm(ctx, grp, sc, vecs[k][0], n) == to_b(wants[k]), (sname, k)
                continue
            ds = ctx.upload(arr32(sc))
            for k in ("distinct", "repeated_point", "alternating_point"):
                aff, jac = table_msm(ctx, grp, tables[k], n, ds, n)
                assert aff == to_b(wants[k]), (sname, "table", k)
                assert_jac(grp, jac, wants[k], (sname, "table", k))
            for k, raw in zip(multi, multi_msm(ctx, grp, [tables[k] for k in multi], n, ds, n)):
                assert_jac(grp, raw, wants[k], (sname, "multi", k))


# ---- d. coincidences after the bucket stage ---------------------------------------------------------------------

def coincidence_cases(E, P, c):
    """(points, scalars, expected multiple of P or None): window 1's sum doubled c times equals window 0's sum; the
    same with the opposite point; the reduction's running sum meets an equal / opposite bucket"""
    Pc = E.mul(1 << c, P)
    return [([P, Pc], [1 << c, 1], E.mul(1 << (c + 1), P)),
            ([P, E.neg(Pc)], [1 << c, 1], None),
            ([P, P], [2, 1], E.mul(3, P)),
            ([P, E.neg(P)], [2, 1], P)]


@pytest.mark.parametrize("grp", [1, 2])
def test_coincidences_after_buckets(ctx, grp):
    """the jac_add branches for equal and opposite operands in gk_reduce (both forms), gk_finish and gk_final:
    variable-base at c = 5, 8, 13 (SPLIT = 1), 11 (SPLIT = 2) and 16; the c = 16 table (single key: SPLIT = 2; two keys:
    SPLIT = 1), where the first case also makes the bucket stage add a point to itself"""
    E, G, to_b, _, width = GROUPS[grp]
    P = E.mul(random.Random(5 + grp).randrange(1, N), G)
    for c in (4, 8, 11, 13, 16):
        cc = mi.make_plan(2, c)[0]
        for pts, sc, want in coincidence_cases(E, P, cc):
            dp = ctx.upload(host_points(grp, pts))
            assert var_msm(ctx, grp, sc, dp, len(pts), window=c) == to_b(want), (c, sc)
    assert mi.reduce_split(16, 1) == 2 and mi.reduce_split(16, 1, K=2) == 1
    for pts, sc, want in coincidence_cases(E, P, 16):
        dp = ctx.upload(host_points(grp, pts))
        table = ctx.bn256_table_build(grp, dp.ptr, len(pts))
        ds = ctx.upload(arr32(sc))
        aff, jac = table_msm(ctx, grp, table, len(pts), ds, len(pts))
        assert aff == to_b(want), sc
        assert_jac(grp, jac, want, sc)
        for raw in multi_msm(ctx, grp, [table, table], len(pts), ds, len(pts)):
            assert_jac(grp, raw, want, ("multi", sc))


# ---- e. the lincomb batch kernel --------------------------------------------------------------------------------

@pytest.mark.parametrize("grp", [1, 2])
def test_lincomb_batch_against_oracle(ctx, mul, grp):
    """vmpc_bn256_lincomb_batch_dev: out[b] = +-(sum_i s[b][i] bases[i] + sum_j rows[b][j]) for batch sizes across
    the 64-lane block, 0 / 1 / 3 / 16 bases, 0 / 1 / 2 row points, negate on and off.  Scalars 0, N - 1 (bit 255),
    2^256 - 1 (not reduced by the kernel) and uniform; bases with the point at infinity, a repeated base (P + P in the
    Straus chain) and P, -P under equal scalars; lanes whose rows cancel the sum to infinity (all-zero bytes)."""
    E, G, to_b, _, width = GROUPS[grp]
    rng = random.Random(60 + grp)
    bexp = [rng.randrange(1, N) for _ in range(16)]
    bexp[1] = 0                                  # the point at infinity
    bexp[2] = bexp[0]                            # a repeated base
    bexp[4] = (N - bexp[3]) % N                  # P and -P (equal scalars below)
    bases = [mul(grp, e) for e in bexp]
    d_bases = ctx.upload(host_points(grp, bases))
    row_exps = [rng.randrange(1, N) for _ in range(3)]
    batches = (1, 63, 64, 65, 200)
    cancelled = set()
    for idx, (nb, nr) in enumerate((nb, nr) for nb in (0, 1, 3, 16) for nr in (0, 1, 2)):
        # five scalar rows / row-point sets, spread over the lanes so that neighbours differ; set 4's rows cancel the sum
        pool = []
        for j in range(5):
            s = [rng.randrange(N) for _ in range(nb)]
            # sets 1 and 4: bit 255 in bases 0 and 2 (the same point), so the chain's first addition meets P + P;
            # set 3: bases 0 .. 2 silent and bases 3, 4 (P, -P) lead with N - 1, so the chain meets P - P
            if nb:
                s[0] = (0, N - 1, 2**256 - 1, 0, N - 1)[j]
            if nb >= 3:
                s[2] = (2**256 - 1, N - 1, 0, 0, 2**255)[j]
            if nb == 16:
                s[4] = s[3] = N - 1 if j == 3 else s[3]
            tot = sum(x * e for x, e in zip(s, bexp)) % N
            rexp = [row_exps[(j + k) % 3] for k in range(nr)]
            if nr and nb and j == 4:
                rexp[-1] = (-tot - sum(rexp[:-1])) % N
            pool.append((s, rexp, (tot + sum(rexp)) % N))
        for neg in (False, True):
            batch = batches[(2 * idx + neg) % len(batches)]
            lane = [(b * 3 + b // 64) % 5 for b in range(batch)]
            d_sc = ctx.upload(arr32([v for b in range(batch) for v in pool[lane[b]][0]])) if nb else None
            d_rows = ctx.upload(host_points(grp, [mul(grp, e) for b in range(batch) for e in pool[lane[b]][1]])) \
                if nr else None
            out = ctx.alloc(width * batch)
            ctx.bn256_lincomb_batch(grp, d_bases.ptr if nb else None, nb, d_sc.ptr if nb else None,
                                    d_rows.ptr if nr else None, nr, batch, neg, out.ptr)
            ctx.sync()
            raw = ctx.download(out.ptr, width * batch).tobytes()
            for b in range(batch):
                want = mul(grp, pool[lane[b]][2])
                if neg:
                    want = E.neg(want)
                if nb and nr and want is None:
                    cancelled.add(neg)
                assert raw[width * b:width * (b + 1)] == to_b(want), (nb, nr, neg, batch, b)
    assert cancelled == {False, True}


@pytest.mark.parametrize("grp", [1, 2])
def test_lincomb_batch_rejects_off_curve(ctx, grp):
    from verifiable_mpc_amd import _native
    E, G, to_b, _, width = GROUPS[grp]
    lib = _native.load_library()
    good = np.frombuffer(to_b(E.mul(7, G)), np.uint8).copy()
    bad = good.copy()
    bad[0] ^= 1
    sc = arr32([5])
    out = np.zeros(width, np.uint8)
    rc = lib.vmpc_bn256_lincomb_batch(grp, _native._np_ptr(bad), 1, _native._np_ptr(sc), None, 0, 1, 0,
                                      _native._np_ptr(out))
    assert rc == _native.E_NOTONCURVE
    rc = lib.vmpc_bn256_lincomb_batch(grp, _native._np_ptr(good), 1, _native._np_ptr(sc), _native._np_ptr(bad), 1, 1,
                                      0, _native._np_ptr(out))
    assert rc == _native.E_NOTONCURVE
    rc = lib.vmpc_bn256_lincomb_batch(grp, _native._np_ptr(good), 1, _native._np_ptr(sc), _native._np_ptr(good), 1, 1,
                                      1, _native._np_ptr(out))
    assert rc == 0
    assert out.tobytes() == to_b(E.neg(E.mul(5 * 7 + 7, G)))


# ---- 3. whole Pinocchio proofs at size --------------------------------------------------------------------------

def proof_expectations(key_logs, n, c_mid, h, deltas, mul):
    """the eight compute_proof elements by the exponent identity: element = (c_mid . e + deltas . tail) G"""
    from verifiable_mpc_amd import pynocchio as pn
    out = {}
    dv = [getattr(deltas, x) for x in pn._DELTAS] if deltas is not None else None
    for name, (_, zk) in pn._ELEMENTS.items():
        e = key_logs[name]
        tot = dot(c_mid, e[:n])
        if dv is not None:
            if name in pn._SHARED_G1:
                tot += dot(dv, e[n:n + 3])               # infinity columns carry exponent 0
            else:
                tot += dot([getattr(deltas, attr) for attr, _ in zk], e[n:])
        out[name] = mul(2 if name.endswith("g2") else 1, tot)
    out["h*g1"] = mul(1, dot(h, key_logs["h*g1"][:len(h)]))
    return out


class Deltas:
    def __init__(self, rng):
        self.v, self.w, self.y = (rng.randrange(N) for _ in range(3))


def check_key_columns(ctx, key_logs, n, rng, mul):
    """16 columns of every device-made key vector against the oracle (fixed-base once more, downloaded)"""
    for name, e in key_logs.items():
        grp = 2 if name.endswith("g2") else 1
        device_points(ctx, grp, e, rng, mul)


def assert_proof(proof, want):
    from verifiable_mpc_amd import pynocchio as pn
    assert set(proof) == set(want)
    for name, pt in want.items():
        grp = 2 if name.endswith("g2") else 1
        assert proof[name].to_bytes() == GROUPS[grp][2](pt), name
        assert isinstance(proof[name], pn.BN256TwistPoint if grp == 2 else pn.BN256Point)


@pytest.mark.parametrize("logn", [16, 18])
def test_compute_proof_at_size(ctx, mul, logn):
    """all eight elements of compute_proof over a synthetic prepared key with known discrete logs (three delta tail
    columns, infinity where an element does not use the delta): wire-like witness and one repeated scalar; deltas
    given and None; c as an (n, 32) array over the identity key and as a list over a key whose mid indices are a
    permutation of half of 2n wires (the gather path, array and list); h of length n and of length 1"""
    from verifiable_mpc_amd import pynocchio as pn
    n = 1 << logn
    rng = random.Random(logn)
    key, logs = pn.PreparedKey.synthetic(ctx, n, seed=logn, exponents=True)
    logs = {k: ints(v) for k, v in logs.items()}
    check_key_columns(ctx, logs, n, rng, mul)
    mid = np.random.default_rng(logn).permutation(2 * n)[:n]
    gkey = pn.PreparedKey.synthetic(ctx, n, seed=logn, mid=mid)
    wire = mi.wire_like(n, 100 + logn)
    rep = [rng.randrange(1, N)] * n
    h_full = mi.wire_like(n, 200 + logn)
    deltas = Deltas(rng)
    for c_mid, dl, h in ((wire, deltas, h_full), (rep, None, h_full[:1])):
        want = proof_expectations(logs, n, c_mid, h, dl, mul)
        assert_proof(pn.compute_proof(None, arr32(c_mid), h, key, dl), want)
        c_all = [rng.randrange(N) for _ in range(2 * n)]        # wires the key does not use: anything
        for j, w in enumerate(mid):
            c_all[w] = c_mid[j]
        other = None if dl is not None else deltas
        want2 = proof_expectations(logs, n, c_mid, h, other, mul)
        assert_proof(pn.compute_proof(None, c_all, h, gkey, other), want2)
        assert_proof(pn.compute_proof(None, arr32(c_all), arr32(h), gkey, other), want2)


def test_compute_proof_dict_path(ctx, mul):
    """n = 2^12: the dict (non-prepared) path and the prepared key over the same points give the oracle's elements"""
    from verifiable_mpc_amd import pynocchio as pn
    n = 1 << 12
    rng = random.Random(12)
    key, logs = pn.PreparedKey.synthetic(ctx, n, seed=12, exponents=True)
    logs = {k: ints(v) for k, v in logs.items()}
    evalkey = {}
    for name, (key_fmt, zk) in pn._ELEMENTS.items():
        grp = 2 if name.endswith("g2") else 1
        width = GROUPS[grp][4]
        dp = device_points(ctx, grp, logs[name], rng, mul)
        raw = ctx.download(dp.ptr, width * len(logs[name])).tobytes()
        cls = pn.BN256TwistPoint if grp == 2 else pn.BN256Point
        pts = [cls.from_bytes(raw[width * i:width * (i + 1)]) for i in range(len(logs[name]))]
        for i in range(n):
            evalkey[key_fmt(i)] = pts[i]
        tail = pts[n:]
        if name in pn._SHARED_G1:
            by = {attr: zname for attr, zname in zk}
            for j, attr in enumerate(pn._DELTAS):
                if attr in by:
                    evalkey[by[attr]] = tail[j]
        else:
            for j, (_, zname) in enumerate(zk):
                evalkey[zname] = tail[j]
    dp = device_points(ctx, 1, logs["h*g1"], rng, mul)
    raw = ctx.download(dp.ptr, 64 * n).tobytes()
    for i in range(n):
        evalkey["s^" + str(i) + "*g1"] = pn.BN256Point.from_bytes(raw[64 * i:64 * (i + 1)])

    class Q:
        indices_mid = list(range(n))

    class H:
        def __init__(self, coeffs):
            self.coeffs = coeffs

        def __len__(self):
            return len(self.coeffs)
    wire = mi.wire_like(n, 312)
    h = mi.wire_like(n, 313)
    deltas = Deltas(rng)
    for dl, hh in ((deltas, h), (None, h[:1])):
        want = proof_expectations(logs, n, wire, hh, dl, mul)
        assert_proof(pn.compute_proof(Q, wire, H(hh), evalkey, dl), want)
        assert_proof(pn.compute_proof(Q, wire, H(hh), key, dl), want)
