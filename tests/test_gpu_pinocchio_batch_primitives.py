"""The batched stages of the Pinocchio prover's h through the C ABI (csrc/bn256_qap_h.hip's *_batch_dev entries and
vmpc_bn256_fr_poly_mul_batch_dev of csrc/bn256_koe.hip): each against K calls of its single relative, byte for byte.
Every per-witness vector lies in rows 5 scalars longer than it needs; the padding is pre-filled with a sentinel and must
come back untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 5
SENTINEL = 0xA5
D_LIST = [1, 2, 63, 64, 65, 512, 513, 1024, 1025]     # QH_KB = 64, QH_KS = 512, QH_CHUNK = 1024 and their neighbours


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as v
    return v.get_context()


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


def _rand(rng, *shape):
    """any 32-byte values (reduced on load), a few rows of all ones (2^256 - 1) and of zero among them"""
    a = rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)
    flat = a.reshape(-1, 32)
    flat[::7] = 0xFF
    flat[3::11] = 0
    return a


def _padded(rows):
    """(K, n, 32) -> (K, n + PAD, 32) with the sentinel behind every row"""
    k, n = rows.shape[:2]
    out = np.full((k, n + PAD, 32), SENTINEL, np.uint8)
    out[:, :n] = rows
    return out


def _blank(ctx, k, n):
    """a device buffer of k rows of n + PAD scalars, all sentinel"""
    return ctx.upload(np.full((k, n + PAD, 32), SENTINEL, np.uint8))


def _rows_back(ctx, buf, k, n):
    """(the k rows' first n scalars, True if every padding byte is still the sentinel)"""
    a = ctx.download(buf.ptr, 32 * k * (n + PAD)).reshape(k, n + PAD, 32)
    return a[:, :n], bool((a[:, n:] == SENTINEL).all())


def _get(ctx, buf, n):
    return ctx.download(buf.ptr, 32 * n).reshape(n, 32)


# ---- moments ------------------------------------------------------------------------------------------------------------

def _single_moments(ctx, u0, u1, d, n_out):
    du0, du1 = ctx.upload(u0), ctx.upload(u1)
    o0, o1 = ctx.alloc(32 * n_out), ctx.alloc(32 * n_out)
    ctx.bn256_qap_moments(du0.ptr, du1.ptr, d, n_out, o0.ptr, o1.ptr)
    ctx.sync()
    return _get(ctx, o0, n_out), _get(ctx, o1, n_out)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("d", D_LIST)
def test_moments_batch(ctx, d, k):
    rng = np.random.default_rng(10 * d + k)
    u0, u1 = _rand(rng, k, d), _rand(rng, k, d)
    du0, du1 = ctx.upload(_padded(u0)), ctx.upload(_padded(u1))
    o0, o1, o2 = _blank(ctx, k, d), _blank(ctx, k, d), _blank(ctx, k, d)
    ctx.bn256_qap_moments_batch(du0.ptr, du1.ptr, d + PAD, d, d, o0.ptr, o1.ptr, d + PAD, k)
    ctx.bn256_qap_moments_batch(du1.ptr, None, d + PAD, d, d, o2.ptr, None, d + PAD, k)     # one vector
    ctx.sync()
    (g0, p0), (g1, p1), (g2, p2) = (_rows_back(ctx, o, k, d) for o in (o0, o1, o2))
    assert p0 and p1 and p2
    for w in range(k):
        w0, w1 = _single_moments(ctx, u0[w], u1[w], d, d)
        assert np.array_equal(g0[w], w0) and np.array_equal(g1[w], w1) and np.array_equal(g2[w], w1), w


def test_moments_batch_where_the_plan_leaves_the_single_one(ctx, nat):
    """groups = min(QH_TARGET_WGS / (n_kseg K), QH_MAX_GROUPS, chunks of j) = min(2048 / (n_kseg K), 32, ceil(d / 1024)).
    Up to d = 1024 there is one chunk and one group whatever K.  d = 1025 (n_out = d: n_kseg = 3) is the smallest d with
    two chunks; the single plan takes 2 groups, and 2048 / (3 K) falls below 2 first at K = 342 (2048 / 1023 = 2.002,
    2048 / 1026 = 1.996).  (d, K) = (1025, 342) is therefore the smallest pair at which the batch sums every j in ONE
    group where K single calls sum two - the arena's size says so - and the moments must not change."""
    d, k = 1025, 342
    align = lambda b: (b + 255) & ~255
    assert nat.bn256_qap_moments_batch_bytes(d, d, 1) == 2 * align(2 * d * 32) + 512
    assert nat.bn256_qap_moments_batch_bytes(d, d, k - 1) == 2 * align((k - 1) * 2 * d * 32) + 512
    assert nat.bn256_qap_moments_batch_bytes(d, d, k) == 2 * align(k * 1 * d * 32) + 512
    rng = np.random.default_rng(342)
    u0, u1 = _rand(rng, k, d), _rand(rng, k, d)
    du0, du1 = ctx.upload(_padded(u0)), ctx.upload(_padded(u1))
    o0, o1 = _blank(ctx, k, d), _blank(ctx, k, d)
    ctx.bn256_qap_moments_batch(du0.ptr, du1.ptr, d + PAD, d, d, o0.ptr, o1.ptr, d + PAD, k)
    ctx.sync()
    (g0, p0), (g1, p1) = _rows_back(ctx, o0, k, d), _rows_back(ctx, o1, k, d)
    assert p0 and p1
    for w in (0, k // 2, k - 1):
        w0, w1 = _single_moments(ctx, u0[w], u1[w], d, d)
        assert np.array_equal(g0[w], w0) and np.array_equal(g1[w], w1), w


# ---- the product --------------------------------------------------------------------------------------------------------

def _single_product(ctx, a, b):
    da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(32 * (len(a) + len(b) - 1))
    ctx.bn256_fr_poly_mul(da.ptr, len(a), db.ptr, len(b), out.ptr)
    ctx.sync()
    return _get(ctx, out, len(a) + len(b) - 1)


@pytest.mark.parametrize("n", [1, 2, 64, 65, 256, 257, 513])
def test_product_batch_windows(ctx, n):
    """FR_CONV_CHUNK = 64, FR_CONV_TILE = 256, shortest segment 256: n = 257 and 513 cut tiles into two and three
    segments (partial sums through the arena), below that every tile is written straight to its row.  The full window and
    the two halves the batched h asks for: [0, n - 1) (empty at n = 1) and [n - 1, 2n - 1)."""
    k = 3
    rng = np.random.default_rng(n)
    a, b = _rand(rng, k, n), _rand(rng, k, n)
    want = [_single_product(ctx, a[w], b[w]) for w in range(k)]
    want_shared = [_single_product(ctx, a[w], b[0]) for w in range(k)]
    da, db = ctx.upload(_padded(a)), ctx.upload(_padded(b))
    db_same = ctx.upload(_padded(np.stack([b[0]] * k)))
    for lo, cnt in ((0, 2 * n - 1), (0, n - 1), (n - 1, n)):
        o_dist, o_shared, o_copies = _blank(ctx, k, cnt), _blank(ctx, k, cnt), _blank(ctx, k, cnt)
        ctx.bn256_fr_poly_mul_batch(da.ptr, n + PAD, n, db.ptr, n + PAD, n, lo, cnt, o_dist.ptr, cnt + PAD, k)
        ctx.bn256_fr_poly_mul_batch(da.ptr, n + PAD, n, db.ptr, 0, n, lo, cnt, o_shared.ptr, cnt + PAD, k)
        ctx.bn256_fr_poly_mul_batch(da.ptr, n + PAD, n, db_same.ptr, n + PAD, n, lo, cnt, o_copies.ptr, cnt + PAD, k)
        ctx.sync()
        (g, p), (gs, ps), (gc, pc) = (_rows_back(ctx, o, k, cnt) for o in (o_dist, o_shared, o_copies))
        assert p and ps and pc, (lo, cnt)
        for w in range(k):
            assert np.array_equal(g[w], want[w][lo:lo + cnt]), (lo, cnt, w)
            assert np.array_equal(gs[w], want_shared[w][lo:lo + cnt]), (lo, cnt, w)
        assert np.array_equal(gs, gc)             # a shared b (stride 0) against K copies of it


def test_product_batch_empty_window_writes_nothing(ctx):
    """d = 1: P's window [0, d - 1) has no outputs"""
    rng = np.random.default_rng(1)
    a, b = _rand(rng, 2, 1), _rand(rng, 2, 1)
    da, db, out = ctx.upload(_padded(a)), ctx.upload(_padded(b)), _blank(ctx, 2, 0)
    ctx.bn256_fr_poly_mul_batch(da.ptr, 1 + PAD, 1, db.ptr, 1 + PAD, 1, 0, 0, out.ptr, PAD, 2)
    ctx.sync()
    assert (ctx.download(out.ptr, 32 * 2 * PAD) == SENTINEL).all()


@pytest.mark.parametrize("na,nb", [(1, 1), (257, 513), (700, 3), (1025, 1025)])
def test_product_batch_of_one_equals_the_single_entry(ctx, na, nb):
    rng = np.random.default_rng(na + nb)
    a, b = _rand(rng, na), _rand(rng, nb)
    da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(32 * (na + nb - 1))
    ctx.bn256_fr_poly_mul_batch(da.ptr, na, na, db.ptr, nb, nb, 0, na + nb - 1, out.ptr, na + nb - 1, 1)
    ctx.sync()
    assert _get(ctx, out, na + nb - 1).tobytes() == _single_product(ctx, a, b).tobytes()


# ---- weights, check, combination ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", D_LIST)
def test_weights_batch(ctx, d):
    k = 3
    rng = np.random.default_rng(d)
    a, b = _rand(rng, k, d), _rand(rng, k, d)
    da, db = ctx.upload(_padded(a)), ctx.upload(_padded(b))
    ua, ub, ua1 = _blank(ctx, k, d), _blank(ctx, k, d), _blank(ctx, k, d)
    ctx.bn256_qap_h_weights_batch(da.ptr, db.ptr, d + PAD, d, ua.ptr, ub.ptr, d + PAD, k)
    ctx.bn256_qap_h_weights_batch(da.ptr, None, d + PAD, d, ua1.ptr, None, d + PAD, k)
    ctx.sync()
    (ga, pa), (gb, pb), (g1, p1) = (_rows_back(ctx, o, k, d) for o in (ua, ub, ua1))
    assert pa and pb and p1
    for w in range(k):
        sa, sb, oa, ob = ctx.upload(a[w]), ctx.upload(b[w]), ctx.alloc(32 * d), ctx.alloc(32 * d)
        ctx.bn256_qap_h_weights(sa.ptr, sb.ptr, d, oa.ptr, ob.ptr)
        ctx.sync()
        assert np.array_equal(ga[w], _get(ctx, oa, d)) and np.array_equal(gb[w], _get(ctx, ob, d)), w
        assert np.array_equal(g1[w], ga[w])


def _to_ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


@pytest.mark.parametrize("d", D_LIST)
def test_check_batch(ctx, d):
    """witness 1 of 3 bad at its LAST row -> (none, d - 1, none); then all good, and a witness with two bad rows"""
    from tests.keygen_ref import N, to_array
    rng = np.random.default_rng(d)
    a, b = _rand(rng, 3, d), _rand(rng, 3, d)
    y = np.stack([to_array([x * z % N for x, z in zip(_to_ints(a[w]), _to_ints(b[w]))]) for w in range(3)])
    da, db = ctx.upload(_padded(a)), ctx.upload(_padded(b))
    bad = ctx.upload(np.full(5, 0x5A5A5A5A, np.uint32))

    def run(spoil):
        yy = y.copy()
        for w, i in set(spoil):
            yy[w, i, 0] ^= 1
        dy = ctx.upload(_padded(yy))
        ctx.bn256_qap_check_batch(da.ptr, db.ptr, dy.ptr, d + PAD, d, bad.ptr, 3)
        ctx.sync()
        got = ctx.download(bad.ptr, 20).view("<u4").tolist()
        assert got[3:] == [0x5A5A5A5A] * 2                      # the words behind the K are not the call's
        for w in range(3):                                      # and each word is what the single entry says
            sa, sb, sy, one = ctx.upload(a[w]), ctx.upload(b[w]), ctx.upload(yy[w]), ctx.alloc(4)
            ctx.bn256_qap_check(sa.ptr, sb.ptr, sy.ptr, d, one.ptr)
            ctx.sync()
            assert int(ctx.download(one.ptr, 4).view("<u4")[0]) == got[w]
        return got[:3]
    none = 0xFFFFFFFF
    assert run([(1, d - 1)]) == [none, d - 1, none]
    assert run([]) == [none] * 3
    assert run([(2, d - 1), (2, d // 2), (0, 0)]) == [0, none, d // 2]


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("d", D_LIST)
def test_combine_batch(ctx, d, zk):
    k = 3
    rng = np.random.default_rng(2 * d + zk)
    A, B = _rand(rng, k, d), _rand(rng, k, d)
    deltas = _rand(rng, k, 3)
    t, t_scratch = ctx.alloc(32 * (d + 1)), ctx.alloc(64 * (d + (d + 127) // 128))
    ctx.bn256_qap_t_coeffs(d, t_scratch.ptr, t.ptr)
    dA, dB, dd = ctx.upload(_padded(A)), ctx.upload(_padded(B)), ctx.upload(deltas)
    scratch, out = ctx.alloc(32 * 3 * d * k), _blank(ctx, k, d + 1)
    ctx.bn256_qap_h_combine_batch(dA.ptr, dB.ptr, d + PAD, t.ptr, d, dd.ptr if zk else None, scratch.ptr, out.ptr,
                                  d + 1 + PAD, k)
    ctx.sync()
    got, pad_ok = _rows_back(ctx, out, k, d + 1)
    assert pad_ok
    for w in range(k):
        sA, sB, sd = ctx.upload(A[w]), ctx.upload(B[w]), ctx.upload(deltas[w])
        s_scratch, s_out = ctx.alloc(32 * 5 * d), ctx.alloc(32 * (d + 1))
        ctx.bn256_qap_h_combine(sA.ptr, sB.ptr, t.ptr, d, sd.ptr if zk else None, s_scratch.ptr, s_out.ptr)
        ctx.sync()
        assert np.array_equal(got[w], _get(ctx, s_out, d + 1)), w


# ---- limits ---------------------------------------------------------------------------------------------------------------

def test_limits(ctx, nat):
    """n_wit above VMPC_BN256_QAP_MAX_WIT and d above the single entries' cap: VMPC_E_RANGE before any pointer is looked
    at (they are all null here); a stride below the row: the same; n_wit = 0: VMPC_OK and nothing written"""
    big, d_cap = nat.BN256_QAP_MAX_WIT + 1, nat.BN256_FR_POLY_MAX
    assert big == 65536
    for n_wit, d in ((big, 8), (1, d_cap)):
        calls = [lambda: ctx.bn256_qap_check_batch(0, 0, 0, d, d, 0, n_wit),
                 lambda: ctx.bn256_qap_h_weights_batch(0, 0, d, d, 0, 0, d, n_wit),
                 lambda: ctx.bn256_qap_moments_batch(0, 0, d, d, 8, 0, 0, 8, n_wit),
                 lambda: ctx.bn256_qap_h_combine_batch(0, 0, d, 0, d, 0, 0, 0, d + 1, n_wit),
                 lambda: ctx.bn256_fr_poly_mul_batch(0, d + 1, d + 1, 0, 0, 8, 0, 8, 0, 8, n_wit)]
        for call in calls:
            with pytest.raises(nat.VmpcError) as ei:
                call()
            assert ei.value.code == nat.E_RANGE
    short = [lambda: ctx.bn256_qap_check_batch(0, 0, 0, 7, 8, 0, 2),
             lambda: ctx.bn256_qap_h_weights_batch(0, 0, 8, 8, 0, 0, 7, 2),
             lambda: ctx.bn256_qap_moments_batch(0, 0, 8, 8, 8, 0, 0, 7, 2),
             lambda: ctx.bn256_qap_h_combine_batch(0, 0, 8, 0, 8, 0, 0, 0, 8, 2),
             lambda: ctx.bn256_fr_poly_mul_batch(0, 8, 8, 0, 7, 8, 0, 15, 0, 15, 2),
             lambda: ctx.bn256_fr_poly_mul_batch(0, 8, 8, 0, 0, 8, 1, 15, 0, 15, 2)]       # a window past the product
    for call in short:
        with pytest.raises(nat.VmpcError) as ei:
            call()
        assert ei.value.code == nat.E_RANGE
    with pytest.raises(nat.VmpcError) as ei:
        ctx.bn256_qap_moments_batch(0, 0, 8, 8, 8, 0, 0, 8, 2)       # in range: null pointers are the complaint
    assert ei.value.code == nat.E_INVAL
    assert nat.bn256_qap_moments_batch_bytes(8, 8, big) == 0 and nat.bn256_qap_moments_batch_bytes(8, 8, 0) == 0
    assert nat.bn256_fr_poly_mul_batch_bytes(8, 8, 0, 15, big) == 0
    d = 8
    buf = [_blank(ctx, 1, 3 * d) for _ in range(6)]
    p = [b.ptr for b in buf]
    ctx.bn256_qap_check_batch(p[0], p[1], p[2], d, d, p[3], 0)
    ctx.bn256_qap_h_weights_batch(p[0], p[1], d, d, p[3], p[4], d, 0)
    ctx.bn256_qap_moments_batch(p[0], p[1], d, d, d, p[3], p[4], d, 0)
    ctx.bn256_qap_h_combine_batch(p[0], p[1], d, p[2], d, None, p[5], p[3], d + 1, 0)
    ctx.bn256_fr_poly_mul_batch(p[0], d, d, p[1], d, d, 0, 2 * d - 1, p[3], 2 * d - 1, 0)
    ctx.sync()
    for b in buf:
        assert (ctx.download(b.ptr, 32 * (3 * d + PAD)) == SENTINEL).all()
