"""GPU tests of the polynomial product by the multi-prime NTT over the integers (csrc/bn256_ntt.hip over csrc/ntt31.h;
vmpc_bn256_fr_poly_mul_ntt_dev / _batch_dev): exactly against Python integers on small shapes, against the schoolbook
entry (csrc/bn256_koe.hip, unchanged) on the rest - at every length where the planner takes another path: one
workgroup in LDS up to BN256_FR_NTT_LDS_LEN points, then one column pass of 1 .. 6 stages, then two."""
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn

pytestmark = pytest.mark.gpu
N = bn.N
TOP = (1 << 256) - 1
PAD = 5


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def nat(vm):
    return vm._native


@pytest.fixture(scope="module")
def ctx(vm):
    return vm.get_context()


def to_arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)


def to_ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def coeff(a, b, k):
    return sum(a[i] * b[k - i] for i in range(max(0, k - len(b) + 1), min(len(a) - 1, k) + 1)) % N


def product(a, b):
    return [coeff(a, b, k) for k in range(len(a) + len(b) - 1)]


def ntt_mul(ctx, a, b):
    """the whole product of two lists of ints / two (len, 32) arrays through the NTT entry, as ints"""
    a, b = (v if isinstance(v, np.ndarray) else to_arr(v) for v in (a, b))
    da, db = ctx.upload(a), ctx.upload(b)
    n = len(a) + len(b) - 1
    out = ctx.alloc(32 * n)
    ctx.bn256_fr_poly_mul_ntt(da.ptr, len(a), db.ptr, len(b), out.ptr)
    ctx.sync()
    return ctx.download(out.ptr, 32 * n).reshape(-1, 32)


def school_mul(ctx, a, b):
    assert ctx.get_poly_product() == 0
    da, db = ctx.upload(a), ctx.upload(b)
    n = len(a) + len(b) - 1
    out = ctx.alloc(32 * n)
    ctx.bn256_fr_poly_mul(da.ptr, len(a), db.ptr, len(b), out.ptr)
    ctx.sync()
    return ctx.download(out.ptr, 32 * n).reshape(-1, 32)


def random_scalars(seed, n):
    """(n, 32) uint8 of any 32-byte values (not reduced: the entry's contract)"""
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


# ---- exactly, against Python integers ---------------------------------------------------------------------------------

def test_lengths_1_to_9_exact(ctx):
    rng = random.Random(1)
    for na in range(1, 10):
        for nb in range(1, 10):
            a = [rng.choice([rng.randrange(N), rng.randrange(1 << 256)]) for _ in range(na)]
            b = [rng.choice([rng.randrange(N), rng.randrange(1 << 256)]) for _ in range(nb)]
            assert to_ints(ntt_mul(ctx, a, b)) == product(a, b), (na, nb)


@pytest.mark.parametrize("na,nb", [(128, 129), (129, 128), (1, 300), (300, 1), (255, 2), (256, 1), (256, 2)])
def test_straddling_a_power_of_two_exact(ctx, na, nb):
    rng = random.Random(na * 1000 + nb)
    a = [rng.randrange(1 << 256) for _ in range(na)]
    b = [rng.randrange(1 << 256) for _ in range(nb)]
    assert to_ints(ntt_mul(ctx, a, b)) == product(a, b)


def test_worst_carries(ctx):
    """all-ones scalars, unreduced: the integer coefficient reaches 257 (2^256 - 1)^2, which 17 primes cannot hold at
    the cap; (n - 1)^2 = 1 mod n"""
    got = to_ints(ntt_mul(ctx, [TOP] * 257, [TOP] * 257))
    assert got == [(min(k, 512 - k) + 1) * TOP * TOP % N for k in range(513)]
    got = to_ints(ntt_mul(ctx, [N - 1] * 1000, [N - 1] * 1000))
    assert got == [min(k, 1998 - k) + 1 for k in range(1999)]


def test_zeros_and_a_multiple_of_n(ctx):
    rng = random.Random(5)
    a = [rng.randrange(N) for _ in range(700)]
    assert to_ints(ntt_mul(ctx, a, [0] * 300)) == [0] * 999
    assert to_ints(ntt_mul(ctx, [0] * 300, a)) == [0] * 999
    assert to_ints(ntt_mul(ctx, [N] * 5, a)) == [0] * 704


# ---- against the schoolbook entry: every plan of passes ---------------------------------------------------------------

def test_one_workgroup_two_pass_boundary(ctx, nat):
    s = nat.BN256_FR_NTT_LDS_LEN
    assert s & (s - 1) == 0
    for total in (s - 1, s, s + 1, 2 * s):
        na = (total + 1) // 2 + 1
        nb = total + 1 - na
        a, b = random_scalars(total, na), random_scalars(total + 1, nb)
        assert np.array_equal(ntt_mul(ctx, a, b), school_mul(ctx, a, b)), (na, nb)


@pytest.mark.parametrize("na,nb", [(5000, 3000), (9000, 7000), (20000, 10000), (40000, 20000),      # one pass: 2 .. 5 stages
                                   (131073, 5), (262145, 7), (524289, 3)])                          # two: 4+3, 4+4, 5+4
def test_every_pass_plan_against_schoolbook(ctx, na, nb):
    a, b = random_scalars(na, na), random_scalars(nb, nb)
    assert np.array_equal(ntt_mul(ctx, a, b), school_mul(ctx, a, b))


def test_2_16_square_equals_schoolbook(ctx):
    n = 1 << 16
    a, b = random_scalars(16, n), random_scalars(17, n)
    got = ntt_mul(ctx, a, b)
    assert got.shape == (2 * n - 1, 32) and np.array_equal(got, school_mul(ctx, a, b))


def test_2_20_square_by_evaluation(ctx, nat):
    """the cap, L = 2^21: a(r) b(r) == c(r) mod n at one random r - exact; a wrong product passes with probability
    about 2^21 / 2^256"""
    n = nat.BN256_FR_POLY_MAX
    a, b = random_scalars(20, n), random_scalars(21, n)
    c = ntt_mul(ctx, a, b)
    r = random.Random(20).randrange(N)

    def horner(arr):
        acc = 0
        raw = arr.tobytes()
        for i in range(len(raw) - 32, -1, -32):
            acc = (acc * r + int.from_bytes(raw[i:i + 32], "little")) % N
        return acc
    assert c.shape == (2 * n - 1, 32)
    assert horner(a) * horner(b) % N == horner(c)
    top = c[:, 31].astype(np.uint32) << 8 | c[:, 30].astype(np.uint32)      # canonical: not above n's top 16 bits
    assert int(top.max()) <= (N >> 240)


# ---- window, batch, groups --------------------------------------------------------------------------------------------

def test_window(ctx):
    na, nb, k = 700, 300, 2
    rng = random.Random(7)
    rows_a = [[rng.randrange(1 << 256) for _ in range(na)] for _ in range(k)]
    rows_b = [[rng.randrange(1 << 256) for _ in range(nb)] for _ in range(k)]
    want = [product(a, b) for a, b in zip(rows_a, rows_b)]
    a_arr = np.zeros((k, na + PAD, 32), np.uint8)
    b_arr = np.zeros((k, nb + PAD, 32), np.uint8)
    for w in range(k):
        a_arr[w, :na], b_arr[w, :nb] = to_arr(rows_a[w]), to_arr(rows_b[w])
        a_arr[w, na:], b_arr[w, nb:] = 0x5A, 0x5A          # what lies between the rows is not part of them
    da, db = ctx.upload(a_arr), ctx.upload(b_arr)
    total = na + nb - 1
    seen = 0
    for lo in (0, 1, 255, 256, 698, 997):
        for cnt in (1, 2, 256, 257, total - lo):
            if lo + cnt > total:
                continue
            seen += 1
            stride = cnt + PAD
            pattern = np.full((k, stride, 32), 0xA5, np.uint8)
            out = ctx.upload(pattern)
            ctx.bn256_fr_poly_mul_ntt_batch(da.ptr, na + PAD, na, db.ptr, nb + PAD, nb, lo, cnt, out.ptr, stride, k)
            ctx.sync()
            got = ctx.download(out.ptr, pattern.nbytes).reshape(k, stride, 32)
            for w in range(k):
                assert to_ints(got[w, :cnt]) == want[w][lo:lo + cnt], (lo, cnt, w)
            assert np.array_equal(got[:, cnt:], pattern[:, cnt:]), (lo, cnt)
    assert seen == 5 * 5 + 3           # from 997 only two outputs are left


@pytest.mark.parametrize("na,nb", [(130, 70), (2100, 50)])
def test_batch_rows_equal_single_products(ctx, na, nb):
    for k in (1, 2, 3):
        a_arr = random_scalars(na + k, k * (na + PAD)).reshape(k, na + PAD, 32)
        b_arr = random_scalars(nb + k, k * (nb + PAD)).reshape(k, nb + PAD, 32)
        da, db, db_tight = ctx.upload(a_arr), ctx.upload(b_arr), ctx.upload(np.ascontiguousarray(b_arr[:, :nb]))
        total = na + nb - 1
        for b_stride, dbuf, b_row in ((0, db, lambda w: b_arr[0, :nb]), (nb, db_tight, lambda w: b_arr[w, :nb]),
                                      (nb + PAD, db, lambda w: b_arr[w, :nb])):
            out = ctx.alloc(32 * total * k)
            ctx.bn256_fr_poly_mul_ntt_batch(da.ptr, na + PAD, na, dbuf.ptr, b_stride, nb, 0, total, out.ptr, total, k)
            ctx.sync()
            got = ctx.download(out.ptr, 32 * total * k).reshape(k, total, 32)
            for w in range(k):
                assert np.array_equal(got[w], ntt_mul(ctx, np.ascontiguousarray(a_arr[w, :na]),
                                                      np.ascontiguousarray(b_row(w)))), (k, b_stride, w)


def test_group_boundary_changes_nothing(ctx, nat):
    """with the arena cap lowered to three rows of residues a batch of five runs as groups of 2, 2, 1 (one b for all) or
    of 1 (a b per product): same rows, same order"""
    na, nb, k = 130, 70, 5
    total = na + nb - 1
    row_bytes = 18 * 256 * 4                  # 18 primes, L = 256, uint32
    a_arr, b_arr = random_scalars(31, k * na).reshape(k, na, 32), random_scalars(32, k * nb).reshape(k, nb, 32)
    da, db = ctx.upload(a_arr), ctx.upload(b_arr)

    def run(b_stride):
        out = ctx.alloc(32 * total * k)
        ctx.bn256_fr_poly_mul_ntt_batch(da.ptr, na, na, db.ptr, b_stride, nb, 0, total, out.ptr, total, k)
        ctx.sync()
        return ctx.download(out.ptr, 32 * total * k).reshape(k, total, 32)
    whole = {s: run(s) for s in (0, nb)}
    for w in range(k):
        assert np.array_equal(whole[nb][w], school_mul(ctx, a_arr[w], b_arr[w]))
        assert np.array_equal(whole[0][w], school_mul(ctx, a_arr[w], b_arr[0]))
    ctx.set_ntt_arena_cap(3 * row_bytes)
    try:
        for s in (0, nb):
            assert np.array_equal(run(s), whole[s]), s
    finally:
        ctx.set_ntt_arena_cap(0)
    assert nat.bn256_fr_poly_mul_ntt_batch_bytes(na, nb, 0, total, k) >= 2 * k * row_bytes


# ---- the answers of the schoolbook entry ------------------------------------------------------------------------------

def test_above_the_cap_is_e_range_and_writes_nothing(ctx, nat):
    cap = nat.BN256_FR_POLY_MAX
    pattern = np.full(64, 0xA5, np.uint8)
    a, b, out = ctx.upload(to_arr([3, 4])), ctx.upload(to_arr([5])), ctx.upload(pattern)
    for na, nb in ((cap + 1, 1), (1, cap + 1), (cap + 1, cap + 1)):
        with pytest.raises(nat.VmpcError) as ei:
            ctx.bn256_fr_poly_mul_ntt(a.ptr, na, b.ptr, nb, out.ptr)
        assert ei.value.code == nat.E_RANGE
        with pytest.raises(nat.VmpcError) as ei:      # before any pointer is looked at
            ctx.bn256_fr_poly_mul_ntt(0, na, 0, nb, 0)
        assert ei.value.code == nat.E_RANGE
        ctx.sync()
        assert np.array_equal(ctx.download(out.ptr, 64), pattern)
    ctx.bn256_fr_poly_mul_ntt(a.ptr, 2, b.ptr, 1, out.ptr)
    ctx.sync()
    assert to_ints(ctx.download(out.ptr, 64)) == [15, 20]


def test_range_null_and_empty_answers_match_the_schoolbook_entry(ctx, nat):
    big = 65536
    a, b, out = ctx.upload(to_arr(range(1, 9))), ctx.upload(to_arr(range(1, 9))), ctx.upload(np.full(32 * 20, 0xA5, np.uint8))
    calls = [
        (0, 8, 8, 0, 0, 8, 0, 8, 0, 8, big),                    # too many products
        (0, 8, 8, 0, 7, 8, 0, 15, 0, 15, 2),                    # a stride of b below nb
        (0, 7, 8, 0, 0, 8, 0, 15, 0, 15, 2),                    # a stride of a below na
        (0, 8, 8, 0, 0, 8, 0, 15, 0, 14, 2),                    # a stride of out below the window
        (0, 8, 8, 0, 0, 8, 1, 15, 0, 15, 2),                    # a window past the product
        (0, 8, 8, 0, 0, 8, 0, 15, 0, (1 << 31) + 1, 2),         # a stride above 2^31
        (a.ptr, 8, 8, 0, 8, 8, 0, 15, out.ptr, 15, 1),          # a null operand
        (a.ptr, 8, 8, b.ptr, 8, 8, 0, 15, 0, 15, 1),            # a null result
        (a.ptr, 8, 0, b.ptr, 8, 8, 0, 0, out.ptr, 15, 1),       # an empty operand
    ]
    for args in calls:
        codes = []
        for fn in (ctx.bn256_fr_poly_mul_batch, ctx.bn256_fr_poly_mul_ntt_batch):
            with pytest.raises(nat.VmpcError) as ei:
                fn(*args)
            codes.append(ei.value.code)
        assert codes[0] == codes[1] and codes[0] in (nat.E_RANGE, nat.E_INVAL), (args, codes)
    assert nat.bn256_fr_poly_mul_ntt_batch_bytes(8, 8, 0, 15, big) == 0
    assert nat.bn256_fr_poly_mul_ntt_batch_bytes(8, 8, 1, 15, 1) == 0
    # no products, or an empty window: VMPC_OK and nothing launched or written
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        ctx.bn256_fr_poly_mul_ntt_batch(a.ptr, 8, 8, b.ptr, 8, 8, 0, 15, out.ptr, 15, 0)
        ctx.bn256_fr_poly_mul_ntt_batch(a.ptr, 8, 8, b.ptr, 8, 8, 3, 0, out.ptr, 15, 1)
        ctx.sync()
        assert not any(k.startswith("bn_fr_ntt") and v[1] for k, v in ctx.profile_read(reset=True).items())
    finally:
        ctx.profile(False)
    assert np.array_equal(ctx.download(out.ptr, 32 * 20), np.full(32 * 20, 0xA5, np.uint8))
