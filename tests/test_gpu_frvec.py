"""The GF(l) vector kernels (csrc/frvec.hip) one entry point at a time, against tests/frvec_ref.py.  Every comparison is
exact (32-byte residues, byte for byte); the vectors are canonical residues, as the entries' contract asks.

The shapes stand for the launch constants, restated here (nothing is imported from the code under test): FR_BLOCK = 256
lanes per workgroup, FR_MAX_GRID = 2048 workgroups, so a launch has at most 524 288 lanes and a lane takes a second trip
of its grid-stride loop only past that; k_fr_dot leaves one partial per workgroup and the single workgroup of k_fr_sum
takes a second trip past 256 of them; fr_chal_arg holds 20 challenges by value.

axpy / scale / axpy_tail, n elements:
    n = 1, 255, 256, 257     one lane; a workgroup one short of full, full, a second of one lane
    n = 524288               every lane of the capped grid, one trip each
    n = 524289               lane 0 of workgroup 0 alone takes a second trip
    n = 524545               the second trip covers workgroup 0 and lane 0 of workgroup 1
    n = 0 (axpy_tail)        only the tail is written, x may be NULL
dot / dot_to_dev:
    n = 0, 1                 no launch; one product
    n = 65536, 65537         256 partials (one trip of k_fr_sum), 257 (lane 0 of k_fr_sum takes a second)
    n = 524288, 524289, 524545   as above, with 2048 partials
    one-hot pairs (a and b zero but for one index): an element that is dropped cannot cancel against another
challenge_products, n = 2^(rounds + low_bits):
    (0, 0), (0, 4)           no challenge: a copy of z
    (1, 0), (4, 0)           z of one element
    (3, 5)                   both
    (20, 0)                  every slot of the by-value array; 2^20 is the smallest power of two past the grid cap
    (2, 18)                  the same n with z of 2^18 elements
tail_scalars (log2_m0, t), m = 2^log2_m0 >> t:
    (1, 0), (2, 1), (6, 5), (9, 8)   m = 2, h = 1: the last round the launcher accepts, at four lengths
    (9, 0)                   two workgroups, no challenge
    (20, 1)                  past the grid cap
tail_scalars_inc at log2_m0 = 9 through every t; tail_scalars_block at log2_m0 = 10 in the blocks [0, 1), [1, 300),
[300, 512), [512, 513), [513, 1024): lengths that are no multiple of 256, cuts on the index bit that t = 1 looks at
(bit 9: 512) and beside the one that t = 10 - 1 looks at (bit 1; 513 is odd).

Every buffer an entry writes lies between two guard elements of 0x5a bytes and starts out as that pattern, which is no
canonical residue: a written zero is a written zero.
"""
import ctypes

import numpy as np
import pytest

from tests import frvec_ref as ref

pytestmark = pytest.mark.gpu

ELL = ref.ELL
PAT_BYTE = 0x5A
POOL_N = 1 << 20
BIG = (524288, 524289, 524545)
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


@pytest.fixture(scope="module")
def ctx(nat):
    c = nat.Context(0)
    yield c
    c.close()


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32).copy()


def _ints(a):
    raw = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _sc(v):
    return ctypes.create_string_buffer(int(v).to_bytes(32, "little"), 32)


def _scs(vals):
    return ctypes.create_string_buffer(b"".join(int(v).to_bytes(32, "little") for v in vals), 32 * max(len(vals), 1))


class Guarded:
    """n elements of device memory between two guard elements; guards and elements start as the pattern (or `fill`)"""

    def __init__(self, ctx, n, fill=None):
        self.ctx, self.n = ctx, n
        host = np.full((n + 2, 32), PAT_BYTE, np.uint8)
        if fill is not None:
            host[1:n + 1] = fill
        self.buf = ctx.upload(host)
        self.ptr = self.buf.ptr + 32

    def read(self):
        """the n elements as (n, 32) bytes, after the stream has drained and the guards have been looked at"""
        self.ctx.sync()
        raw = self.ctx.download(self.buf.ptr, 32 * (self.n + 2), (self.n + 2, 32))
        assert (raw[0] == PAT_BYTE).all(), "the element in front of the buffer was written"
        assert (raw[-1] == PAT_BYTE).all(), "the element behind the buffer was written"
        return raw[1:-1]

    def untouched(self):
        return bool((self.read() == PAT_BYTE).all())


def same(got, want, what):
    want = np.asarray(want, np.uint8).reshape(-1, 32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ, the first at {i}: got "
                             f"{_ints(got[i])[0]:#x}, want {_ints(want[i])[0]:#x}")


class Pool:
    """2^20 random residues (below 2^252: the planted l - 1 stands for the range above), as bytes and as ints"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.b = rng.integers(0, 256, size=(POOL_N, 32), dtype=np.uint8)
        self.b[:, 31] &= 0x0F
        self.i = _ints(self.b)

    def planted(self, n, offset=0):
        """(bytes, ints) of n elements from `offset` on, with l - 1 at index 0 and at the last index"""
        assert offset + n <= POOL_N
        b, i = self.b[offset:offset + n].copy(), self.i[offset:offset + n]
        if n:
            b[0] = b[-1] = _bytes([ELL - 1])[0]
            i[0] = i[-1] = ELL - 1
        return b, i


@pytest.fixture(scope="module")
def pools():
    return Pool(20250), Pool(20251)


@pytest.fixture(scope="module")
def big_axpy(pools):
    """c and the bytes of c x + y and c x over the unplanted pools, once for every large n: a case takes a prefix and
    restates the two planted elements"""
    X, Y = pools
    c = X.i[-1] | (1 << 251)
    assert c < ELL
    n = max(BIG)
    return c, _bytes(ref.axpy(c, X.i[:n], Y.i[:n])), _bytes(ref.axpy(c, X.i[:n]))


def _expected_axpy(big_axpy, c, x, y):
    """bytes of (c x + y, c x) for planted prefixes x, y of the pools"""
    n = len(x)
    if c == big_axpy[0] and n > 4096:
        wa, ws = big_axpy[1][:n].copy(), big_axpy[2][:n].copy()
        for k in (0, n - 1):
            wa[k] = _bytes(ref.axpy(c, [x[k]], [y[k]]))[0]
            ws[k] = _bytes(ref.axpy(c, [x[k]]))[0]
        return wa, ws
    return _bytes(ref.axpy(c, x, y)), _bytes(ref.axpy(c, x))


# ---- vmpc_fr_axpy_dev, vmpc_fr_scale_dev, vmpc_fr_axpy_tail_dev --------------------------------------------------------------
def _axpy_family(ctx, c, xb, yb, want_axpy, want_scale, tails):
    n = len(xb)
    dx, dy = ctx.upload(xb), ctx.upload(yb)
    out = Guarded(ctx, n)
    ctx.fr_axpy(c, dx.ptr, dy.ptr, n, out.ptr)
    same(out.read(), want_axpy, "axpy")
    out = Guarded(ctx, n)
    ctx.fr_scale(c, dx.ptr, n, out.ptr)
    same(out.read(), want_scale, "scale")
    for tail in tails:
        for y_ptr, want, what in ((dy.ptr, want_axpy, "axpy_tail"), (None, want_scale, "axpy_tail, y = NULL")):
            out = Guarded(ctx, n + 1)
            ctx.fr_axpy_tail(c, dx.ptr, y_ptr, n, tail, out.ptr)
            got = out.read()
            same(got[:n], want, what)
            same(got[n:], _bytes([tail]), f"{what}: the tail {tail:#x}")
    # in place, as z' = z_l + c z_r overwrites either operand
    g = Guarded(ctx, n, fill=yb)
    ctx.fr_axpy(c, dx.ptr, g.ptr, n, g.ptr)
    same(g.read(), want_axpy, "axpy, out == y")
    g = Guarded(ctx, n, fill=xb)
    ctx.fr_axpy(c, g.ptr, dy.ptr, n, g.ptr)
    same(g.read(), want_axpy, "axpy, out == x")
    g = Guarded(ctx, n, fill=xb)
    ctx.fr_scale(c, g.ptr, n, g.ptr)
    same(g.read(), want_scale, "scale, out == x")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 524288, 524289, 524545])
def test_axpy_scale_axpy_tail(ctx, pools, big_axpy, n):
    X, Y = pools
    (xb, x), (yb, y) = X.planted(n), Y.planted(n)
    c = big_axpy[0]
    want_axpy, want_scale = _expected_axpy(big_axpy, c, x, y)
    _axpy_family(ctx, c, xb, yb, want_axpy, want_scale, (0, 1, ELL - 1))


@pytest.mark.parametrize("c", [0, 1, ELL - 1, "random"])
def test_axpy_constants(ctx, pools, big_axpy, c):
    X, Y = pools
    n = 257
    c = X.i[7] if c == "random" else c
    (xb, x), (yb, y) = X.planted(n, 1000), Y.planted(n, 1000)
    want_axpy, want_scale = _expected_axpy(big_axpy, c, x, y)
    if c == 1:
        same(want_scale, xb, "the restatement at c = 1")
    _axpy_family(ctx, c, xb, yb, want_axpy, want_scale, (ELL - 1,))


def test_axpy_tail_of_nothing(ctx, pools):
    """n = 0: out[0] = tail and nothing else; x may be NULL"""
    X, _ = pools
    dx = ctx.upload(X.b[:1])
    for tail in (0, 1, ELL - 1):
        for x_ptr, y_ptr in ((None, None), (dx.ptr, None), (dx.ptr, dx.ptr)):
            out = Guarded(ctx, 1)
            ctx.fr_axpy_tail(X.i[3], x_ptr, y_ptr, 0, tail, out.ptr)
            same(out.read(), _bytes([tail]), "the tail alone")


# ---- vmpc_fr_dot_dev, vmpc_fr_dot_to_dev -------------------------------------------------------------------------------------
def _dot_both(ctx, a_ptr, b_ptr, n):
    """the inner product through both entries; they must agree"""
    out = Guarded(ctx, 1)
    assert ctx.lib.vmpc_fr_dot_to_dev(ctx.handle, vp(a_ptr), vp(b_ptr), n, vp(out.ptr)) == 0
    host = ctx.fr_dot(a_ptr, b_ptr, n)
    dev = _ints(out.read())[0]
    assert host == dev, (hex(host), hex(dev))
    return host


@pytest.mark.parametrize("n", [0, 1, 65536, 65537, 524288, 524289, 524545])
def test_dot_and_dot_to_dev(ctx, pools, n):
    X, Y = pools
    if n == 0:
        assert _dot_both(ctx, None, None, 0) == 0           # 32 zero bytes over the pattern
        d = ctx.upload(X.b[:1])
        assert _dot_both(ctx, d.ptr, d.ptr, 0) == 0
        return
    (ab, a), (bb, b) = X.planted(n), Y.planted(n)
    da, db = ctx.upload(ab), ctx.upload(bb)
    assert _dot_both(ctx, da.ptr, db.ptr, n) == ref.dot(a, b), "random"
    if n == 1:
        return
    # every element l - 1: every accumulator and every partial at the largest products
    top = [ELL - 1] * n
    dt = ctx.upload(np.tile(_bytes([ELL - 1]), (n, 1)))
    assert _dot_both(ctx, dt.ptr, dt.ptr, n) == ref.dot(top, top) == n % ELL, "every element l - 1"
    assert _dot_both(ctx, dt.ptr, da.ptr, n) == ref.dot(top, a), "l - 1 against random"
    # one-hot pairs
    zero = np.zeros((n, 32), np.uint8)
    dza, dzb = ctx.upload(zero), ctx.upload(zero)
    assert _dot_both(ctx, dza.ptr, dzb.ptr, n) == 0
    for k in sorted({k for k in (0, 65536, 524288, n - 1) if k < n}):
        u, v = X.i[k + 1] | 1, Y.i[k + 1] | 1
        ctx.upload_into(dza.ptr + 32 * k, _bytes([u]))
        ctx.upload_into(dzb.ptr + 32 * k, _bytes([v]))
        assert _dot_both(ctx, dza.ptr, dzb.ptr, n) == u * v % ELL != 0, f"one-hot pair at {k}"
        # a alone at k against the random b: the one product a[k] b[k]
        assert _dot_both(ctx, dza.ptr, db.ptr, n) == u * b[k] % ELL, f"one-hot a at {k}"
        ctx.upload_into(dza.ptr + 32 * k, zero[:1])
        ctx.upload_into(dzb.ptr + 32 * k, zero[:1])


# ---- vmpc_fr_challenge_products_dev ------------------------------------------------------------------------------------------
def _challenges(pool, R, offset):
    cs = pool.i[offset:offset + R]
    if R:
        cs[0] = cs[-1] = ELL - 1
    return cs


def _challenge_products(ctx, cs, low_bits, zb):
    out = Guarded(ctx, 1 << (len(cs) + low_bits))
    dz = ctx.upload(zb)
    ctx.fr_challenge_products(cs, low_bits, dz.ptr, out.ptr)
    return out.read()


@pytest.mark.parametrize("rounds,low_bits", [(0, 0), (0, 4), (1, 0), (4, 0), (3, 5), (20, 0), (2, 18)])
def test_challenge_products(ctx, pools, rounds, low_bits):
    X, Y = pools
    cs = _challenges(Y, rounds, 5000)
    zb, z = X.planted(1 << low_bits, 77)
    table = ref.bit_products_by_halves(cs) if rounds > 10 else ref.bit_products(cs)
    want = ref.challenge_products(cs, low_bits, z, table)
    same(_challenge_products(ctx, cs, low_bits, zb), _bytes(want), f"challenge products {rounds, low_bits}")


def test_challenge_products_of_ones_and_of_a_zero(ctx, pools):
    X, Y = pools
    low_bits = 4
    zb, z = X.planted(1 << low_bits, 300)
    same(_challenge_products(ctx, [1, 1, 1], low_bits, zb), np.tile(zb, (8, 1)), "challenges 1: z repeated")
    cs = [Y.i[1], 0, Y.i[2]]
    got = _challenge_products(ctx, cs, low_bits, zb)
    same(got, _bytes(ref.challenge_products(cs, low_bits, z)), "a challenge 0")
    # round 1 looks at bit low_bits + 1: zero wherever that bit is 0, and nowhere else (z has no zero)
    assert all(v for v in z)
    assert [not row.any() for row in got] == [(j >> (low_bits + 1)) & 1 == 0 for j in range(len(got))]


# ---- vmpc_fr_tail_scalars_dev ------------------------------------------------------------------------------------------------
def _tail_direct(ctx, cs, log2_m0, zb):
    m0 = 1 << log2_m0
    a, b = Guarded(ctx, m0), Guarded(ctx, m0)
    dz = ctx.upload(zb)
    ctx.fr_tail_scalars(cs, log2_m0, dz.ptr, a.ptr, b.ptr)
    return a.read(), b.read()


@pytest.mark.parametrize("log2_m0,t", [(1, 0), (2, 1), (6, 5), (9, 0), (9, 8), (20, 1)])
def test_tail_scalars(ctx, pools, log2_m0, t):
    X, Y = pools
    cs = _challenges(Y, t, 6000)
    zb, z = X.planted((1 << log2_m0) >> t, 13)
    wa, wb = ref.tail_scalars(cs, log2_m0, z)
    ga, gb = _tail_direct(ctx, cs, log2_m0, zb)
    same(ga, _bytes(wa), "A")
    same(gb, _bytes(wb), "B")


# ---- vmpc_fr_tail_scalars_inc_dev, vmpc_fr_tail_scalars_block_dev --------------------------------------------------------------
def _expanded(table, log2_m0, j0=0, count=None):
    """products[j], j in [j0, j0 + count): the table entry of the top t bits of j"""
    t = len(table).bit_length() - 1
    count = (1 << log2_m0) - j0 if count is None else count
    return [table[j >> (log2_m0 - t)] for j in range(j0, j0 + count)]


def test_tail_scalars_inc_through_the_last_round(ctx, pools):
    X, Y = pools
    log2_m0 = 9
    m0 = 1 << log2_m0
    prod = Guarded(ctx, m0)
    cs = []
    for t in range(log2_m0):
        zb, z = X.planted(m0 >> t, 1000 * t)
        dz = ctx.upload(zb)
        a, b = Guarded(ctx, m0), Guarded(ctx, m0)
        ctx.fr_tail_scalars_inc(cs[-1] if cs else 0, t, log2_m0, dz.ptr, prod.ptr, a.ptr, b.ptr)
        ga, gb = a.read(), b.read()
        wa, wb = ref.tail_scalars(cs, log2_m0, z)
        same(ga, _bytes(wa), f"A, t = {t}")
        same(gb, _bytes(wb), f"B, t = {t}")
        same(prod.read(), _bytes(_expanded(ref.bit_products(cs), log2_m0)), f"products, t = {t}")
        da, db = _tail_direct(ctx, cs, log2_m0, zb)
        same(da, ga, f"A of the direct kernel, t = {t}")
        same(db, gb, f"B of the direct kernel, t = {t}")
        cs.append(ELL - 1 if t in (0, log2_m0 - 2) else Y.i[40 + t])


BLOCKS = [(0, 1), (1, 300), (300, 512), (512, 513), (513, 1024)]


def test_tail_scalars_blocks_equal_slices_of_the_whole(ctx, pools):
    X, Y = pools
    log2_m0 = 10
    bufs = [tuple(Guarded(ctx, j1 - j0) for _ in range(3)) for j0, j1 in BLOCKS]      # products, A, B per block
    cs = []
    for t in range(log2_m0):
        zb, z = X.planted((1 << log2_m0) >> t, 2000 * t + 5)
        dz = ctx.upload(zb)
        wa, wb = ref.tail_scalars(cs, log2_m0, z)
        wp = _expanded(ref.bit_products(cs), log2_m0)
        for (j0, j1), (prod, _, _) in zip(BLOCKS, bufs):
            if t == 0:
                assert prod.untouched()
            a, b = Guarded(ctx, j1 - j0), Guarded(ctx, j1 - j0)
            ctx.fr_tail_scalars_block(cs[-1] if cs else 0, t, log2_m0, dz.ptr, j0, j1 - j0, prod.ptr, a.ptr, b.ptr)
            same(a.read(), _bytes(wa[j0:j1]), f"A[{j0}:{j1}], t = {t}")
            same(b.read(), _bytes(wb[j0:j1]), f"B[{j0}:{j1}], t = {t}")
            same(prod.read(), _bytes(wp[j0:j1]), f"products[{j0}:{j1}], t = {t}")
            assert ref.tail_scalars_block(cs, log2_m0, z, j0, j1 - j0) == (wa[j0:j1], wb[j0:j1])
            if t == 0:
                same(prod.read(), _bytes([1] * (j1 - j0)), "t = 0 sets the products to 1")
        cs.append(ELL - 1 if t == 3 else Y.i[90 + t])


def test_tail_scalars_block_of_nothing(ctx, pools):
    X, _ = pools
    log2_m0 = 4
    dz = ctx.upload(X.b[:16])
    for j0 in (0, 5, 16):
        for t in (0, 2):
            g = [Guarded(ctx, 0) for _ in range(3)]
            ctx.fr_tail_scalars_block(X.i[9], t, log2_m0, dz.ptr, j0, 0, g[0].ptr, g[1].ptr, g[2].ptr)
            for x in g:
                x.read()


# ---- argument contracts: every case returns before a launch ------------------------------------------------------------------
NONCANON = [ELL, (1 << 256) - 1]


def test_axpy_refuses_non_canonical_constants(nat, ctx, pools):
    X, Y = pools
    n = 300
    lib, h = ctx.lib, ctx.handle
    dx, dy = ctx.upload(X.b[:n]), ctx.upload(Y.b[:n])
    for c in NONCANON:
        out = Guarded(ctx, n + 1)
        assert lib.vmpc_fr_axpy_dev(h, _sc(c), vp(dx.ptr), vp(dy.ptr), n, vp(out.ptr)) == nat.E_NONCANON
        assert lib.vmpc_fr_scale_dev(h, _sc(c), vp(dx.ptr), n, vp(out.ptr)) == nat.E_NONCANON
        assert lib.vmpc_fr_axpy_tail_dev(h, _sc(c), vp(dx.ptr), vp(dy.ptr), n, _sc(1), vp(out.ptr)) == nat.E_NONCANON
        assert lib.vmpc_fr_axpy_tail_dev(h, _sc(1), vp(dx.ptr), None, n, _sc(c), vp(out.ptr)) == nat.E_NONCANON
        assert lib.vmpc_fr_axpy_tail_dev(h, _sc(1), None, None, 0, _sc(c), vp(out.ptr)) == nat.E_NONCANON
        assert out.untouched()
    # the largest canonical values pass
    out = Guarded(ctx, n + 1)
    assert lib.vmpc_fr_axpy_tail_dev(h, _sc(ELL - 1), vp(dx.ptr), vp(dy.ptr), n, _sc(ELL - 1), vp(out.ptr)) == 0
    same(out.read(), _bytes(ref.axpy(ELL - 1, X.i[:n], Y.i[:n], ELL - 1)), "c = tail = l - 1")


def test_nothing_to_do_is_ok(nat, ctx):
    lib, h = ctx.lib, ctx.handle
    out = Guarded(ctx, 1)
    assert lib.vmpc_fr_axpy_dev(h, _sc(5), None, None, 0, None) == 0
    assert lib.vmpc_fr_axpy_dev(h, _sc(5), None, None, 0, vp(out.ptr)) == 0
    assert lib.vmpc_fr_scale_dev(h, _sc(5), None, 0, vp(out.ptr)) == 0
    assert out.untouched()
    host = ctypes.create_string_buffer(bytes([PAT_BYTE]) * 32, 32)
    assert lib.vmpc_fr_dot_dev(h, None, None, 0, host) == 0
    assert host.raw == bytes(32)


def test_challenge_products_contract(nat, ctx, pools):
    X, Y = pools
    lib, h = ctx.lib, ctx.handle
    fn = lib.vmpc_fr_challenge_products_dev
    dz = ctx.upload(X.b[:4])
    for rounds, n_alloc in ((3, 32), (20, 1 << 20)):
        for slot in (0, rounds - 1):
            cs = Y.i[:rounds]
            cs[slot] = ELL
            low_bits = 2 if rounds == 3 else 0
            out = Guarded(ctx, n_alloc)
            assert fn(h, _scs(cs), rounds, low_bits, vp(dz.ptr), n_alloc, vp(out.ptr)) == nat.E_NONCANON, (rounds, slot)
            assert out.untouched()
    # rounds = 21: one more than the argument array holds (the output would have 2^21 elements)
    out21 = ctx.alloc(32 << 21)
    assert fn(h, _scs(Y.i[:21]), 21, 0, vp(dz.ptr), 1 << 21, vp(out21.ptr)) == nat.E_INVAL
    assert fn(h, _scs(Y.i[:3]), -1, 0, vp(dz.ptr), 1, vp(out21.ptr)) == nat.E_INVAL
    # n is not 2^(rounds + low_bits)
    out = Guarded(ctx, 64)
    for n in (0, 31, 33, 16, 64):
        assert fn(h, _scs(Y.i[:3]), 3, 2, vp(dz.ptr), n, vp(out.ptr)) == nat.E_INVAL, n
    assert out.untouched()
    assert fn(h, _scs(Y.i[:3]), 3, 2, vp(dz.ptr), 32, vp(out.ptr)) == 0
    same(out.read()[:32], _bytes(ref.challenge_products(Y.i[:3], 2, X.i[:4])), "the accepted call")


def test_tail_scalars_contract(nat, ctx, pools):
    X, Y = pools
    lib, h = ctx.lib, ctx.handle
    direct, block, inc = lib.vmpc_fr_tail_scalars_dev, lib.vmpc_fr_tail_scalars_block_dev, lib.vmpc_fr_tail_scalars_inc_dev
    log2_m0 = 6
    m0 = 1 << log2_m0
    dz = ctx.upload(X.b[:m0])
    a, b, prod = Guarded(ctx, m0 + 1), Guarded(ctx, m0 + 1), Guarded(ctx, m0 + 1)
    z_, a_, b_, p_ = vp(dz.ptr), vp(a.ptr), vp(b.ptr), vp(prod.ptr)
    # a challenge equal to l: slot 0 and the last slot of the direct entry, the newest one of the round-by-round entries
    for slot in (0, 4):
        cs = Y.i[:5]
        cs[slot] = ELL
        assert direct(h, _scs(cs), 5, log2_m0, z_, a_, b_) == nat.E_NONCANON, slot
    for t in (1, 5):
        for c in NONCANON:
            assert block(h, _sc(c), t, log2_m0, z_, 3, 40, p_, a_, b_) == nat.E_NONCANON, t
            assert inc(h, _sc(c), t, log2_m0, z_, p_, a_, b_) == nat.E_NONCANON, t
    # t = log2_m0, log2_m0 = 0, a negative t
    for t, lg in ((log2_m0, log2_m0), (0, 0), (-1, log2_m0), (7, log2_m0)):
        assert direct(h, _scs(Y.i[:8]), t, lg, z_, a_, b_) == nat.E_INVAL, (t, lg)
        assert block(h, _sc(Y.i[0]), t, lg, z_, 0, 1, p_, a_, b_) == nat.E_INVAL, (t, lg)
        assert inc(h, _sc(Y.i[0]), t, lg, z_, p_, a_, b_) == nat.E_INVAL, (t, lg)
    # a block that ends one element past the vector
    for j0, count in ((0, m0 + 1), (1, m0), (m0, 1), (m0 + 1, 0)):
        assert block(h, _sc(Y.i[0]), 0, log2_m0, z_, j0, count, p_, a_, b_) == nat.E_INVAL, (j0, count)
    # j0 + count wraps to 0 and to 1: the lanes of an unchecked launch would stay inside the count elements of each
    # buffer and inside z, so a missing check is a wrong return code here and nothing worse
    for t in (0, 1):
        for j0, count in (((1 << 64) - 1, 1), ((1 << 64) - m0, m0 + 1)):
            assert block(h, _sc(Y.i[0]), t, log2_m0, z_, j0, count, p_, a_, b_) == nat.E_INVAL, (t, j0, count)
    assert a.untouched() and b.untouched() and prod.untouched()
    # the whole vector as one block and the last element alone are accepted
    assert block(h, _sc(0), 0, log2_m0, z_, 0, m0, p_, a_, b_) == 0
    wa, wb = ref.tail_scalars([], log2_m0, X.i[:m0])
    same(a.read()[:m0], _bytes(wa), "A of the accepted call")
    same(b.read()[:m0], _bytes(wb), "B of the accepted call")
    assert block(h, _sc(0), 0, log2_m0, z_, m0 - 1, 1, p_, a_, b_) == 0
    same(a.read()[:1], _bytes(wa[-1:]), "A of the last element alone")
    same(b.read()[:1], _bytes(wb[-1:]), "B of the last element alone")
    ctx.sync()
