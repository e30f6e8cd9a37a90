"""vmpc_bn256_scale_points_dev (csrc/bn256_scale.hip): out[i] = scalars[i] * points[i], byte for
byte against oracle/bn256_ref.py's affine group law on Python ints - both groups, element counts at the edges of the
kernel's 64-lane workgroup and past several of them, the scalars that take the chain through its special cases (0, 1, 2,
n - 1, n, n + 1, 2^255, 2^256 - 1: used as they stand, not reduced), infinity as a point, neighbouring lanes whose
chains differ in every bit, equal and distinct points side by side, the argument rules, and the independence of the
bytes from where in a launch - and in which launch - an element sits.

The n elements of a call repeat a pool of (point, scalar) pairs, so the reference computes each product once per group
and never changes it."""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn

pytestmark = pytest.mark.gpu
N = bn.N
TOP = (1 << 256) - 1
EDGE = [0, 1, 2, N - 1, N, N + 1, 1 << 255, TOP]
CURVE = {1: (bn.E1, bn.G1, bn.g1_to_bytes, 64), 2: (bn.E2, bn.G2, bn.g2_to_bytes, 128)}
LANES = 64                                            # SC_LANES of csrc/bn256_scale.hip: one workgroup
SIZES = [1, 63, 64, 65, 127, 128, 129, 257]


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as v
    return v.get_context()


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _bases(group):
    """four multiples of the generator that the tests know no relation between, and the negative of the first"""
    E, G = CURVE[group][:2]
    rng = random.Random(70 + group)
    pts = [E.mul(rng.randrange(1, N), G)]
    for _ in range(3):
        pts.append(E.add(E.add(pts[-1], pts[-1]), G))
    return pts + [E.neg(pts[0])]


@functools.lru_cache(maxsize=None)
def _pool(group):
    """(base index or None for infinity, scalar) pairs: every edge scalar on ONE point (equal points side by side), full
    256-bit and sub-order random scalars on distinct points, infinity under a zero, an edge and a random scalar, and 0 next
    to 2^256 - 1 on two points"""
    rng = random.Random(700 + group)
    pool = [(0, k) for k in EDGE]
    pool += [(b, rng.getrandbits(256) | 1 << 255) for b in (1, 2, 3, 4)]
    pool += [(b, rng.randrange(1, N)) for b in (0, 1, 2, 3)]
    pool += [(None, 0), (None, N - 1), (None, rng.getrandbits(256))]
    pool += [(1, 0), (1, TOP), (2, 0), (2, TOP), (4, N + 1), (4, N - 1)]
    return pool


@functools.lru_cache(maxsize=None)
def _want(group):
    """the pool's products as bytes: plain affine double-and-add on the integer as it stands"""
    E, _, enc, _ = CURVE[group]
    return [enc(None if b is None else E.mul(k, _bases(group)[b])) for b, k in _pool(group)]


def _point_bytes(group, b):
    return CURVE[group][2](None if b is None else _bases(group)[b])


def _scale(ctx, group, items, extra_out=2, poison=0x5A):
    """items: (base index, scalar) pairs -> (the products, the rest of the out buffer)"""
    width, n = CURVE[group][3], len(items)
    pts = np.frombuffer(b"".join(_point_bytes(group, b) for b, _ in items), np.uint8).reshape(n, width)
    sc = np.frombuffer(b"".join(k.to_bytes(32, "little") for _, k in items), np.uint8).reshape(n, 32)
    d_p, d_s = ctx.upload(pts), ctx.upload(sc)
    out = ctx.upload(np.full((n + extra_out, width), poison, np.uint8))
    ctx.bn256_scale_points(group, d_p.ptr, d_s.ptr, n, out.ptr)
    ctx.sync()
    got = ctx.download(out.ptr, width * (n + extra_out), (n + extra_out, width))
    return [g.tobytes() for g in got[:n]], got[n:]


@pytest.mark.parametrize("group", [1, 2])
def test_against_the_affine_group_law(ctx, group):
    pool, want = _pool(group), _want(group)
    for n in SIZES:
        got, rest = _scale(ctx, group, [pool[i % len(pool)] for i in range(n)])
        for i in range(n):
            assert got[i] == want[i % len(pool)], (n, i, pool[i % len(pool)])
        assert (rest == 0x5A).all(), n                               # out beyond n untouched


@pytest.mark.parametrize("group", [1, 2])
def test_the_named_edges_are_in_the_pool(group):
    """what the edge scalars have to give, stated on the reference: they are the pool's first eight entries"""
    E, _, enc, width = CURVE[group]
    P = _bases(group)[0]
    want = _want(group)
    assert [k for _, k in _pool(group)[:8]] == EDGE
    inf = bytes(width)
    assert want[0] == inf and want[1] == enc(P) and want[2] == enc(E.add(P, P))
    assert want[3] == enc(E.neg(P)) and want[4] == inf and want[5] == enc(P)
    assert want[6] == enc(E.mul((1 << 255) % N, P)) and want[7] == enc(E.mul(TOP % N, P))
    assert all(want[i] == inf for i, (b, _) in enumerate(_pool(group)) if b is None)      # infinity stays infinity


@pytest.mark.parametrize("group", [1, 2])
def test_divergent_neighbours_in_one_wavefront(ctx, group):
    """lanes 2j at scalar 0 and 2j + 1 at 2^256 - 1 on the same point, a whole wavefront and one lane more: every bit
    differs between neighbours, the accumulator of the even lanes never leaves infinity"""
    E, _, enc, width = CURVE[group]
    pool, want = _pool(group), _want(group)
    zero, top = pool.index((1, 0)), pool.index((1, TOP))
    got, _ = _scale(ctx, group, [pool[top if i & 1 else zero] for i in range(LANES + 1)])
    assert got == [want[top] if i & 1 else bytes(width) for i in range(LANES + 1)]


@pytest.mark.parametrize("group", [1, 2])
def test_bytes_do_not_depend_on_the_order_or_the_launch(ctx, group):
    """the same 129 inputs in their order, in a shuffled order and as two launches of 64 and 65: the same bytes"""
    pool = _pool(group)
    items = [pool[i % len(pool)] for i in range(129)]
    first, _ = _scale(ctx, group, items)
    perm = list(range(129))
    random.Random(9).shuffle(perm)
    shuffled, _ = _scale(ctx, group, [items[j] for j in perm])
    back = [None] * 129
    for pos, j in enumerate(perm):
        back[j] = shuffled[pos]
    assert back == first
    assert _scale(ctx, group, items[:64])[0] + _scale(ctx, group, items[64:])[0] == first


def test_argument_rules(ctx, nat):
    f, h = ctx.lib.vmpc_bn256_scale_points_dev, ctx.handle
    p = ctypes.c_void_p
    pts, sc, out = ctx.upload(np.zeros((4, 128), np.uint8)), ctx.upload(np.zeros((4, 32), np.uint8)), ctx.alloc(128 * 4)
    # (group, points, scalars, n, out): VMPC_E_RANGE before the group or any pointer is looked at
    assert f(h, 1, None, None, (1 << 31) + 1, None) == nat.E_RANGE
    assert f(h, 7, None, None, (1 << 31) + 1, None) == nat.E_RANGE
    # VMPC_E_INVAL: another group (with n = 0 too), a null pointer where there is work
    for group in (0, 3, -1):
        assert f(h, group, p(pts.ptr), p(sc.ptr), 4, p(out.ptr)) == nat.E_INVAL
        assert f(h, group, None, None, 0, None) == nat.E_INVAL
    assert f(None, 1, p(pts.ptr), p(sc.ptr), 4, p(out.ptr)) == nat.E_INVAL
    for group in (1, 2):
        assert f(h, group, None, p(sc.ptr), 4, p(out.ptr)) == nat.E_INVAL
        assert f(h, group, p(pts.ptr), None, 4, p(out.ptr)) == nat.E_INVAL
        assert f(h, group, p(pts.ptr), p(sc.ptr), 4, None) == nat.E_INVAL
    # n = 0: VMPC_OK, nothing launched (the null pointers would fault a launch)
    ctx.profile(True)
    try:
        ctx.profile_read()
        assert f(h, 1, None, None, 0, None) == nat.OK
        assert f(h, 2, None, None, 0, None) == nat.OK
        ctx.sync()
        assert all(count == 0 for _, count in ctx.profile_read().values())
        # n = 2^31 itself is inside the range: the null pointers are the error, and nothing is launched
        assert f(h, 1, None, None, 1 << 31, None) == nat.E_INVAL
        ctx.sync()
        assert all(count == 0 for _, count in ctx.profile_read().values())
    finally:
        ctx.profile(False)
