"""vmpc_bn256_recombine_dev (csrc/bn256_recombine.hip): out[e] = sum_p weights[p] parts[p][e], byte
for byte against oracle/bn256_ref.py's affine group law on Python ints - both groups, 1 to 5 parties, element counts at
the edges of a wavefront and of a workgroup's 64 elements and past one workgroup, every weight set that takes another
path on the host or in the kernel (full-size, the real Lagrange weights, n - 1 which travels as -1, a zero, the pairs that
make the addition a doubling or give infinity), infinity as a part, strides with poisoned padding, and the argument rules.

The n elements of a call repeat a pool of at most 16 lists of parts, so the reference computes 16 sums per weight set
and its scalar multiples are shared: made once per (group, M), never changed."""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import keygen_ref as K
from tests import trinocchio_ref as tr

pytestmark = pytest.mark.gpu
N = bn.N
CURVE = {1: (bn.E1, bn.G1, bn.g1_to_bytes, 64), 2: (bn.E2, bn.G2, bn.g2_to_bytes, 128)}
SIZES = [1, 63, 64, 65, 257]


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
def nat():
    from verifiable_mpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _bases(group):
    """five points: four multiples of the generator that the tests know no relation between, and the negative of the first"""
    E, G = CURVE[group][:2]
    rng = random.Random(40 + group)
    pts = [E.mul(rng.randrange(1, N), G)]
    for _ in range(3):
        pts.append(E.add(E.add(pts[-1], pts[-1]), G))
    return pts + [E.neg(pts[0])]


@functools.lru_cache(maxsize=None)
def _multiple(group, w, b):
    return CURVE[group][0].mul(w, _bases(group)[b])


def _pool(M):
    """lists of M parts as indices into _bases (None: infinity)"""
    mid = M // 2
    pool = [[p % 4 for p in range(M)], [(p + 1) % 4 for p in range(M)], [(3 * p + 2) % 4 for p in range(M)],
            [None] * M, [0] * M, [1] * M, [4 if p % 2 else 0 for p in range(M)]]
    for at in sorted({0, mid, M - 1}):
        pool.append([None if p == at else (p + 2) % 4 for p in range(M)])
        pool.append([0 if p == at else None for p in range(M)])
    assert len(pool) <= 16
    return pool


def _weight_sets(M):
    rng = random.Random(7 * M)
    full = [rng.randrange(N >> 1, N) for _ in range(M)]
    sets = {"full": full, "lagrange": tr.weights(list(range(1, M + 1))), "n-1": [N - 1] * M,
            "zero": [0 if p == M // 2 else w for p, w in enumerate(full)], "ones": [1] * M}
    if M == 2:
        sets["1,n-1"] = [1, N - 1]
    return sets


@functools.lru_cache(maxsize=None)
def _reference(group, M):
    """weight set -> (weights, the pool's expected sums as bytes)"""
    E, _, enc, _ = CURVE[group]
    out = {}
    for name, wts in _weight_sets(M).items():
        sums = []
        for entry in _pool(M):
            acc = None
            for p, b in enumerate(entry):
                if b is not None:
                    acc = E.add(acc, _multiple(group, wts[p], b))
            sums.append(enc(acc))
        out[name] = (wts, sums)
    return out


def _part_bytes(group, b):
    return CURVE[group][2](None if b is None else _bases(group)[b])


def _run(ctx, group, M, n, wts, stride, poison=0xA5, extra_out=2):
    """-> (the n results, the rest of the out buffer)"""
    width, pool = CURVE[group][3], _pool(M)
    host = np.full((M, stride, width), poison, np.uint8)
    for p in range(M):
        for e in range(n):
            host[p, e] = np.frombuffer(_part_bytes(group, pool[e % len(pool)][p]), np.uint8)
    parts = ctx.upload(host)
    out = ctx.upload(np.full((n + extra_out, width), 0x5A, np.uint8))
    ctx.bn256_recombine(group, parts.ptr, M, n, stride, wts, out.ptr)
    ctx.sync()
    got = ctx.download(out.ptr, width * (n + extra_out), (n + extra_out, width))
    return got[:n], got[n:]


@pytest.mark.parametrize("M", [1, 2, 3, 5])
@pytest.mark.parametrize("group", [1, 2])
def test_against_the_affine_group_law(ctx, group, M):
    pool = _pool(M)
    for name, (wts, sums) in _reference(group, M).items():
        for n in SIZES:
            got, rest = _run(ctx, group, M, n, wts, n)
            for e in range(n):
                assert got[e].tobytes() == sums[e % len(pool)], (name, n, e, pool[e % len(pool)])
            assert (rest == 0x5A).all(), (name, n)                   # out beyond n untouched


def test_the_named_edges_are_in_the_pool():
    """the doubling, the cancellation and the all-infinity element are what the pool and the weight sets produce"""
    E = bn.E1
    ref = _reference(1, 2)
    pool = _pool(2)
    same, opposite = pool.index([0, 0]), pool.index([0, 4])
    P = _bases(1)[0]
    assert ref["ones"][1][same] == bn.g1_to_bytes(E.add(P, P))          # weights (1, 1), parts (P, P): a doubling
    assert ref["1,n-1"][1][same] == bytes(64)                           # weights (1, n - 1), parts (P, P): infinity
    assert ref["ones"][1][opposite] == bytes(64)                        # a part equal to the other's negative
    assert ref["full"][1][pool.index([None, None])] == bytes(64)
    assert ref["lagrange"][0] == [2, N - 1] and _reference(1, 3)["lagrange"][0] == [3, N - 3, 1]


@pytest.mark.parametrize("group", [1, 2])
def test_stride_with_poisoned_padding(ctx, group):
    """rows wider than n, the padding bytes that are no point of the curve: not read into any result"""
    for M in (2, 3):
        wts, sums = _reference(group, M)["full"]
        for n in (1, 65):
            got, rest = _run(ctx, group, M, n, wts, n + 3)
            assert [g.tobytes() for g in got] == [sums[e % len(sums)] for e in range(n)]
            assert (rest == 0x5A).all()


@pytest.mark.parametrize("group", [1, 2])
def test_equals_msm_on_columns(pn, ctx, group):
    """a column of the table through pynocchio.msm (the general path, what trinocchio.prove ran before): the same bytes"""
    cls = pn.BN256Point if group == 1 else pn.BN256TwistPoint
    M = 3
    pool = _pool(M)
    for name in ("full", "lagrange"):
        wts, sums = _reference(group, M)[name]
        for e in (0, 1, pool.index([0, 0, 0])):
            column = [cls.from_bytes(_part_bytes(group, b)) for b in pool[e]]
            assert pn.msm(wts, column, ctx).to_bytes() == sums[e], (name, e)


def test_argument_rules(ctx, nat):
    f, h = ctx.lib.vmpc_bn256_recombine_dev, ctx.handle
    one = ctypes.create_string_buffer(K.to_array([1] * 65).tobytes(), 32 * 65)
    buf = ctx.upload(np.zeros((3, 4, 64), np.uint8))
    out = ctx.alloc(64 * 4)
    p = ctypes.c_void_p
    # (group, parts, parties, n, part_stride, weights, out): VMPC_E_RANGE before any pointer is looked at
    assert f(h, 1, None, 65, 1, 1, None, None) == nat.E_RANGE
    assert f(h, 1, None, 3, (1 << 31) + 1, (1 << 31) + 1, None, None) == nat.E_RANGE
    assert f(h, 1, None, 3, 1, (1 << 31) + 1, None, None) == nat.E_RANGE
    # VMPC_E_NONCANON at once, with nothing to do included
    wn = ctypes.create_string_buffer(K.to_array([1, N, 1]).tobytes(), 96)
    assert f(h, 1, p(buf.ptr), 3, 4, 4, wn, p(out.ptr)) == nat.E_NONCANON
    assert f(h, 1, None, 3, 0, 0, wn, None) == nat.E_NONCANON
    # VMPC_E_INVAL
    assert f(h, 1, p(buf.ptr), 3, 4, 3, one, p(out.ptr)) == nat.E_INVAL          # part_stride < n
    assert f(h, 3, p(buf.ptr), 3, 4, 4, one, p(out.ptr)) == nat.E_INVAL          # group
    assert f(h, 0, p(buf.ptr), 3, 4, 4, one, p(out.ptr)) == nat.E_INVAL
    assert f(h, 1, p(buf.ptr), 0, 4, 4, one, p(out.ptr)) == nat.E_INVAL          # no party, work
    assert f(h, 1, None, 3, 4, 4, one, p(out.ptr)) == nat.E_INVAL                # null pointers, work
    assert f(h, 1, p(buf.ptr), 3, 4, 4, one, None) == nat.E_INVAL
    assert f(h, 1, p(buf.ptr), 3, 4, 4, None, p(out.ptr)) == nat.E_INVAL
    # n = 0: VMPC_OK, nothing launched (the null pointers would fault a launch)
    ctx.profile(True)
    try:
        ctx.profile_read()
        assert f(h, 1, None, 3, 0, 0, one, None) == nat.OK
        assert f(h, 2, None, 0, 0, 5, None, None) == nat.OK
        ctx.sync()
        assert all(count == 0 for _, count in ctx.profile_read().values())
    finally:
        ctx.profile(False)
