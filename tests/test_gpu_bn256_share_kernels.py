"""csrc/mpc_share.hip's GF(n) entries and vmpc_bn256_qap_residual_dev through the C ABI, bit for bit against
tests/trinocchio_ref.py: the dealing kernel at its loop edges, party counts and degrees (a degree 2t = M - 1 dealing of
zeros included), the combination at the accumulator's worst case - every part and weight n - 1 at 1, 3, 4 (the first
count whose plain 512-bit sum overflows) and 64 parties - with its scatter and its addend, the refusals, and the
residual across its geometry.

The residual runs workgroups of 256 lanes, at most 64 of them; beyond 64 x 256 = 16384 rows a lane takes several rows
(its power of rho advanced by rho^16384) and the second pass adds one partial per workgroup.  So d crosses 64 (a
wavefront), 256 (one workgroup, one partial), 1025 (five partials) as the issue lists them, and in addition 16384 /
16385 / 16641 (the lane loop: the 64-workgroup cap, one row past it, one workgroup and a row past it)."""
import ctypes
import random

import numpy as np
import pytest

from tests import trinocchio_ref as tr

pytestmark = pytest.mark.gpu
N = tr.N


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def ctx(vm):
    return vm.get_context()


def arr(vals):
    from verifiable_mpc_amd import _native
    return _native.ints_to_array(list(vals), 32)


def up(vm, vals):
    return vm.ScalarVector.from_array(arr(vals))


def values(rng, n):
    """0, 1 and n - 1 among random residues"""
    special = [0, 1, N - 1, N - 1, 1, 0]
    return [special[i % 6] if i % 3 == 0 else rng.randrange(N) for i in range(n)]


# ---- vmpc_bn256_fr_share_mul_deal_dev --------------------------------------------------------------------------------
@pytest.mark.parametrize("parties,t", [(1, 0), (3, 1), (5, 2), (5, 4), (64, 31)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("with_b", [False, True])
def test_mul_deal(vm, ctx, parties, t, n, with_b):
    rng = random.Random(1000 * parties + 10 * t + n)
    a, b = values(rng, n), values(rng, n)[::-1] if with_b else None
    coeffs = [values(rng, n) for _ in range(t)]
    want = tr.mul_deal(a, b, coeffs, parties)
    da, db = up(vm, a), up(vm, b) if with_b else None
    dc = up(vm, [v for row in coeffs for v in row]) if t else None
    stride = n + 3                                          # rows further apart than they are long
    out = up(vm, [5] * (parties * stride))
    ctx.bn256_share_mul_deal(da.ptr, db.ptr if with_b else None, n, dc.ptr if t else None, t, parties, out.ptr, stride)
    ctx.sync()
    got = out.to_ints()
    for q in range(parties):
        assert got[q * stride:q * stride + n] == want[q], (q,)
        assert got[q * stride + n:(q + 1) * stride] == [5] * 3       # the padding of every row is left alone


@pytest.mark.parametrize("parties,t", [(3, 1), (5, 2)])
def test_mul_deal_of_zeros_with_degree_2t_shares_zero(vm, ctx, parties, t):
    """a all zeros, the degree argument 2t: every column is a degree-2t sharing of 0 (and is not all zero)"""
    n = 65
    rng = random.Random(parties)
    coeffs = [[rng.randrange(N) for _ in range(n)] for _ in range(2 * t)]
    out = vm.ScalarVector.empty(parties * n)
    da, dc = up(vm, [0] * n), up(vm, [v for row in coeffs for v in row])
    ctx.bn256_share_mul_deal(da.ptr, None, n, dc.ptr, 2 * t, parties, out.ptr, n)
    ctx.sync()
    got = out.to_ints()
    assert got == [v for row in tr.mul_deal([0] * n, None, coeffs, parties) for v in row]
    for i in range(n):
        col = [got[q * n + i] for q in range(parties)]
        assert tr.recombine(col) == 0 and any(col)


def test_mul_deal_refusals(vm, ctx):
    from verifiable_mpc_amd import _native
    lib, null, p = ctx.lib, ctypes.c_void_p(None), ctypes.c_void_p
    assert lib.vmpc_bn256_fr_share_mul_deal_dev(ctx.handle, null, null, 1, null, 0, 65, null, 1) == _native.E_RANGE
    x = up(vm, [1])
    # t < parties, out_stride >= n
    assert lib.vmpc_bn256_fr_share_mul_deal_dev(ctx.handle, p(x.ptr), null, 1, p(x.ptr), 3, 3, p(x.ptr), 1) == \
        _native.E_INVAL
    assert lib.vmpc_bn256_fr_share_mul_deal_dev(ctx.handle, p(x.ptr), null, 2, null, 0, 1, p(x.ptr), 1) == _native.E_INVAL


# ---- vmpc_bn256_fr_share_combine_dev ---------------------------------------------------------------------------------
def _run_combine(vm, ctx, parts, wts, n, scatter, with_addend, rng):
    parties, stride = len(parts), n + 1
    flat = []
    for row in parts:
        flat += row + [9]
    dp = up(vm, flat)
    if scatter:
        dst = list(range(0, 2 * n, 2))                   # every other position of an output twice as long
        rng.shuffle(dst)
        before = [7] * (2 * n)
        dd = ctx.upload(np.asarray(dst, np.uint32))
    else:
        dst, before, dd = None, [7] * n, None
    addend = values(rng, n) if with_addend else None
    da = up(vm, addend) if with_addend else None
    out = up(vm, before)
    ctx.bn256_share_combine(dp.ptr, parties, n, stride, wts, dd.ptr if scatter else None, da.ptr if with_addend else None,
                            out.ptr)
    ctx.sync()
    assert out.to_ints() == tr.combine(parts, wts, dst, before, addend)    # positions no dst names stay 7


@pytest.mark.parametrize("parties", [1, 3, 4, 64])
@pytest.mark.parametrize("with_addend", [False, True])
def test_combine_worst_case(vm, ctx, parties, with_addend):
    """every part and every weight n - 1: parties (n - 1)^2 passes 2^512 from four parties on"""
    n = 65
    assert ((parties * (N - 1) ** 2).bit_length() > 512) == (parties >= 4)
    _run_combine(vm, ctx, [[N - 1] * n for _ in range(parties)], [N - 1] * parties, n, False, with_addend,
                 random.Random(parties))


@pytest.mark.parametrize("parties", [1, 3, 4, 64])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_combine_random(vm, ctx, parties, n):
    rng = random.Random(100 * parties + n)
    for scatter, with_addend in ((False, False), (True, True), (True, False), (False, True)):
        _run_combine(vm, ctx, [values(rng, n) for _ in range(parties)], values(rng, parties), n, scatter, with_addend,
                     rng)


def test_combine_addend_above_n_is_taken_mod_n(vm, ctx):
    out, part, addend = up(vm, [7]), up(vm, [5]), up(vm, [(1 << 256) - 1])
    ctx.bn256_share_combine(part.ptr, 1, 1, 1, [3], None, addend.ptr, out.ptr)
    ctx.sync()
    assert out.to_ints() == [(15 + (1 << 256) - 1) % N]


def test_combine_refuses_what_is_not_canonical(vm, ctx):
    from verifiable_mpc_amd import _native
    parts = up(vm, [1, 2, 3, 4])
    out = up(vm, [7, 7])
    # a weight: checked on the host, at once, nothing written
    with pytest.raises(_native.VmpcError) as e:
        ctx.bn256_share_combine(parts.ptr, 2, 2, 2, [1, N], None, None, out.ptr)
    assert e.value.code == _native.E_NONCANON
    ctx.sync()
    assert out.to_ints() == [7, 7]
    # an element of parts: seen by the kernel, its output is not written, the next synchronisation reports it
    bad = up(vm, [1, 2, 3, N])
    ctx.bn256_share_combine(bad.ptr, 2, 2, 2, [1, 1], None, None, out.ptr)
    with pytest.raises(_native.VmpcError) as e:
        ctx.sync()
    assert e.value.code == _native.E_NONCANON
    assert out.to_ints() == [4, 7]
    ctx.sync()                                              # reported once


def test_combine_caps_and_stride(vm, ctx):
    from verifiable_mpc_amd import _native
    null, p = ctypes.c_void_p(None), ctypes.c_void_p
    fn = ctx.lib.vmpc_bn256_fr_share_combine_dev
    assert fn(ctx.handle, null, 65, 1, 1, null, null, null, null) == _native.E_RANGE      # looks at no pointer
    x = up(vm, [1, 2])
    w = ctypes.create_string_buffer((1).to_bytes(32, "little"), 32)
    assert fn(ctx.handle, p(x.ptr), 1, 2, 1, w, null, null, p(x.ptr)) == _native.E_INVAL   # stride < n


# ---- vmpc_bn256_qap_residual_dev -------------------------------------------------------------------------------------
RES_D = [1, 63, 64, 65, 255, 256, 257, 1025, 16384, 16385, 16641]


def _residual(vm, ctx, a, b, y, rho):
    out, da, db, dy = up(vm, [7]), up(vm, a), up(vm, b), up(vm, y)
    ctx.bn256_qap_residual(da.ptr, db.ptr, dy.ptr, len(a), rho, out.ptr)
    ctx.sync()
    return out.to_ints()[0]


@pytest.fixture(scope="module")
def triples():
    """per d: a satisfying triple (a, b, y = a b), made once"""
    out = {}
    for d in RES_D:
        rng = random.Random(d)
        a, b = values(rng, d), values(rng, d)[::-1]
        out[d] = (a, b, [x * z % N for x, z in zip(a, b)])
    return out


@pytest.mark.parametrize("d", RES_D)
def test_residual(vm, ctx, triples, d):
    a, b, y = triples[d]
    rng = random.Random(7 * d)
    for rho in (0, 1, N - 1, rng.randrange(N)):
        assert _residual(vm, ctx, a, b, y, rho) == 0                      # a satisfying triple
        for j in sorted({1, d}):                                          # one violated row, first and last
            bad = list(y)
            bad[j - 1] = (bad[j - 1] + 1 + rng.randrange(N - 1)) % N
            want = tr.residual(a, b, bad, rho)
            assert want != 0 or (rho == 0 and j > 1)                      # (rho = 0 sees only the first row)
            assert _residual(vm, ctx, a, b, bad, rho) == want
        # nothing satisfied: random y
        ry = [rng.randrange(N) for _ in range(d)]
        assert _residual(vm, ctx, a, b, ry, rho) == tr.residual(a, b, ry, rho)


@pytest.mark.parametrize("d", [1, 257, 16385])
def test_residual_all_operands_n_minus_1(vm, ctx, d):
    v = [N - 1] * d
    for rho in (1, N - 1):
        want = tr.residual(v, v, v, rho)
        assert _residual(vm, ctx, v, v, v, rho) == want
    assert tr.residual(v, v, v, 1) == 2 * d % N                          # (n-1)^2 - (n-1) = 2 mod n, d times


def test_residual_refusals(vm, ctx):
    from verifiable_mpc_amd import _native
    x = up(vm, [1])
    with pytest.raises(_native.VmpcError) as e:
        ctx.bn256_qap_residual(x.ptr, x.ptr, x.ptr, 1, N, x.ptr)
    assert e.value.code == _native.E_NONCANON
    null = ctypes.c_void_p(None)
    fn = ctx.lib.vmpc_bn256_qap_residual_dev
    assert fn(ctx.handle, null, null, null, _native.BN256_FR_POLY_MAX, null, null) == _native.E_RANGE
    assert fn(ctx.handle, null, null, null, 1, null, null) == _native.E_INVAL
    ctx.sync()
    assert x.to_ints() == [1]
