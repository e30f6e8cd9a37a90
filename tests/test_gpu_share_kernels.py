"""csrc/mpc_share.hip and vmpc_fr_cs_extend_fg_dev through the C ABI, bit for bit against tests/share_ref.py: the
dealing / product kernel at its loop edges and party counts, the combination at the accumulator's worst case (every
operand and weight l - 1, 64 parties), its scatter, its refusals, and the split extension of f and g against both the
reference and what vmpc_fr_cs_extend_dev multiplies into z."""
import ctypes
import random

import numpy as np
import pytest

from tests import share_ref as sh

pytestmark = pytest.mark.gpu
ELL = sh.ELL


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
    return _native.ints_to_array([v for v in vals], 32)


def up(vm, vals):
    return vm.ScalarVector.from_array(arr(vals))


def values(rng, n):
    """0, 1 and l - 1 among random residues"""
    special = [0, 1, ELL - 1, ELL - 1, 1, 0]
    return [special[i % 6] if i % 3 == 0 else rng.randrange(ELL) for i in range(n)]


# ---- vmpc_fr_share_mul_deal_dev ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parties,t", [(1, 0), (3, 1), (5, 2), (64, 31)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("with_b", [False, True])
def test_mul_deal(vm, ctx, parties, t, n, with_b):
    rng = random.Random(1000 * parties + n)
    a, b = values(rng, n), values(rng, n)[::-1] if with_b else None
    coeffs = [values(rng, n) for _ in range(t)]
    want = sh.mul_deal(a, b, coeffs, parties)
    da, db = up(vm, a), up(vm, b) if with_b else None
    dc = up(vm, [v for row in coeffs for v in row]) if t else None
    stride = n + 3                                          # rows further apart than they are long
    out = vm.ScalarVector.from_array(arr([5] * (parties * stride)))
    ctx.share_mul_deal(da.ptr, db.ptr if with_b else None, n, dc.ptr if t else None, t, parties, out.ptr, stride)
    ctx.sync()
    got = out.to_ints()
    for q in range(parties):
        assert got[q * stride:q * stride + n] == want[q], (q,)
        if q < parties - 1:
            assert got[q * stride + n:(q + 1) * stride] == [5] * 3       # the gap between rows is left alone


def test_mul_deal_refusals(vm, ctx):
    from verifiable_mpc_amd import _native
    lib, null = ctx.lib, ctypes.c_void_p(None)
    assert lib.vmpc_fr_share_mul_deal_dev(ctx.handle, null, null, 1, null, 0, 65, null, 1) == _native.E_RANGE
    x = up(vm, [1])
    p = ctypes.c_void_p
    # t < parties, out_stride >= n
    assert lib.vmpc_fr_share_mul_deal_dev(ctx.handle, p(x.ptr), null, 1, p(x.ptr), 3, 3, p(x.ptr), 1) == _native.E_INVAL
    assert lib.vmpc_fr_share_mul_deal_dev(ctx.handle, p(x.ptr), null, 2, null, 0, 1, p(x.ptr), 1) == _native.E_INVAL


# ---- vmpc_fr_share_combine_dev ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parties", [1, 2, 64])
@pytest.mark.parametrize("scatter", [False, True])
def test_combine_worst_case_and_scatter(vm, ctx, parties, scatter):
    """every operand and every weight l - 1: parties * (l - 1)^2, the largest sum the 16-limb accumulator meets; then
    random operands"""
    n = 257
    rng = random.Random(parties)
    for parts, wts in (([[ELL - 1] * n for _ in range(parties)], [ELL - 1] * parties),
                       ([values(rng, n) for _ in range(parties)], values(rng, parties))):
        stride = n + 1
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
        out = up(vm, before)
        ctx.share_combine(dp.ptr, parties, n, stride, wts, dd.ptr if scatter else None, out.ptr)
        ctx.sync()
        assert out.to_ints() == sh.combine(parts, wts, dst, before)    # positions no dst names stay 7


def test_combine_refuses_what_is_not_canonical(vm, ctx):
    from verifiable_mpc_amd import _native
    parts = up(vm, [1, 2, 3, 4])
    out = up(vm, [7, 7])
    # a weight: checked on the host, at once
    with pytest.raises(_native.VmpcError) as e:
        ctx.share_combine(parts.ptr, 2, 2, 2, [1, ELL], None, out.ptr)
    assert e.value.code == _native.E_NONCANON
    # an element of parts: seen by the kernel, its output is not written, the next synchronisation reports it
    bad = up(vm, [1, 2, 3, ELL])
    ctx.share_combine(bad.ptr, 2, 2, 2, [1, 1], None, out.ptr)
    with pytest.raises(_native.VmpcError) as e:
        ctx.sync()
    assert e.value.code == _native.E_NONCANON
    assert out.to_ints() == [4, 7]
    ctx.sync()                                              # reported once


def test_combine_above_the_cap_looks_at_no_pointer(vm, ctx):
    from verifiable_mpc_amd import _native
    null = ctypes.c_void_p(None)
    assert ctx.lib.vmpc_fr_share_combine_dev(ctx.handle, null, 65, 1, 1, null, null, null) == _native.E_RANGE


# ---- vmpc_fr_cs_extend_fg_dev -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 64, 65, 257])
def test_extend_fg(vm, ctx, m):
    rng = random.Random(m)
    a, b = values(rng, m + 1), values(rng, m + 1)[::-1]
    K = 2 * m + 1
    fact, ifact = vm.ScalarVector.empty(K + 1), vm.ScalarVector.empty(K + 1)
    ctx.cs_tables(K, fact.ptr, ifact.ptr)
    da, db = up(vm, a), up(vm, b)
    f, g = up(vm, [5] * (m + 1)), up(vm, [5] * (m + 1))     # one element more than is written
    ctx.cs_extend_fg(da.ptr, db.ptr, m, fact.ptr, ifact.ptr, f.ptr, g.ptr)
    want_f, want_g = sh.extend_fg(a, b)
    got_f, got_g = f.to_ints(), g.to_ints()
    assert got_f == want_f + [5] and got_g == want_g + [5]
    # the unsplit entry multiplies the same values into z's tail
    tail = up(vm, [3] * (3 + 2 * m))
    ctx.cs_extend(da.ptr, db.ptr, m, fact.ptr, ifact.ptr, tail.ptr)
    t = tail.to_ints()
    assert t[:3] == [got_f[0], got_g[0], got_f[0] * got_g[0] % ELL]
    assert t[3:3 + m] == [3] * m and t[3 + m] == a[m] * b[m] % ELL
    assert t[4 + m:] == [x * y % ELL for x, y in zip(got_f[1:m], got_g[1:m])]
