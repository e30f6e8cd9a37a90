"""vmpc_bn256_fr_cs_extend_fg_dev (csrc/circuit_sat.hip: cs_extend<frbn> with f_out / g_out), the share form of Protocol 8's
extension over GF(n): f(0), f(m+2 .. 2m) and g alike, kept apart and unmultiplied.  Against tests/p8_field_ref.py at
p = n - the interpolating polynomials evaluated naively, and the products against the barycentric z tail - at m on both
sides of 1, of 2 (the first m with a correlation) and of VMPC_FR_CS_EXT_NTT_MIN = 64; the NTT route against the direct
one bit for bit; words >= n; and on Shamir shares, where linearity is what the M-party prover uses."""
import ctypes
import random

import numpy as np
import pytest

from tests import mpc_koe_ref as mref
from tests import p8_field_ref as fref

pytestmark = pytest.mark.gpu

N = fref.BN_N
F = fref.P8(N)
FG_M = [0, 1, 2, 3, 63, 64, 65]
PAT_BYTE = 0xA5
PAT = int.from_bytes(bytes([PAT_BYTE]) * 32, "little")      # above n: no kernel here can write it


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as vm
    return vm.get_context()


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _ints(a):
    raw = a.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _inputs(m):
    rng = random.Random(9300 + m)
    return [rng.randrange(N) for _ in range(m + 1)], [rng.randrange(N) for _ in range(m + 1)]


def _points(m):
    """where f_out / g_out hold their polynomial: 0, then m+2 .. 2m"""
    return [0] + list(range(m + 2, 2 * m + 1))


def _extend_fg(ctx, m, a, b, mode):
    """-> (f_out, g_out) with one scalar of the fill pattern after each"""
    from verifiable_mpc_amd import device
    fact, ifact = (ctx.upload(_bytes(t)) for t in F.tables(max(2 * m + 1, 1)))
    d_a, d_b = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
    k = max(m, 1)
    f, g = (ctx.upload(np.full((k + 1, 32), PAT_BYTE, np.uint8)) for _ in range(2))
    with device.cs_extension(mode, ctx):
        ctx.cs_extend_fg(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, f.ptr, g.ptr, bn=True)
    ctx.sync()
    return _ints(ctx.download(f.ptr, 32 * (k + 1))), _ints(ctx.download(g.ptr, 32 * (k + 1)))


@pytest.fixture(scope="module")
def want():
    """m -> (f at _points(m), g at _points(m)) from the interpolating polynomials: once, shared by every test"""
    out = {}
    for m in FG_M:
        a, b = _inputs(m)
        pf, pg = F.interpolate(a), F.interpolate(b)
        out[m] = ([F.poly_eval(pf, x) for x in _points(m)], [F.poly_eval(pg, x) for x in _points(m)])
    return out


def test_the_output_has_max_m_1_scalars():
    assert [len(_points(m)) for m in FG_M] == [max(m, 1) for m in FG_M]


@pytest.mark.parametrize("m", FG_M)
def test_direct_route_against_the_interpolating_polynomials(ctx, want, m):
    a, b = _inputs(m)
    f, g = _extend_fg(ctx, m, a, b, "direct")
    k = max(m, 1)
    assert (f[:k], g[:k]) == want[m]
    assert f[k] == PAT and g[k] == PAT                               # nothing written past max(m, 1) scalars
    # and their products are the h of the single prover's z tail: h(0), h(m+2 .. 2m)
    tail = F.z_tail_bary(a[:m], b[:m], a[m], b[m])
    assert [x * y % N for x, y in zip(f[:k], g[:k])] == [tail[2 + x] for x in _points(m)]
    assert (f[0], g[0]) == (tail[0], tail[1])


@pytest.mark.parametrize("m", FG_M)
def test_ntt_route_is_the_direct_one_bit_for_bit(ctx, want, m):
    a, b = _inputs(m)
    assert (ctx.cs_extend_ntt_len(m) > 0) == (m >= 2)                # below 2 there is no correlation: direct whatever the mode
    ntt = _extend_fg(ctx, m, a, b, "ntt")
    assert ntt == _extend_fg(ctx, m, a, b, "direct")
    assert ntt == _extend_fg(ctx, m, a, b, "auto")                   # the NTT from 64 gates on, the direct kernel below
    k = max(m, 1)
    assert (ntt[0][:k], ntt[1][:k]) == want[m]


@pytest.mark.parametrize("m", [3, 65])
def test_words_above_the_order_are_reduced_on_load(ctx, want, m):
    a, b = _inputs(m)
    top = (1 << 256) - 1
    lift = lambda v: [x + N if x + N <= top else x for x in v]      # noqa: E731  the other encoding of the same residue
    assert any(x >= N for x in lift(a))
    for mode in ("direct", "ntt"):
        f, g = _extend_fg(ctx, m, lift(a), lift(b), mode)
        assert (f[:m], g[:m]) == want[m], mode
    # n - 1 everywhere: the largest residues, sums that carry out of eight limbs
    hi = [N - 1] * (m + 1)
    pf = F.interpolate(hi)
    f, g = _extend_fg(ctx, m, hi, hi, "direct")
    assert f[:m] == g[:m] == [F.poly_eval(pf, x) for x in _points(m)]


@pytest.mark.parametrize("m", [2, 65])
def test_on_shamir_shares_it_gives_shares_of_f_and_g(ctx, want, m):
    """M = 3, t = 1: every party's f and g on its shares of (a, b) recombine to f and g of the secrets"""
    a, b = _inputs(m)
    rng = random.Random(77 + m)
    a_sh, b_sh = mref.deal(a, 1, 3, rng), mref.deal(b, 1, 3, rng)
    outs = [_extend_fg(ctx, m, a_sh[p], b_sh[p], "auto") for p in range(3)]
    assert (mref.recombine([o[0][:m] for o in outs]), mref.recombine([o[1][:m] for o in outs])) == want[m]
    assert outs[0][0][:m] != want[m][0]                              # (a share is not the value)


def test_argument_contracts(ctx):
    from verifiable_mpc_amd import _native as nat
    f, h, p = ctx.lib.vmpc_bn256_fr_cs_extend_fg_dev, ctx.handle, ctypes.c_void_p
    buf = ctx.alloc(32 * 8)
    ptrs = [p(buf.ptr)] * 6
    assert f(None, None, None, (1 << 20) + 1, None, None, None, None) == nat.E_RANGE      # before any pointer
    assert f(None, ptrs[0], ptrs[1], 3, ptrs[2], ptrs[3], ptrs[4], ptrs[5]) == nat.E_INVAL
    for missing in range(6):
        args = list(ptrs)
        args[missing] = None
        assert f(h, args[0], args[1], 3, args[2], args[3], args[4], args[5]) == nat.E_INVAL, missing
