"""vmpc_fr_batch_products_dev (csrc/batch_verify.hip) through the C ABI, byte for byte against tests/batch_verify_ref.py.

The index of v_p is cut at bit b = R + lb - a, a = min(R, (R + lb) / 2), restated here (nothing is imported from the code
under test): a table of 2^a entries per proof over the high challenges, one of 2^b over the low ones and z'.  A
workgroup of the u kernel and of the dot kernel takes 256 columns of the low table; the dot's rows are cut into segments
of at least 16.  Shapes (K, R, lb):
    (1, R, lb), w = 1        also equal to vmpc_fr_challenge_products_dev: (0, 0), (0, 4), (1, 0), (4, 0), (3, 5)
    K = 2, 3, 17             at (3, 1) and (7, 1): the 4-proof unrolled loop of the u kernel with 2, 3 and 1 left over
    (1, 1), (2, 1)           a = 1, b = 1 and a = 1, b = 2; (1, 0): the low table is z' alone; (0, 4): the high one is w
    (4, 1), (5, 1)           R + lb odd and even: b = a + 1 and b = a
    (7, 1), (8, 1)           N = 256 and 512, 16 rows of 16 and of 32 columns: one row segment
    (15, 1), K = 3           a = b = 8: a full 256-lane workgroup per row, 256 rows in 16 segments for the dot's second launch
    (16, 1), (1, 9)          b = 9: two column blocks per row (a = 8, and a = 1 clamped by R)
    (1, 17), K = 1           512 column blocks: the second launch's lanes take a second trip over the segments
form_len = 0, N - 1, N; one-hot forms and one-hot z' (a dropped element cannot cancel); a challenge 0 and a challenge 1;
weights l - 1 and 2^128.  u_out and dots_out lie between guard elements of 0x5a bytes and start as that pattern.
"""
import ctypes
import random

import numpy as np
import pytest

from tests import batch_verify_ref as ref
from tests import frvec_ref

pytestmark = pytest.mark.gpu

ELL = ref.ELL
PAT_BYTE = 0x5A
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
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32).copy()


def _ints(a):
    raw = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


class Guarded:
    """n elements of device memory between two guard elements; guards and elements start as the pattern"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.buf = ctx.upload(np.full((n + 2, 32), PAT_BYTE, np.uint8))
        self.ptr = self.buf.ptr + 32

    def read(self):
        self.ctx.sync()
        raw = self.ctx.download(self.buf.ptr, 32 * (self.n + 2), (self.n + 2, 32))
        assert (raw[0] == PAT_BYTE).all(), "the element in front of the buffer was written"
        assert (raw[-1] == PAT_BYTE).all(), "the element behind the buffer was written"
        return raw[1:-1]

    def untouched(self):
        return bool((self.read() == PAT_BYTE).all())


def same(got, want, what):
    want = _bytes(want) if len(want) else np.zeros((0, 32), np.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ, the first at {i}: got "
                             f"{_ints(got[i])[0]:#x}, want {_ints(want[i])[0]:#x}")


class Case:
    """K proofs' worth of random operands, with l - 1 planted at both ends of every vector"""

    def __init__(self, K, R, lb, seed):
        rng = random.Random(seed)
        self.K, self.R, self.lb, self.n = K, R, lb, 1 << (R + lb)

        def vec(m):
            v = [rng.randrange(ELL) for _ in range(m)]
            if m:
                v[0] = v[-1] = ELL - 1
            return v
        self.cs = [vec(R) for _ in range(K)]
        self.zs = [vec(1 << lb) for _ in range(K)]
        self.ws = [rng.randrange(1, ELL) for _ in range(K)]
        self.forms = [vec(self.n) for _ in range(K)]

    def run(self, ctx, form_len=None):
        """(u, dots) as bytes from the library, guards checked"""
        form_len = self.n if form_len is None else form_len
        chal = ctx.upload(_bytes([c for cs in self.cs for c in cs])) if self.R else None
        zp = ctx.upload(_bytes([z for zs in self.zs for z in zs]))
        wts = ctx.upload(_bytes(self.ws))
        fbufs = [ctx.upload(_bytes(f)) for f in self.forms]
        fptr = ctx.upload(np.array([f.ptr for f in fbufs], np.uint64))
        u, dots = Guarded(ctx, self.n), Guarded(ctx, self.K)
        ctx.fr_batch_products(self.K, self.R, self.lb, chal.ptr if chal else None, zp.ptr, wts.ptr, fptr.ptr, form_len,
                              u.ptr, dots.ptr)
        return u.read(), dots.read()

    def check(self, ctx, form_len=None):
        form_len = self.n if form_len is None else form_len
        u, dots = self.run(ctx, form_len)
        want_u, want_dots = ref.batch_products(self.cs, self.lb, self.zs, self.ws, self.forms, form_len)
        what = f"K={self.K} R={self.R} lb={self.lb} form_len={form_len}"
        same(u, want_u, "u " + what)
        same(dots, want_dots, "dots " + what)
        return u, dots


@pytest.mark.parametrize("R,lb", [(0, 0), (0, 4), (1, 0), (4, 0), (3, 5)])
def test_one_proof_weight_one_is_challenge_products(ctx, R, lb):
    case = Case(1, R, lb, 100 + 10 * R + lb)
    case.ws = [1]
    u, dots = case.check(ctx)
    z = ctx.upload(_bytes(case.zs[0]))
    out = Guarded(ctx, case.n)
    ctx.fr_challenge_products(case.cs[0], lb, z.ptr, out.ptr)
    assert np.array_equal(u, out.read())


@pytest.mark.parametrize("K,R,lb", [(2, 3, 1), (3, 3, 1), (17, 3, 1), (2, 7, 1), (3, 7, 1), (17, 7, 1),
                                    (2, 1, 1), (3, 2, 1), (2, 4, 1), (2, 5, 1), (3, 8, 1), (5, 1, 9), (3, 15, 1), (2, 16, 1), (1, 1, 17)])
def test_matches_reference(ctx, K, R, lb):
    Case(K, R, lb, 1000 * K + 10 * R + lb).check(ctx)


@pytest.mark.parametrize("K,R,lb", [(3, 3, 1), (2, 8, 1), (2, 1, 9)])
def test_form_len(ctx, K, R, lb):
    case = Case(K, R, lb, 77 + R)
    for form_len in (0, case.n - 1, case.n):
        case.check(ctx, form_len)


def test_form_len_zero_takes_no_form_pointers(ctx):
    case = Case(2, 3, 1, 5)
    zp, wts, chal = ctx.upload(_bytes(sum(case.zs, []))), ctx.upload(_bytes(case.ws)), ctx.upload(_bytes(sum(case.cs, [])))
    u, dots = Guarded(ctx, case.n), Guarded(ctx, 2)
    ctx.fr_batch_products(2, 3, 1, chal.ptr, zp.ptr, wts.ptr, None, 0, u.ptr, dots.ptr)
    same(dots.read(), [0, 0], "dots")
    same(u.read(), ref.batch_products(case.cs, 1, case.zs, case.ws, [None, None], 0)[0], "u")


@pytest.mark.parametrize("R,lb", [(7, 1), (8, 1)])
def test_one_hot_forms_and_responses(ctx, R, lb):
    """each proof's form is zero but for one index, and its z' but for one element: the one product that is left cannot
    cancel against another"""
    case = Case(3, R, lb, 31 + R)
    n = case.n
    for p, j in enumerate((0, n - 1, n // 2 + 1)):
        case.forms[p] = [0] * n
        case.forms[p][j] = 1 + p
        case.zs[p] = [0] * (1 << lb)
        case.zs[p][j % (1 << lb)] = ELL - 1 - p
    _, dots = case.check(ctx)
    assert all(v != 0 for v in _ints(dots))
    case.check(ctx, n - 1)                              # proof 1's only element is cut off

def test_challenges_zero_and_one_and_extreme_weights(ctx):
    case = Case(3, 7, 1, 99)
    case.cs[0][2] = 0
    case.cs[1][6] = 1
    case.cs[2][0] = 0
    case.cs[2][1] = 1
    case.ws = [ELL - 1, 1 << 128, 1]
    case.check(ctx)


def test_bit_reproducible(ctx):
    case = Case(17, 8, 1, 3)
    u1, d1 = case.run(ctx)
    u2, d2 = case.run(ctx)
    assert np.array_equal(u1, u2) and np.array_equal(d1, d2)


def test_refusals_come_before_any_launch(ctx, nat):
    case = Case(2, 3, 1, 11)
    zp, wts, chal = ctx.upload(_bytes(sum(case.zs, []))), ctx.upload(_bytes(case.ws)), ctx.upload(_bytes(sum(case.cs, [])))
    fbufs = [ctx.upload(_bytes(f)) for f in case.forms]
    fptr = ctx.upload(np.array([f.ptr for f in fbufs], np.uint64))
    u, dots = Guarded(ctx, case.n), Guarded(ctx, 2)
    fn, h = ctx.lib.vmpc_fr_batch_products_dev, ctx.handle
    good = dict(ctx=h, K=2, R=3, lb=1, chal=vp(chal.ptr), zp=vp(zp.ptr), w=vp(wts.ptr), f=vp(fptr.ptr), fl=case.n,
                u=vp(u.ptr), d=vp(dots.ptr))

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["ctx"], a["K"], a["R"], a["lb"], a["chal"], a["zp"], a["w"], a["f"], a["fl"], a["u"], a["d"])
    # caps: answered before any pointer is looked at
    assert call(K=4097) == nat.E_RANGE
    assert call(R=21, lb=0) == nat.E_RANGE
    assert call(R=20, lb=11) == nat.E_RANGE
    assert call(R=0, lb=31) == nat.E_RANGE
    assert call(K=4097, chal=None, zp=None, w=None, f=None, u=None, d=None) == nat.E_RANGE
    for bad in (dict(ctx=None), dict(K=0), dict(K=-1), dict(R=-1), dict(lb=-1), dict(chal=None), dict(zp=None), dict(w=None),
                dict(f=None), dict(u=None), dict(d=None), dict(fl=case.n + 1)):
        assert call(**bad) == nat.E_INVAL, bad
    assert u.untouched() and dots.untouched()
    assert call() == 0
    want_u, want_dots = ref.batch_products(case.cs, 1, case.zs, case.ws, case.forms, case.n)
    same(u.read(), want_u, "u after the refusals")
    same(dots.read(), want_dots, "dots after the refusals")
    # no rounds: no challenge pointer is needed (N = 2)
    assert call(R=0, lb=1, chal=None, fl=2) == 0
    ctx.sync()
