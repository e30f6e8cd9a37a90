"""The element-wise Ed25519 point-vector kernels (csrc/exact.hip, and vmpc_points_validate_dev, vmpc_fixed_base_dev and
vmpc_points_sum(_many)_dev of csrc/msm.hip) one entry point at a time, against oracle/ed25519_ref.py, the threaded C
oracle and tests/ptvec_ref.py.  Every comparison is exact: bytes against bytes, or Python ints against Python ints.

The shapes stand for the launch constants, restated here (nothing is imported from the code under test): EX_BLOCK =
MSM_BLOCK = 256 lanes per workgroup; below 4096 elements a normalisation runs one lane per element (k_normalize), from
4096 on one lane per chain of NORM_BATCH = 8 elements t, t + lanes, t + 2 lanes, .. with lanes = ceil(n / 8)
(k_normalize_batched: one inversion per chain, the running products parked in the output buffer); the fold takes
k_fold_pipe<1> (FP_ELEMS = 16 elements per workgroup) up to 16 C elements on a device of C compute units,
k_fold_pipe<2> (32 per workgroup, two pairs of waves) up to 8192, k_fold_quad up to 16384, and k_fold beyond.

normalize, n elements:
    n = 1, 255, 256, 257     one lane; a workgroup one short of full, full, a second of one lane
    n = 4095                 the last length of the per-element kernel
    n = 4096                 the first batched length: 512 lanes, two full workgroups, every chain 8 elements long
    n = 4097                 513 lanes, a third workgroup of one lane; the chains of lanes 506 .. 512 stop at 7 elements
    n = 4103, 4104           n mod 8 = 7 (lane 512 alone stops short) and the next multiple of 8
    among the inputs: the identity as (0 : lam : lam), a point with Z = p - 1, one with X = p - 1
    Z = 0 at n = 257 and n = 4097: the first, a middle and the last element of one chain; two neighbours in one chain;
    a whole chain of 8 and the whole 7-element chain of lane 510; element 0 and element n - 1; all of these at once.
    Wanted: (0, 0) at exactly those elements from either kernel, every other element as without them
affine_to_proj: n = 1, 255, 256, 257
points_validate: n = 0 (NULL); n = 1, 255, 256, 257, 70001 clean (274 workgroups, the last of 113 lanes), the points
    of order 1, 2 and 4 among them; offenders at 0, 255, 256, n - 1 and 17 random indices, one kind at a time and
    mixed: x + p and y + p of points with a coordinate below 19, (0, p) (which is (0, 0)), (0, p + 1) (the identity
    one encoding up), (sqrt(-1), p), bit 255 of x, a flipped bit of y, (0, 0); a clean call right after
repeat: n = 255, 256, 257 with scalars 2^k and 2^k - 1 on the word boundaries; modes 1 and 2 at n = 64; one affine
    base for 257 exponents; n_bases neither 1 nor n
tree_reduce: n = 255 .. 1025 around one and two workgroups in the first level (512 pairs), with and without the
    identity; n = 0
fold: half = 16 C, 16 C + 1 (the last k_fold_pipe<2> workgroup has one live element), 16 C + 16 (its second pair of
    waves has none); 8193 and 16400 with affine input and affine output only
fixed_base: n = 255, 256, 257 and 4095, 4096, 4097 (it ends in the same normalisation switch)
points_sum(_many): m = 0, 1, 5; k = 1, 3, 300; k = 0 and k = 65536 refused

Every buffer an entry writes lies between two guard elements of 0x5a bytes and starts out as that pattern, which is
no point of the curve (tests/test_ptvec_ref.py): a written zero is a written zero.
"""
import ctypes
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import ed25519_ref as ed
from tests import ptvec_ref as ref

pytestmark = pytest.mark.gpu

ELL, P = ed.ELL, ed.P
PAT_BYTE = 0x5A
AFF, PROJ, EXT = 64, 96, 128
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


def _rows(tuples, width):
    """tuples of `width` ints below 2^256 -> (n, 32 width) bytes"""
    raw = b"".join(int(v).to_bytes(32, "little") for t in tuples for v in t)
    return np.frombuffer(raw, np.uint8).reshape(-1, 32 * width).copy()


def _tuples(a):
    """(n, 32 w) bytes -> n tuples of w ints"""
    a = np.ascontiguousarray(a)
    w = a.shape[1] // 32
    raw = a.tobytes()
    vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    return [tuple(vals[i:i + w]) for i in range(0, len(vals), w)]


def _scalars(vals):
    return _rows([(v,) for v in vals], 1)


class Guarded:
    """n elements of `elem` bytes of device memory between two guard elements; all of it starts as the pattern"""

    def __init__(self, ctx, n, elem):
        self.ctx, self.n, self.elem = ctx, n, elem
        self.buf = ctx.upload(np.full((n + 2, elem), PAT_BYTE, np.uint8))
        self.ptr = self.buf.ptr + elem

    def read(self):
        """the n elements as (n, elem) bytes, after the stream has drained and the guards have been looked at"""
        self.ctx.sync()
        raw = self.ctx.download(self.buf.ptr, self.elem * (self.n + 2), (self.n + 2, self.elem))
        assert (raw[0] == PAT_BYTE).all(), "the element in front of the buffer was written"
        assert (raw[-1] == PAT_BYTE).all(), "the element behind the buffer was written"
        return raw[1:-1]

    def untouched(self):
        return bool((self.read() == PAT_BYTE).all())


def same(got, want, what):
    want = np.asarray(want, np.uint8).reshape(-1, got.shape[1])
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ, the first at {i}: got "
                             f"{[hex(v) for v in _tuples(got[i:i + 1])[0]]}, want "
                             f"{[hex(v) for v in _tuples(want[i:i + 1])[0]]}")


class Pool:
    """64 ladder results (Z != 1), their affine forms, and vectors of any length made of rescaled copies"""

    def __init__(self):
        rng = random.Random(25519)
        self.base = [ed.pt_repeat(ed.BASE, rng.randrange(1, ELL)) for _ in range(64)]
        assert all(z != 1 and x and y for x, y, z in self.base)
        self.aff = ref.normalize(self.base)

    def proj(self, n, seed):
        """n projective points: element i is a random representative of a random one of the 64"""
        rng = random.Random(seed)
        return [ref.rescale(self.base[rng.randrange(64)], rng.randrange(1, P)) for _ in range(n)]

    def affine(self, n, seed):
        """(n, 64) bytes: the points of order 1, 2, 4 first, then the 64, then random ones of the 68"""
        table = _rows(ref.LOW_ORDER + self.aff, 2)
        idx = np.arange(n) % len(table)
        if n > len(table):
            idx[len(table):] = np.random.default_rng(seed).integers(0, len(table), n - len(table))
        return table[idx]


@pytest.fixture(scope="module")
def pool():
    return Pool()


# ---- vmpc_normalize_dev ------------------------------------------------------------------------------------------------------
NORM_MAX = 4104


@pytest.fixture(scope="module")
def norm_pool(pool):
    """4104 points and their normalisation, computed once: a case takes a prefix and restates what it plants"""
    pts = pool.proj(NORM_MAX, 1)
    return pts, ref.normalize(pts)


def _norm_case(pool, norm_pool, n):
    """(points, wanted affine) of n elements with the three special representatives at 0, n / 2 and n - 1"""
    pts, want = list(norm_pool[0][:n]), list(norm_pool[1][:n])
    x, _, z = pool.base[1]
    specials = [ref.rescale(ed.IDENTITY, 0x1234567 + n),
                ref.rescale(pool.base[1], (P - 1) * pow(z, P - 2, P)),
                ref.rescale(pool.base[1], (P - 1) * pow(x, P - 2, P))]
    assert specials[0][0] == 0 and specials[0][1] == specials[0][2] != 1
    assert specials[1][2] == P - 1 and specials[2][0] == P - 1
    for k, at in enumerate((0, n // 2, n - 1)):
        pts[at] = specials[(k + n) % 3]
        want[at] = ref.normalize([pts[at]])[0]
    return pts, want


def _normalize(ctx, pts):
    d = ctx.upload(_rows(pts, 3))
    out = Guarded(ctx, len(pts), AFF)
    ctx.normalize(d.ptr, len(pts), out.ptr)
    return out.read()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 4103, 4104])
def test_normalize(ctx, pool, norm_pool, n):
    pts, want = _norm_case(pool, norm_pool, n)
    same(_normalize(ctx, pts), _rows(want, 2), f"normalize, n = {n}")


def _zero_patterns(n):
    lanes = (n + 7) // 8
    chain = lambda t: [t + k * lanes for k in range(8) if t + k * lanes < n]          # noqa: E731
    pats = {
        "chain_first_middle_last": [chain(5)[0], chain(5)[4], chain(5)[7]],
        "chain_two_neighbours": chain(7)[2:4],                  # e and e + lanes
        "chain_whole": chain(9),
        "short_chain_whole": chain(lanes - 3),                  # a lane whose chain has 7 elements
        "first_and_last_element": [0, n - 1],
    }
    assert len(chain(9)) == 8 and len(chain(lanes - 3)) == 7 and chain(lanes - 3)[-1] + lanes >= n
    pats["all_of_them"] = sorted({i for v in pats.values() for i in v})
    return pats


@pytest.mark.parametrize("pattern", list(_zero_patterns(4097)))
@pytest.mark.parametrize("n", [257, 4097])
def test_normalize_z_zero_comes_out_as_zero_zero_and_disturbs_nobody(ctx, pool, norm_pool, n, pattern):
    pts, want = _norm_case(pool, norm_pool, n)
    planted = _zero_patterns(n)[pattern]
    for i in planted:
        x, y, _ = norm_pool[0][i]
        assert x and y
        pts[i] = (x, y, 0)
        want[i] = ref.normalize([pts[i]])[0]
        assert want[i] == (0, 0)
    got = _normalize(ctx, pts)
    zero_rows = [int(i) for i in np.flatnonzero(~got.any(axis=1))]
    assert zero_rows == sorted(planted), (pattern, zero_rows)
    same(got, _rows(want, 2), f"normalize with Z = 0 at {planted}, n = {n}")


# ---- vmpc_affine_to_proj_dev -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_affine_to_proj(ctx, pool, n):
    ab = pool.affine(n, 2)
    d = ctx.upload(ab)
    out = Guarded(ctx, n, PROJ)
    ctx.affine_to_proj(d.ptr, n, out.ptr)
    want = np.concatenate([ab, np.tile(_rows([(1,)], 1), (n, 1))], axis=1)
    assert _tuples(want[:1]) == [(0, 1, 1)]
    same(out.read(), want, f"affine_to_proj, n = {n}")


# ---- vmpc_points_validate_dev ------------------------------------------------------------------------------------------------
def _offender_kinds(pool):
    """kind -> (raw x, raw y) of one element that must be counted"""
    sx = next(pt for pt in map(ref.affine_with_x, range(1, 19)) if pt)
    sy = next(pt for pt in map(ref.affine_with_y, range(1, 19)) if pt)
    kinds = {
        "x + p": (sx[0] + P, sx[1]),
        "y + p": (sy[0], sy[1] + P),
        "(0, p)": (0, P),
        "(0, p + 1), the identity one encoding up": (0, P + 1),
        "(sqrt(-1), p)": (ed.SQRT_M1, P),
        "bit 255 of x": (pool.aff[3][0] | 1 << 255, pool.aff[3][1]),
        "a flipped bit of y": (pool.aff[5][0], pool.aff[5][1] ^ 1),
        "(0, 0)": (0, 0),
    }
    assert all(not ref.is_valid_affine(*v) for v in kinds.values())
    # these four are points of the curve once reduced: the encoding alone is wrong
    for k in ("x + p", "y + p", "(0, p + 1), the identity one encoding up", "(sqrt(-1), p)"):
        x, y = kinds[k]
        assert ed.on_curve((x, y, 1)) and x < 1 << 255 and y < 1 << 255, k
    return kinds


def test_validate_nothing(ctx):
    assert ctx.validate_points(None, 0) == 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_validate_passes_clean_vectors_low_order_points_included(ctx, pool, n):
    ab = pool.affine(n, 3)
    assert all(ref.is_valid_affine(*t) for t in _tuples(ab[:68]))
    assert _tuples(ab[:1]) == [(0, 1)]
    d = ctx.upload(ab)
    assert ctx.validate_points(d.ptr, n) == 0


@pytest.mark.parametrize("n", [257, 70001])
def test_validate_counts_every_offender(ctx, pool, n):
    kinds = _offender_kinds(pool)
    clean = pool.affine(n, 4)
    d_clean = ctx.upload(clean)
    rng = random.Random(n)
    at = sorted({0, 255, 256, n - 1} | set(rng.sample(range(n), 17)))
    assert 17 <= len(at) <= 21
    names = list(kinds)
    for which in names + ["every kind"]:
        ab = clean.copy()
        for j, i in enumerate(at):
            ab[i] = _rows([kinds[which if which in kinds else names[j % len(names)]]], 2)[0]
        assert sum(not ref.is_valid_affine(*t) for t in _tuples(ab[at])) == len(at)
        d = ctx.upload(ab)
        assert ctx.validate_points(d.ptr, n) == len(at), which
        # one offender alone, on the last lane of the first workgroup and on the first lane of the second
        for i in (255, 256):
            one = clean.copy()
            one[i] = ab[i]
            d = ctx.upload(one)
            assert ctx.validate_points(d.ptr, n) == 1, (which, i)
    assert ctx.validate_points(d_clean.ptr, n) == 0, "the counter starts from 0 again"


# ---- vmpc_repeat_dev ---------------------------------------------------------------------------------------------------------
WORD_EDGES = [v for k in (31, 32, 33, 63, 64, 65, 224, 252) for v in (1 << k, (1 << k) - 1)]


@pytest.fixture(scope="module")
def repeat_mode0(pool):
    """257 projective bases, 257 scalars (the word-boundary ones first and again on the last three elements), and
    ed.pt_repeat of each pair"""
    rng = random.Random(8)
    bases = pool.proj(257, 5)
    sc = WORD_EDGES + [rng.randrange(ELL) for _ in range(257 - len(WORD_EDGES))]
    sc[254], sc[255], sc[256] = (1 << 252) - 1, 1 << 64, (1 << 64) - 1
    sc[16], sc[17] = 0, 1
    return bases, sc, [ed.pt_repeat(b, s) for b, s in zip(bases, sc)]


def _repeat(ctx, base_rows, n_bases, affine, scalar_rows, n, mode, want_proj, want_aff, what, proj=True, aff=True):
    db, ds = ctx.upload(base_rows), ctx.upload(scalar_rows)
    op, oa = Guarded(ctx, n, PROJ), Guarded(ctx, n, AFF)
    ctx.repeat(db.ptr, n_bases, affine, ds.ptr, n, mode, op.ptr if proj else None, oa.ptr if aff else None)
    if proj:
        same(op.read(), _rows(want_proj, 3), f"{what}: (X, Y, Z)")
    else:
        assert op.untouched()
    if aff:
        same(oa.read(), _rows(want_aff, 2), f"{what}: affine")
    else:
        assert oa.untouched()


@pytest.mark.parametrize("n", [255, 256, 257])
def test_repeat_elementwise(ctx, repeat_mode0, n):
    bases, sc, want = (v[:n] for v in repeat_mode0)
    _repeat(ctx, _rows(bases, 3), n, False, _scalars(sc), n, 0, want, ref.normalize(want), f"repeat, n = {n}")


def test_repeat_residues_read_as_signed(ctx, pool):
    rng = random.Random(9)
    n = 64
    bases = pool.proj(n, 6)
    sc = [0, 1, ELL - 1, ELL // 2, ELL // 2 + 1, ELL // 2 - 1, ELL // 2 + 2, ELL - 2, 1 << 252, (1 << 252) - 1]
    sc += [rng.randrange(ELL) for _ in range(n - len(sc))]
    assert sum(s > ELL // 2 for s in sc) >= 20 and sum(s <= ELL // 2 for s in sc) >= 20
    assert ed.scalar_int(ELL // 2) == ELL // 2 and ed.scalar_int(ELL // 2 + 1) == -(ELL // 2)
    want = [ed.pt_repeat(b, ed.scalar_int(s)) for b, s in zip(bases, sc)]
    _repeat(ctx, _rows(bases, 3), n, False, _scalars(sc), n, 1, want, ref.normalize(want), "repeat, mode 1")


def test_repeat_sign_magnitude_exponents_are_python_ints(ctx, pool):
    rng = random.Random(10)
    n = 64
    bases = pool.proj(n, 7)
    mags = [1, ELL - 1, ELL, ELL + 1, 2 * ELL, 1 << 254, (1 << 255) - 1]
    exps = [0, 0] + [s * m for m in mags for s in (1, -1)]
    exps += [rng.choice((1, -1)) * rng.randrange(1 << rng.choice((64, 200, 253, 255))) for _ in range(n - len(exps))]
    raw = [ref.sign_magnitude(e, negative_zero=(i == 1)) for i, e in enumerate(exps)]
    assert raw[1] == bytes(31) + b"\x80" and [ref.from_sign_magnitude(b) for b in raw] == exps
    want = [ed.pt_repeat(b, e) for b, e in zip(bases, exps)]
    assert want[0] == want[1] == ed.IDENTITY
    sb = np.frombuffer(b"".join(raw), np.uint8).reshape(n, 32)
    _repeat(ctx, _rows(bases, 3), n, False, sb, n, 2, want, ref.normalize(want), "repeat, mode 2")


def test_repeat_one_affine_base_affine_output_only(ctx, pool):
    rng = random.Random(11)
    n = 257
    base = pool.aff[2] + (1,)
    sc = [rng.randrange(1 << rng.randrange(1, 253)) for _ in range(n)]
    sc[0], sc[255], sc[256] = ELL - 1, 0, (1 << 252) - 1
    want = ref.normalize([ed.pt_repeat(base, s) for s in sc])
    _repeat(ctx, _rows([base[:2]], 2), 1, True, _scalars(sc), n, 0, None, want, "repeat of one base", proj=False)


def test_repeat_refuses_a_base_count_that_is_neither_one_nor_n(nat, ctx, pool):
    n = 8
    db, ds = ctx.upload(_rows(pool.proj(n, 8), 3)), ctx.upload(_scalars([3] * n))
    op, oa = Guarded(ctx, n, PROJ), Guarded(ctx, n, AFF)
    for n_bases in (0, 2, n - 1, n + 1):
        for mode in (0, 1, 2):
            assert ctx.lib.vmpc_repeat_dev(ctx.handle, vp(db.ptr), n_bases, 0, vp(ds.ptr), n, mode, vp(op.ptr),
                                           vp(oa.ptr)) == nat.E_INVAL, (n_bases, mode)
    assert op.untouched() and oa.untouched()


# ---- vmpc_tree_reduce_dev ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree_pool(pool):
    return pool.proj(1025, 12)


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 1000, 1025])
def test_tree_reduce(ctx, tree_pool, n):
    pts = tree_pool[:n]
    rows = _rows(pts, 3)
    for append in (False, True):
        d = ctx.upload(rows)            # the entry may clobber its input
        out = Guarded(ctx, 1, PROJ)
        ctx.tree_reduce(d.ptr, n, append, out.ptr)
        want = ed.tree_reduce(ed.pt_add, pts, ed.IDENTITY if append else None)
        same(out.read(), _rows([want], 3), f"tree_reduce, n = {n}, identity appended: {append}")


def test_tree_reduce_of_nothing(nat, ctx):
    out = Guarded(ctx, 1, PROJ)
    ctx.tree_reduce(None, 0, True, out.ptr)
    same(out.read(), _rows([(0, 1, 1)], 3), "the identity alone")
    out = Guarded(ctx, 1, PROJ)
    assert ctx.lib.vmpc_tree_reduce_dev(ctx.handle, None, 0, 0, vp(out.ptr)) == nat.E_INVAL
    assert out.untouched()


# ---- vmpc_fold_dev -----------------------------------------------------------------------------------------------------------
def _fold_vectors(pool, n, seed, proj=True):
    """two vectors of n points, as projective bytes (random representatives) and as affine bytes of the same points"""
    rng = np.random.default_rng(seed)
    il, ir = rng.integers(0, 64, n), rng.integers(0, 64, n)
    aff = _rows(pool.aff, 2)
    prng = random.Random(seed)
    pl = _rows([ref.rescale(pool.base[i], prng.randrange(1, P)) for i in il], 3) if proj else None
    pr = _rows([ref.rescale(pool.base[i], prng.randrange(1, P)) for i in ir], 3) if proj else None
    return pl, pr, aff[il], aff[ir]


def _threaded(fn):
    c_oracle.set_threads(c_oracle.host_threads())
    try:
        return fn()
    finally:
        c_oracle.set_threads(1)


def _c_bytes(c):
    return np.frombuffer(int(c).to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def cu_count(nat):
    """C as the library reports it of the device it runs on (cus= of vmpc_backend_info): the very figure
    vmpc_fold_dev compares half with.  torch is not asked: a process in which the library has brought up the HIP
    runtime need not be one in which torch can open the device as well"""
    import re
    return int(re.search(r"cus=(\d+)", nat.backend_info()[1]).group(1))


@pytest.fixture(scope="module")
def fold_switch(pool, cu_count):
    """vectors of 16 C + 16 pairs and the oracle's folds of them, once: the fold is element-wise, so each length takes
    a prefix"""
    if 16 * cu_count >= 8192:
        pytest.skip("k_fold_pipe<2> is never launched on a device this wide")
    n = 16 * cu_count + 16
    pl, pr, al, ar = _fold_vectors(pool, n, 13)
    c = random.Random(14).randrange(1 << 251, ELL)
    refs = _threaded(lambda: {("proj", c): c_oracle.fold(pl, pr, _c_bytes(c), proj_in=True),
                              ("proj", ELL - 1): c_oracle.fold(pl, pr, _c_bytes(ELL - 1), proj_in=True),
                              ("proj", 1): c_oracle.fold(pl, pr, _c_bytes(1), proj_in=True),
                              ("affine", c): c_oracle.fold(al, ar, _c_bytes(c), proj_in=False)})
    return {"proj": (pl, pr), "affine": (al, ar)}, c, refs


def _fold(ctx, gl, gr, affine, c, half, want, what, proj=True, aff=True):
    dl, dr = ctx.upload(gl[:half]), ctx.upload(gr[:half])
    op, oa = Guarded(ctx, half, PROJ), Guarded(ctx, half, AFF)
    ctx.fold(dl.ptr, dr.ptr, affine, c, half, op.ptr if proj else None, oa.ptr if aff else None)
    if proj:
        same(op.read(), want[0][:half], f"{what}: (X, Y, Z)")
    else:
        assert op.untouched()
    if aff:
        same(oa.read(), want[1][:half], f"{what}: affine")
    else:
        assert oa.untouched()


@pytest.mark.parametrize("past", [0, 1, 16])
def test_fold_at_the_switch_between_one_and_two_pairs_of_waves(ctx, cu_count, fold_switch, past):
    inputs, c, refs = fold_switch
    half = 16 * cu_count + past
    pl, pr = inputs["proj"]
    al, ar = inputs["affine"]
    _fold(ctx, pl, pr, False, c, half, refs["proj", c], f"fold, half = {half}")
    _fold(ctx, pl, pr, False, c, half, refs["proj", c], f"fold, half = {half}, affine output only", proj=False)
    _fold(ctx, al, ar, True, c, half, refs["affine", c], f"fold, half = {half}, affine input")
    _fold(ctx, pl, pr, False, ELL - 1, half, refs["proj", ELL - 1], f"fold, half = {half}, c = l - 1")
    _fold(ctx, pl, pr, False, 1, half, refs["proj", 1], f"fold, half = {half}, c = 1")


def test_fold_affine_in_affine_out_on_the_longer_paths(ctx, pool):
    """k_fold_quad (8193) and k_fold (16400) with both flags; a 64-bit c, because the flags do not depend on the
    ladder's length and tests/test_gpu_cabi.py runs the full-length ladders of these kernels"""
    n = 16400
    _, _, al, ar = _fold_vectors(pool, n, 15, proj=False)
    c = random.Random(16).randrange(1 << 63, 1 << 64)
    want = _threaded(lambda: c_oracle.fold(al, ar, _c_bytes(c), proj_in=False))
    for half in (8193, n):
        _fold(ctx, al, ar, True, c, half, want, f"fold, half = {half}, affine in, affine out", proj=False)


# ---- vmpc_fixed_base_dev -----------------------------------------------------------------------------------------------------
RECODING_EDGES = [0, 1, 2, 127, 128, 129, 255, 256, 257, 0x8080, 0x7f7f7f7f, (1 << 252) - 1, 1 << 252, ELL - 1, ELL - 2,
                  int.from_bytes(bytes([0x80] * 31 + [0x0f]), "little"),
                  int.from_bytes(bytes([0x81] * 31 + [0x0f]), "little"),
                  int.from_bytes(bytes([0xff] * 31 + [0x0f]), "little")]


@pytest.fixture(scope="module")
def fixed_base_ref(pool):
    rng = random.Random(17)
    n = 4097
    base = pool.aff[0]
    sc = RECODING_EDGES + [rng.randrange(ELL) for _ in range(n - len(RECODING_EDGES))]
    sc[254], sc[255], sc[256], sc[4094], sc[4095], sc[4096] = ELL - 1, 0, 1, ELL - 2, 0, ELL - 1
    sb = _scalars(sc)
    proj, _ = _threaded(lambda: c_oracle.fixed_base(_rows([base + (1,)], 3)[0], sb))
    return _rows([base], 2), sb, _rows(ref.normalize(_tuples(proj)), 2)


@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096, 4097])
def test_fixed_base(ctx, fixed_base_ref, n):
    base, sb, want = fixed_base_ref
    db, ds = ctx.upload(base), ctx.upload(sb[:n])
    out = Guarded(ctx, n, AFF)
    ctx.fixed_base(db.ptr, ds.ptr, n, out.ptr)
    same(out.read(), want[:n], f"fixed_base, n = {n}")


# ---- vmpc_points_sum_dev, vmpc_points_sum_many_dev ---------------------------------------------------------------------------
def _extended(pt):
    x, y, z = pt
    return (x * z % P, y * z % P, z * z % P, x * y % P)


def _sums(ctx, ext_rows, m, k, want, what, many=True):
    """k sums of m points through one entry; the extended output as a group element and as X Y = T Z, the affine
    output as bytes"""
    d = ctx.upload(ext_rows) if m else None
    oe, oa = Guarded(ctx, k, EXT), Guarded(ctx, k, AFF)
    if many:
        ctx.points_sum_many(d.ptr if m else None, m, k, oe.ptr, oa.ptr)
    else:
        ctx.points_sum(d.ptr if m else None, m, oe.ptr, oa.ptr)
    same(oa.read(), _rows(want, 2), f"{what}: affine")
    ext = _tuples(oe.read())
    assert all(max(e) < P for e in ext), f"{what}: a coordinate is not canonical"
    assert [x * y % P == t * z % P and z != 0 for x, y, z, t in ext] == [True] * k, f"{what}: X Y = T Z"
    assert ref.normalize([e[:3] for e in ext]) == want, f"{what}: the extended output"


def test_points_sum_of_nothing_and_of_one(ctx, pool):
    _sums(ctx, None, 0, 1, [(0, 1)], "sum of nothing", many=False)
    _sums(ctx, None, 0, 1, [(0, 1)], "sum_many of nothing, k = 1")
    _sums(ctx, None, 0, 3, [(0, 1)] * 3, "sum_many of nothing, k = 3")
    pts = pool.proj(3, 18)
    rows = _rows([_extended(p) for p in pts], 4)
    _sums(ctx, rows[:1], 1, 1, ref.normalize(pts[:1]), "sum of one", many=False)
    _sums(ctx, rows, 1, 3, ref.normalize(pts), "sum_many of one, k = 3")


@pytest.mark.parametrize("k", [1, 3, 300])
def test_points_sum_many_interleaved(ctx, pool, k):
    m = 5
    pts = pool.proj(m * k, 19 + k)                       # point i of sum j at index i k + j
    want = []
    for j in range(k):
        acc = pts[j]
        for i in range(1, m):
            acc = ed.pt_add(acc, pts[i * k + j])
        want.append(acc)
    want = ref.normalize(want)
    rows = _rows([_extended(p) for p in pts], 4)
    _sums(ctx, rows, m, k, want, f"sum_many, m = {m}, k = {k}")
    if k == 1:
        _sums(ctx, rows, m, 1, want, f"sum, m = {m}", many=False)


def test_points_sum_many_refuses_no_sums_and_too_many(nat, ctx, pool):
    d = ctx.upload(_rows([_extended(p) for p in pool.proj(2, 20)], 4))
    oe, oa = Guarded(ctx, 1, EXT), Guarded(ctx, 1, AFF)
    for k in (0, 65536):
        assert ctx.lib.vmpc_points_sum_many_dev(ctx.handle, vp(d.ptr), 0, k, vp(oe.ptr), vp(oa.ptr)) == nat.E_INVAL, k
        assert ctx.lib.vmpc_points_sum_many_dev(ctx.handle, vp(d.ptr), 1, k, vp(oe.ptr), vp(oa.ptr)) == nat.E_INVAL, k
    assert oe.untouched() and oa.untouched()
