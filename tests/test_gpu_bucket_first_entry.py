"""k_msm_bucket starts a run's accumulator from the run's FIRST table entry (csrc/ge25519.h ge_ext_from_niels_neg: one
product, -q by swapping y - x and y + x) and adds the rest with the carry-in column form of the mixed addition
(ge_madd_cols).  What can go wrong is at the start of a run, so every case puts EXACTLY L entries into one bucket, as
tests/test_gpu_bucket_runs.py does, with L on both sides of the 8-entry burst, of the 32-entry staging window (its
refill) and of the 64-entry segment, and additionally fixes the SIGN of the run: the order of a run's entries is the
sort's business, so "first entry negative" is a run whose entries are all negative digits, and likewise positive.

Checked by the exponent identity: points e_i B, so a commitment is ((sum s_i e_i) mod l) B by the oracle.

Not every combination exists.  Balanced segments of a split bucket are never shorter than half a segment, so split
runs have 4 - 8 entries (the planner's 8-entry segments at these sizes) or 32 - 64 (64-entry segments).  A 13-row table
of 5 columns holds at most 61 entries of one bucket (a scalar from 2^240 up gets a column-dependent multiple of l added
before it is recoded, tests/msm_sort_ref.py wide_k, so only column 0 controls its top digit): its cases stop at 40."""
import random

import pytest

from oracle import ed25519_ref as ed
from tests.msm_sort_ref import recode, recode_wide
from tests.test_gpu_bucket_runs import N_RANDOM, WIDE, make_ctx, want
from tests.test_gpu_cabi import gpu_points, sc_bytes
from tests.test_gpu_wide_table import ext_affine, stages

pytestmark = pytest.mark.gpu
ELL = ed.ELL
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 40, 64, 65]


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


def digits_of(s, i, c, W):
    """the library's digits of the scalar of column i: the wide table adds a column-dependent multiple of l first"""
    return recode_wide(s, i) if (c, W) == (20, 13) else recode(s, c, W, ELL)


def run_vector(rng, L, v, c, W, one_set, sign, n_random=N_RANDOM):
    """L + n_random scalars in random order.  L of them have +v or -v as their digit of window 0 (scalars v and
    2^c - v; the latter also +1 in window 1) - sign "pos": all +v, "neg": all -v, "mixed": every third -v - the others
    are uniform and clear of bucket v.  one_set: every window feeds the same bucket set (fixed-base tables)."""
    assert 1 < v < (1 << (c - 1))
    windows = range(W) if one_set else range(1)

    def hits(s, i):
        d = digits_of(s, i, c, W)
        return [d[w] for w in windows if abs(d[w]) == v]
    neg = {"pos": lambda k: False, "neg": lambda k: True, "mixed": lambda k: k % 3 == 2}[sign]
    slots = list(range(L)) + [None] * n_random
    rng.shuffle(slots)
    x = []
    for i, k in enumerate(slots):
        s = ((1 << c) - v if neg(k) else v) if k is not None else rng.randrange(ELL)
        while k is None and hits(s, i):
            s = rng.randrange(ELL)
        x.append(s)
    found = [d for i, s in enumerate(x) for d in hits(s, i)]
    assert len(found) == L
    if sign != "mixed":
        assert all((d < 0) == (sign == "neg") for d in found)
    return x


class EntryPoints:
    """the commitments of one context over n points e_i B: every way into k_msm_bucket"""

    def __init__(self, nat, ctx, n, seed, exps=None):
        self.nat, self.ctx, self.n = nat, ctx, n
        rng = random.Random(seed)
        self.exps = exps if exps is not None else [rng.randrange(1, ELL) for _ in range(n)]
        self.dp = gpu_points(nat, ctx, self.exps)
        self.out = ctx.alloc(128 * 3)
        self.tables = {}
        ctx.set_short_path(False)       # the fused path for short 16-row tables has no bucket kernel

    def table(self, rows):
        if rows not in self.tables:
            self.tables[rows] = self.ctx.msm_table_build(self.dp.ptr, self.n, None, 0, rows)
        return self.tables[rows]

    def check(self, xs, fn, what):
        """xs: the scalar vectors of the call's commitments"""
        ds = [self.ctx.upload(sc_bytes(self.nat, x)) for x in xs]
        st = stages(self.ctx, lambda: fn(ds))
        assert "short_bins" not in st and ("msm_bucket" in st or not any(any(x) for x in xs)), (what, st)
        raw = self.ctx.download(self.out.ptr, 128 * len(xs)).tobytes()
        got = [ext_affine(raw[128 * k:128 * k + 128]) for k in range(len(xs))]
        assert got == [want(x, self.exps) for x in xs], what

    def variable_base(self, x):
        ctx, n = self.ctx, self.n
        self.check([x], lambda ds: ctx.msm(ds[0].ptr, self.dp.ptr, n, None, None, 0, self.out.ptr, None), "msm")

    def rows(self, rows, xs):
        ctx, n, t = self.ctx, self.n, self.table(rows)
        if len(xs) == 1:
            self.check(xs, lambda ds: ctx.msm_table(t.ptr, n, 0, ds[0].ptr, n, None, self.out.ptr, None, rows),
                       f"rows={rows}")
        else:
            self.check(xs, lambda ds: ctx.msm_table_batch(t.ptr, n, 0, [d.ptr for d in ds], n, None, self.out.ptr,
                                                          None, rows), f"rows={rows} K={len(xs)}")


def all_entry_points(nat, ctx, rng, L, sign, seed):
    """one bucket of L entries through variable base (c = 11, a bucket set per window), the one-row table (c = 16, a
    bucket set per window), the 16-row table (c = 16, one set), the wide table (c = 20, one set) alone and three at a
    time with the heavy buckets at different values"""
    n = L + N_RANDOM
    ep = EntryPoints(nat, ctx, n, seed)
    c, W = ctx.msm_plan(n)
    assert c == 11
    ep.variable_base(run_vector(rng, L, 5, c, W, False, sign))
    ep.rows(1, [run_vector(rng, L, 1234, 16, 16, False, sign)])
    ep.rows(16, [run_vector(rng, L, 77, 16, 16, True, sign)])
    ep.rows(WIDE, [run_vector(rng, L, 300001, 20, 13, True, sign)])
    ep.rows(WIDE, [run_vector(rng, L, v, 20, 13, True, sign) for v in (2, 300001, (1 << 19) - 1)])


@pytest.mark.parametrize("sign", ["neg", "pos"])
@pytest.mark.parametrize("L", LENGTHS)
def test_run_of_one_sign(nat, monkeypatch, L, sign):
    """64-entry segments: L = 1 .. 64 is one task (the 8-entry burst up to 8, the 32-entry burst, from 33 on a
    refill), 65 is two tasks of 33 and 32 entries that end in partial sums of a split bucket"""
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        all_entry_points(nat, ctx, random.Random(9100 + 2 * L + (sign == "neg")), L, sign, 9300 + L)
    finally:
        ctx.close()


@pytest.mark.parametrize("L", LENGTHS)
def test_split_bucket_runs(nat, monkeypatch, L):
    """the planner's 8-entry segments: L entries are one task up to 8, ceil(L / 8) equal tasks above (9: 5 + 4;
    65: nine tasks of 8 and 7), every one of them a partial sum that the finish kernel adds.  And a bucket of 2 L
    entries that splits into exactly two runs of L: under 8-entry segments for L = 7, 8, under 64-entry segments for
    L = 33, 40, 64."""
    rng = random.Random(9500 + L)
    ctx = make_ctx(nat, monkeypatch, False)
    try:
        all_entry_points(nat, ctx, rng, L, "mixed", 9600 + L)
        if L in (7, 8):
            ep = EntryPoints(nat, ctx, 2 * L + N_RANDOM, 9700 + L)
            for sign in ("neg", "pos"):
                ep.rows(WIDE, [run_vector(rng, 2 * L, 4242, 20, 13, True, sign)])
    finally:
        ctx.close()
    if L in (33, 40, 64):
        ctx = make_ctx(nat, monkeypatch, True)
        try:
            ep = EntryPoints(nat, ctx, 2 * L + N_RANDOM, 9700 + L)
            for sign in ("neg", "pos"):
                ep.rows(WIDE, [run_vector(rng, 2 * L, 4242, 20, 13, True, sign)])
                ep.variable_base(run_vector(rng, 2 * L, 5, *ctx.msm_plan(ep.n), False, sign))
        finally:
            ctx.close()


def five_column_vectors(L, sign, v):
    """5 scalars below 2^240 whose 20-bit digits of rows 0 .. 10 are +-v in L of the 55 cells and 0 elsewhere; row 11
    holds a positive guard digit (another bucket) that keeps an all-negative scalar positive"""
    assert L <= 55 and v > 12
    cells = [(r, i) for r in range(11) for i in range(5)][:L]
    neg = {"pos": lambda k: False, "neg": lambda k: True, "mixed": lambda k: k % 3 == 2}[sign]
    x = [(7 + i) << 220 for i in range(5)]
    for k, (r, i) in enumerate(cells):
        x[i] += (-v if neg(k) else v) << (20 * r)
    digits = [recode_wide(s, i) for i, s in enumerate(x)]
    signed = [d for row in digits for d in row if abs(d) == v]
    assert len(signed) == L and all(0 < s < (1 << 240) for s in x)
    if sign != "mixed":
        assert all((d < 0) == (sign == "neg") for d in signed)
    return x


@pytest.mark.parametrize("sign", ["neg", "pos", "mixed"])
@pytest.mark.parametrize("L", [length for length in LENGTHS if length <= 55])
def test_wide_table_of_5_columns(nat, monkeypatch, L, sign):
    """all 13 x 5 table entries feed one bucket set: the run collects entries of several rows of the same columns;
    alone and three commitments at a time"""
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        ep = EntryPoints(nat, ctx, 5, 9800 + L)
        ep.rows(WIDE, [five_column_vectors(L, sign, 300001)])
        ep.rows(WIDE, [five_column_vectors(L, sign, v) for v in (13, 300001, (1 << 19) - 1)])
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def points_8193():
    rng = random.Random(9900)
    return [rng.randrange(1, ELL) for _ in range(8193)]


@pytest.mark.parametrize("L", LENGTHS)
def test_wide_table_of_8193_columns(nat, monkeypatch, points_8193, L):
    """one column more than a sort chunk of 8192 per table row; the run's sign alternates with L"""
    n = 8193
    rng = random.Random(9950 + L)
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        ep = EntryPoints(nat, ctx, n, 0, exps=points_8193)
        ep.rows(WIDE, [run_vector(rng, L, 300001, 20, 13, True, "neg" if L & 1 else "pos", n_random=n - L)])
    finally:
        ctx.close()


def test_all_zero_scalars(nat, monkeypatch):
    """no task at all: every entry point returns the identity"""
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        n = 50
        ep = EntryPoints(nat, ctx, n, 9990)
        zero = [0] * n
        assert want(zero, ep.exps) == (0, 1)
        ep.variable_base(zero)
        ep.rows(1, [zero])
        ep.rows(16, [zero])
        ep.rows(WIDE, [zero])
        ep.rows(WIDE, [zero, run_vector(random.Random(1), 9, 300001, 20, 13, True, "neg", n_random=n - 9), zero])
    finally:
        ctx.close()
