"""The bucket stage's task records and staged index runs (csrc/msm_sort.hip k_msm_plan2, csrc/msm.hip k_msm_bucket,
csrc/bn256_impl.h gk_bucket): a task is a self-contained record (first sorted position, length, destination, split
flag), and k_msm_bucket copies a lane's run of sorted indices into LDS a window of 32 at a time.

Every case puts EXACTLY L entries into one bucket - L terms whose only non-zero digit is +-v in window 0 (scalars v and
2^c - v), checked on the CPU by recoding the scalars as the library does - beside a few dozen full-size scalars that
populate other buckets.  L walks the edges of the staging window (32), of the segment (64 under
VMPC_EXPERIMENTAL=1 VMPC_SEG_SHIFT_MIN=0, 8 as the planner picks at these sizes), of the serial finish (<= 32 partial
sums) and of the workgroup-tree finish.  Results are checked by the exponent identity: points e_i B, so the sum is
((sum s_i e_i) mod l) B by the oracle."""
import random

import numpy as np
import pytest

from oracle import ed25519_ref as ed
from tests.msm_sort_ref import recode
from tests.test_gpu_cabi import gpu_points, sc_bytes
from tests.test_gpu_wide_table import ext_affine, stages

pytestmark = pytest.mark.gpu
ELL = ed.ELL
WIDE = 13
N_RANDOM = 40
SEG64 = [1, 31, 32, 33, 63, 64, 65, 200, 64 * 33 + 5]
DEFAULT = [7, 8, 9, 300]


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


def make_ctx(nat, monkeypatch, seg64):
    """the segment length is read when the context is created"""
    if seg64:
        monkeypatch.setenv("VMPC_EXPERIMENTAL", "1")
        monkeypatch.setenv("VMPC_SEG_SHIFT_MIN", "0")
    return nat.Context(0)


def heavy_vector(rng, L, v, c, W, one_set, order=ELL, n_random=N_RANDOM):
    """L + n_random scalars in random order: L of them v or 2^c - v (digit +v / -v in window 0, and +1 in window 1 for
    the latter), the others uniform and clear of the heavy bucket.  one_set: every window feeds the same bucket set
    (fixed-base tables); otherwise window 0 has its own."""
    assert 1 < v < (1 << (c - 1))
    windows = range(W) if one_set else range(1)

    def hits(s):
        d = recode(s, c, W, order)
        return sum(1 for w in windows if abs(d[w]) == v)
    heavy = [(1 << c) - v if i % 3 == 2 else v for i in range(L)]
    rest = []
    while len(rest) < n_random:
        s = rng.randrange(order)
        if hits(s) == 0:
            rest.append(s)
    x = heavy + rest
    rng.shuffle(x)
    assert sum(hits(s) for s in x) == L
    return x


def want(x, exps):
    return ed.pt_affine(ed.pt_repeat(ed.BASE, sum(a * b for a, b in zip(x, exps)) % ELL))


def run_entry_points(nat, ctx, L, batch):
    rng = random.Random(6400 + L)
    n = L + N_RANDOM
    exps = [rng.randrange(1, ELL) for _ in range(n)]
    dp = gpu_points(nat, ctx, exps)
    out = ctx.alloc(128 * 3)

    def check(x, fn, what):
        ds = ctx.upload(sc_bytes(nat, x))
        st = stages(ctx, lambda: fn(ds))
        assert "msm_bucket" in st and "short_bins" not in st, (what, st)
        assert ext_affine(ctx.download(out.ptr, 128).tobytes()) == want(x, exps), (what, L)

    # variable base: c = 11 below 2^13 terms, every window its own bucket set
    c, W = ctx.msm_plan(n)
    assert c == 11
    check(heavy_vector(rng, L, 5, c, W, False), lambda ds: ctx.msm(ds.ptr, dp.ptr, n, None, None, 0, out.ptr, None),
          "msm")
    # 16-row table on the general path: c = 16, one bucket set
    t16 = ctx.msm_table_build(dp.ptr, n, None, 0, 16)
    ctx.set_short_path(False)
    check(heavy_vector(rng, L, 77, 16, 16, True),
          lambda ds: ctx.msm_table(t16.ptr, n, 0, ds.ptr, n, None, out.ptr, None, 16), "rows=16")
    ctx.set_short_path(True)
    # wide-window table: c = 20, one set of 2^19 buckets
    wide = ctx.msm_table_build(dp.ptr, n, None, 0, WIDE)
    check(heavy_vector(rng, L, 300001, 20, 13, True),
          lambda ds: ctx.msm_table(wide.ptr, n, 0, ds.ptr, n, None, out.ptr, None, WIDE), "rows=13")
    if batch:
        # three commitments in one pass, their heavy buckets at different values: a record with another
        # commitment's offset or destination gives a wrong sum
        xs = [heavy_vector(rng, L, v, 20, 13, True) for v in (2, 300001, (1 << 19) - 1)]
        ds = [ctx.upload(sc_bytes(nat, x)) for x in xs]
        ctx.msm_table_batch(wide.ptr, n, 0, [d.ptr for d in ds], n, None, out.ptr, None, WIDE)
        raw = ctx.download(out.ptr, 128 * 3).tobytes()
        assert [ext_affine(raw[128 * k:128 * k + 128]) for k in range(3)] == [want(x, exps) for x in xs], L


@pytest.mark.parametrize("L", SEG64)
def test_heavy_bucket_with_64_entry_segments(nat, monkeypatch, L):
    """L = 1 .. 64: one task on either side of the staging window and of the segment; 65, 200: 2 - 4 segments, summed
    by one lane; 64 * 33 + 5: 34 partial sums, summed by the workgroup tree"""
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        run_entry_points(nat, ctx, L, batch=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("L", DEFAULT)
def test_heavy_bucket_with_the_planners_segments(nat, monkeypatch, L):
    """8-entry segments at these sizes: one task, one full segment, two, and 38 (the workgroup tree)"""
    ctx = make_ctx(nat, monkeypatch, False)
    try:
        run_entry_points(nat, ctx, L, batch=False)
    finally:
        ctx.close()


def test_bn256_heavy_bucket_full_segment_plus_remainder(nat, monkeypatch):
    """G1, n = 300 (c = 6): 70 entries in one bucket of window 0 are one full 64-entry segment plus a remainder of 6
    (BN-256 plans are not balanced), two task records that gk_finish_light adds"""
    from oracle import bn256_ref as bn
    from tests import bn256_msm_inputs as mi
    from tests.test_gpu_bn256 import walk_points
    from tests.test_gpu_bn256_edges import arr32, dot, host_points
    n, L = 300, 70
    rng = random.Random(7006)
    c, W = mi.make_plan(n)
    assert c == 6
    exps, pts = walk_points(bn.E1, bn.G1, rng, n)
    x = heavy_vector(rng, L, 9, c, W, False, order=bn.N, n_random=n - L)
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        dp, ds, out = ctx.upload(host_points(1, pts)), ctx.upload(arr32(x)), ctx.alloc(64)
        ctx.bn256_msm(1, ds.ptr, dp.ptr, n, out.ptr)
        ctx.sync()
        assert ctx.download(out.ptr, 64).tobytes() == bn.g1_to_bytes(bn.E1.mul(dot(x, exps), bn.G1))
    finally:
        ctx.close()
