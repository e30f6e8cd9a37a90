"""The MSM sort front end (csrc/msm_sort.hip) stage by stage against its CPU restatement (tests/msm_sort_ref.py).

Every case is ONE call of a real entry point at the smallest shape that reaches a path of the sort.  After it the MSM
result is checked by the exponent identity (points e_i B, so the sum is ((sum s_i e_i) mod order) B by the oracle),
the view of the sort's arrays (Context.msm_sort_view) goes through check_view - which names the stage that broke -
and the facts that say WHICH path the case took are asserted from the view: window width, bin geometry, the number of
coarse bins beyond the LDS stage (ctrl[3]), whether the entry between the passes carries the fine bucket, ...
A case prints one `SORTVIEW` line with the plan and the counters it saw (EXPERIMENTS.md keeps the table)."""
import random

import numpy as np
import pytest

from oracle import ed25519_ref as ed
from tests import msm_sort_ref as ref
from tests.test_gpu_bucket_runs import heavy_vector
from tests.test_gpu_cabi import gpu_points, sc_bytes
from tests.test_gpu_wide_table import ext_affine

pytestmark = pytest.mark.gpu
ELL = ed.ELL
WIDE = 13
MSM_STAGES = {"msm_prep", "msm_recode", "msm_hist", "msm_part", "msm_sort", "msm_plan", "msm_bucket",
              "msm_bucket_finish", "msm_reduce", "msm_final"}


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


def env_ctx(nat, **env):
    """a context created under VMPC_EXPERIMENTAL=1 and the given knobs (they are read when the context is created)"""
    with pytest.MonkeyPatch.context() as mp:
        if env:
            mp.setenv("VMPC_EXPERIMENTAL", "1")
        for k, v in env.items():
            mp.setenv(k, str(v))
        return nat.Context(0)


@pytest.fixture(scope="module")
def ctxs(nat):
    """False: the planner's segments (8 entries at these sizes); True: 64-entry segments"""
    c = {False: env_ctx(nat), True: env_ctx(nat, VMPC_SEG_SHIFT_MIN=0)}
    yield c
    for v in c.values():
        v.close()


def edge_scalars(c, order=ELL):
    return [v for v in (1 << (c - 1), (1 << (c - 1)) - 1, (1 << 252) - 1, 1 << 252, order - 1, 1, 0) if v < order]


def rand_vec(rng, n, c, order=ELL):
    """uniform scalars carrying the edge scalars (as many as fit; a single scalar is 2^(c-1))"""
    x = [rng.randrange(order) for _ in range(n)]
    edge = edge_scalars(c, order)
    for k in range(min(n, len(edge))):
        x[(k * 7919 + n // 2) % n if n > len(edge) else k] = edge[k]
    return x


def want_ed(x, exps):
    return ed.pt_affine(ed.pt_repeat(ed.BASE, sum(a * b for a, b in zip(x, exps)) % ELL))


def log_view(name, p, A):
    print("\nSORTVIEW | %s | %d | %d | %d | %d | %d | %d | %d | %d | %d | %d | %s | %d |" % (
        name, p["c"], p["W"], p["period"], p["LB"], p["LB_top"], p["NC"], p["J"], p["seg_shift"], p["balanced"],
        p["fine_in_entry"], " ".join(str(int(v)) for v in A["ctrl"][:5]), len(A["tasks"])))


def checked_view(ctx, name, kind, commitments, **kw):
    """the view of the call just made, through check_view: (plan, arrays, expected digits, Expect)"""
    plan, A = ctx.msm_sort_view()
    D = ref.expected_digits(kind, plan, commitments, **kw)
    e = ref.check_view(plan, A, D)
    log_view(name, plan, A)
    return plan, A, D, e


def run_msm(nat, ctx, name, x, extras=(), window=0, rng=None):
    """vmpc_msm_dev over len(x) + len(extras) terms: result by the exponent identity, then the checked view"""
    rng = rng or random.Random(len(x))
    n, ne = len(x), len(extras)
    exps = [rng.randrange(1, ELL) for _ in range(n + ne)]
    dp = gpu_points(nat, ctx, exps[:n])
    de = gpu_points(nat, ctx, exps[n:]) if ne else None
    ds = ctx.upload(sc_bytes(nat, x))
    dx = ctx.upload(sc_bytes(nat, list(extras))) if ne else None
    out = ctx.alloc(128)
    ctx.set_window(window)
    try:
        ctx.msm(ds.ptr, dp.ptr, n, dx.ptr if ne else None, de.ptr if ne else None, ne, out.ptr, None)
        view = checked_view(ctx, name, "msm", [(x, list(extras))])
    finally:
        ctx.set_window(0)
    assert ext_affine(ctx.download(out.ptr, 128).tobytes()) == want_ed(list(x) + list(extras), exps), name
    return view


# ---- the view itself ------------------------------------------------------------------------------------------------
def test_view_is_refused_without_a_sort_and_adds_no_stage(nat):
    ctx = nat.Context(0)
    try:
        with pytest.raises(nat.VmpcError) as ei:
            ctx.msm_sort_view()                               # nothing has run
        assert ei.value.code == nat.E_INVAL
        rng = random.Random(1)
        n = 40
        exps = [rng.randrange(1, ELL) for _ in range(n)]
        dp, out = gpu_points(nat, ctx, exps), ctx.alloc(128)
        x = rand_vec(rng, n, 11)
        ds = ctx.upload(sc_bytes(nat, x))
        ctx.profile(True)
        ctx.profile_read(reset=True)
        ctx.msm(ds.ptr, dp.ptr, n, None, None, 0, out.ptr, None)
        plan, A = ctx.msm_sort_view()
        plan2, A2 = ctx.msm_sort_view()                       # reading it changes nothing
        st = {k: launches for k, (_, launches) in ctx.profile_read(reset=True).items() if launches}
        ctx.profile(False)
        assert set(st) == MSM_STAGES and set(st.values()) == {1}, st
        assert plan == plan2 and all(np.array_equal(A[k], A2[k]) for k in A)
        assert A["digits"].dtype == np.int16 and A["tasks"].shape == (A["ctrl"][1], 4)
        assert ctx.validate_points(dp.ptr, n) == 0            # takes the arena: the sort's arrays are void
        with pytest.raises(nat.VmpcError) as ei:
            ctx.msm_sort_view()
        assert ei.value.code == nat.E_INVAL
        # the fused short path does not sort
        t16 = ctx.msm_table_build(dp.ptr, n, None, 0, 16)
        ctx.msm_table(t16.ptr, n, 0, ds.ptr, n, None, out.ptr, None, 16)
        ctx.sync()
        assert ext_affine(ctx.download(out.ptr, 128).tobytes()) == want_ed(x, exps)
        with pytest.raises(nat.VmpcError) as ei:
            ctx.msm_sort_view()
        assert ei.value.code == nat.E_INVAL
        ctx.set_short_path(False)
        ctx.msm_table(t16.ptr, n, 0, ds.ptr, n, None, out.ptr, None, 16)
        plan, A = ctx.msm_sort_view()
        assert plan["c"] == 16 and plan["W"] == 1 and A["hist1"][-1] == len(A["sorted"]) > 0
    finally:
        ctx.close()


# ---- Ed25519 msm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_extra", [(1, 0), (7, 0), (8, 0), (9, 0), (200, 0), (200, 3)])
def test_msm_small(nat, ctxs, n, n_extra):
    rng = random.Random(100 + n + n_extra)
    x = rand_vec(rng, n, 11)
    p, A, D, e = run_msm(nat, ctxs[False], f"msm n={n}+{n_extra}", x, rand_vec(rng, n_extra, 11)[:n_extra], rng=rng)
    assert (p["c"], p["NC"], p["top_row"], p["LB_top"]) == (11, 2, p["W"] - 1, 0)
    assert p["n_pad"] == (n + n_extra + 7) // 8 * 8 and p["seg_shift"] == -3


@pytest.mark.parametrize("c", [4, 5, 13, 16])
def test_msm_set_window(nat, ctxs, c):
    rng = random.Random(200 + c)
    x = rand_vec(rng, 200, c)
    p, A, D, e = run_msm(nat, ctxs[False], f"msm n=200 window={c}", x, window=c, rng=rng)
    assert p["c"] == c and p["W"] == (255 + c - 1) // c and p["top_row"] == p["W"] - 1
    assert p["top_max_b"] == (ELL - 1) >> (c * (p["W"] - 1))
    if c == 4:
        assert p["W"] == 64
    if c == 16:
        assert p["LB_top"] < p["LB"] and e.unreachable.any()
        top = D[15]
        assert top.max() == p["top_max_b"] == 4096              # l - 1 reaches the largest top bucket
        k = x.index((1 << 252) - 1)
        assert top[k] == 4096 and (x[k] >> 240) == 4095          # ... and 2^252 - 1 gets there by a carry


@pytest.mark.parametrize("n,J,c", [(8191, 1, 11), (8192, 1, 11), (8193, 2, 16), (16385, 3, 16)])
def test_msm_chunk_edges(nat, ctxs, n, J, c):
    rng = random.Random(n)
    p, A, D, e = run_msm(nat, ctxs[False], f"msm n={n}", rand_vec(rng, n, c), rng=rng)
    assert (p["J"], p["c"]) == (J, c) and A["ctrl"][3] == 0


def one_bin(rng, n, heavy=0):
    """n scalars (c = 16) whose window-0 digit lies in coarse bin 0 - buckets 1 .. 512, either sign - spread evenly over
    the bin's fine buckets; the first `heavy` of them all in bucket 77.  The other windows are uniform."""
    out = []
    for i in range(n):
        v = 77 if i < heavy else 1 + (i * 131) % 512
        low = v if (i % 3 or i < heavy) else (1 << 16) - v
        out.append((rng.randrange(1 << 235) << 16) | low)
    return out


def bin0_fill(p, e):
    return int(e.bin_fill[0])           # (row 0, coarse bin 0)


def test_msm_bin_fills_the_stage_exactly(nat, ctxs):
    """12288 entries in one coarse bin: the last size k_sort_fine stages in LDS"""
    rng = random.Random(12288)
    p, A, D, e = run_msm(nat, ctxs[False], "msm n=12288 one bin", one_bin(rng, 12288), rng=rng)
    assert p["c"] == 16 and p["fine_cap"] == 12288 and bin0_fill(p, e) == 12288
    assert A["ctrl"][3] == 0


def test_msm_bin_one_past_the_stage(nat, ctxs):
    """12289: k_sort_fine only counts the bin, k_sort_fine_big sorts it in two tiles, one wave per bucket run"""
    rng = random.Random(12289)
    p, A, D, e = run_msm(nat, ctxs[False], "msm n=12289 one bin", one_bin(rng, 12289), rng=rng)
    assert bin0_fill(p, e) == 12289 and A["ctrl"][3] == 1
    assert e.counts[1:513].max() <= 512 and e.counts[1:513].min() >= 1


@pytest.mark.parametrize("seg64", [False, True])
def test_msm_one_scalar_repeated(nat, ctxs, seg64):
    """12289 copies of one scalar: every window has ONE bucket of 12289 entries - a tiled bin whose waves are
    uniform (the ballot branch) and whose single run is longer than 512 (the whole-workgroup copy)"""
    rng = random.Random(777)
    while True:
        s = rng.randrange(ELL)
        if all(ref.recode(s, 16, 16, ELL)):
            break
    p, A, D, e = run_msm(nat, ctxs[seg64], f"msm n=12289 one scalar seg64={int(seg64)}", [s] * 12289, rng=rng)
    assert A["ctrl"][3] == 16 and e.counts.max() == 12289 > 512 and A["ctrl"][4] == 16
    assert e.seg == (64 if seg64 else 8)


def test_msm_two_tiles_and_a_rest_with_both_copy_branches(nat, ctxs):
    """2 * 12288 + 1 entries in one bin: two full tiles and a one-entry tile; the first 600 terms share a bucket, so
    the first tile has one run beyond 512 (whole workgroup) among runs copied by single waves"""
    rng = random.Random(24577)
    p, A, D, e = run_msm(nat, ctxs[False], "msm n=24577 one bin, bucket of 600", one_bin(rng, 24577, heavy=600),
                         rng=rng)
    assert bin0_fill(p, e) == 2 * 12288 + 1 and A["ctrl"][3] == 1
    assert e.counts[77] >= 600 and np.delete(e.counts[1:513], 76).max() <= 512
    assert (np.abs(D[0, :600]) == 77).all()            # all in chunk 0: the bin's first tile


# ---- 16-row-family tables, general path -----------------------------------------------------------------------------
def run_table(nat, ctx, name, rows, table, table_n, exps, coms, m, windows=16):
    """vmpc_msm_table(_batch)_dev for the commitments `coms` = [(scalars, extras)]: results, then the checked view"""
    K, ne = len(coms), len(coms[0][1])
    ds = [ctx.upload(sc_bytes(nat, x)) for x, _ in coms]
    dx = [ctx.upload(sc_bytes(nat, ex)) for _, ex in coms] if ne else None
    out = ctx.alloc(128 * K)
    if K == 1:
        ctx.msm_table(table.ptr, table_n, ne, ds[0].ptr, m, dx[0].ptr if ne else None, out.ptr, None, rows)
    else:
        ctx.msm_table_batch(table.ptr, table_n, ne, [d.ptr for d in ds], m, [d.ptr for d in dx] if ne else None,
                            out.ptr, None, rows)
    view = checked_view(ctx, name, "wide" if rows == WIDE else "rows", [(x[:m], ex) for x, ex in coms],
                        table_n=table_n, rows=rows, windows=windows)
    raw = ctx.download(out.ptr, 128 * K).tobytes()
    for k, (x, ex) in enumerate(coms):
        assert ext_affine(raw[128 * k:128 * k + 128]) == want_ed(x[:m] + ex, exps[:m] + exps[table_n:]), (name, k)
    return view


def build_table(nat, ctx, rng, table_n, ne, rows):
    exps = [rng.randrange(1, ELL) for _ in range(table_n + ne)]
    dp = gpu_points(nat, ctx, exps[:table_n])
    de = gpu_points(nat, ctx, exps[table_n:]) if ne else None
    return exps, ctx.msm_table_build(dp.ptr, table_n, de.ptr if ne else None, ne, rows)


@pytest.mark.parametrize("rows", [1, 2, 4, 16])
def test_row_tables(nat, ctxs, rows):
    """300 columns + 3 extras, m = 123 < table_n: the columns [m, table_n) are zero.  The one-row table has every window
    in a row of its own - its top window is a top row when the call's window equals the table's 16 bits (the planner
    itself picks c = 11 for 2400 positions, and the table plan then has no top row)"""
    ctx = ctxs[False]
    rng = random.Random(300 + rows)
    exps, table = build_table(nat, ctx, rng, 300, 3, rows)
    ctx.set_short_path(False)
    ctx.set_window(16 if rows == 1 else 0)
    try:
        coms = [(rand_vec(rng, 123, 16), rand_vec(rng, 3, 16)[:3])]
        p, A, D, e = run_table(nat, ctx, f"table rows={rows}", rows, table, 300, exps, coms, 123)
    finally:
        ctx.set_window(0)
        ctx.set_short_path(True)
    assert (p["c"], p["period"], p["W"], p["n_pad"]) == (16, 16 // rows, 16 // rows, rows * 304)
    assert p["top_row"] == (15 if rows == 1 else -1)
    if rows == 1:
        assert p["top_max_b"] == 4096 and p["LB_top"] < p["LB"]
    assert not D.reshape(p["W"], rows, 304)[:, :, 123:300].any() and D.reshape(p["W"], rows, 304)[:, :, 300:303].any()


@pytest.mark.parametrize("seg64", [False, True])
def test_row_table_batch_of_three(nat, ctxs, seg64):
    """rows = 4, K = 3: W = 12 digit rows; 70 terms share a bucket, at a different value in every commitment"""
    ctx = ctxs[seg64]
    rng = random.Random(443)
    n = 70 + 40
    exps, table = build_table(nat, ctx, rng, n, 0, 4)
    ctx.set_short_path(False)
    try:
        coms = [(heavy_vector(rng, 70, v, 16, 16, True), []) for v in (2, 30001, (1 << 15) - 1)]
        p, A, D, e = run_table(nat, ctx, f"table rows=4 K=3 seg64={int(seg64)}", 4, table, n, exps, coms, n)
    finally:
        ctx.set_short_path(True)
    assert (p["W"], p["period"]) == (12, 4) and e.seg == (64 if seg64 else 8)
    heavy = np.nonzero(e.counts >= 70)[0]
    assert sorted(int(h) % p["nb1"] for h in heavy) == [2, 30001, (1 << 15) - 1]
    assert sorted(int(h) // p["nb1"] // 4 for h in heavy) == [0, 1, 2]          # one per commitment


BIG_COLS = (1 << 18) + 5


@pytest.fixture(scope="module")
def big_table(nat):
    """16 rows over 2^18 + 5 columns + 3 extras (512 MiB): a digit row of more than 2^22 positions, in a context whose
    sort keeps 9 fine bits - 23 index bits + 9 fine bits do not fit the entry, so the fine sort re-reads the digit
    (FINE_IN_ENTRY = false)"""
    ctx = env_ctx(nat, VMPC_SORT_FINE_BITS=9)
    rng = random.Random(18)
    exps, table = build_table(nat, ctx, rng, BIG_COLS, 3, 16)
    ctx.set_short_path(False)
    yield ctx, exps, table
    ctx.close()


def test_big_table_fine_bucket_not_in_entry(nat, big_table):
    ctx, exps, table = big_table
    rng = random.Random(5000)
    x = [v or 1 for v in rand_vec(rng, 5000, 16)]
    p, A, D, e = run_table(nat, ctx, "table rows=16 2^18+5 cols m=5000", 16, table, BIG_COLS, exps,
                           [(x, rand_vec(rng, 3, 16)[:3])], 5000)
    assert (p["idx_bits"], p["fine_in_entry"], p["LB"], p["NC"]) == (23, 0, 9, 64)
    assert A["ctrl"][3] == 0 and int((A["sorted"] & 0x7fffffff).max()) >= 1 << 22


def test_big_table_fine_bucket_not_in_entry_tiled(nat, big_table):
    ctx, exps, table = big_table
    rng = random.Random(12500)
    while True:
        s = rng.randrange(ELL)
        if all(ref.recode(s, 16, 16, ELL)):
            break
    p, A, D, e = run_table(nat, ctx, "table rows=16 2^18+5 cols 12500 copies", 16, table, BIG_COLS, exps,
                           [([s] * 12500, rand_vec(rng, 3, 16)[:3])], 12500)
    assert (p["idx_bits"], p["fine_in_entry"]) == (23, 0)
    assert A["ctrl"][3] >= 1 and e.counts.max() >= 12500


# ---- wide-window table ----------------------------------------------------------------------------------------------
def wide_vec(rng, n):
    """scalars on both sides of 2^240 (k_msm_recode_wide adds a multiple of l from there on) with the edges of both"""
    x = [rng.randrange(ELL) if i % 2 else rng.randrange(1 << rng.randrange(1, 241)) for i in range(n)]
    edge = edge_scalars(20) + [(1 << 240) - 1, 1 << 240]
    for k in range(min(n, len(edge))):
        x[(k * 7919 + n // 2) % n if n > len(edge) else k] = edge[k]
    return x


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("cols,cpr", [(5, 1), (8192, 1), (8193, 2)])
def test_wide_table(nat, ctxs, cols, cpr, K):
    """`cols` table columns, the last two of them extras: 8192 fill one sort chunk per table row, 8193 need two"""
    ctx = ctxs[False]
    rng = random.Random(cols + K)
    tn = cols - 2
    exps, table = build_table(nat, ctx, rng, tn, 2, WIDE)
    ctx.set_short_path(False)
    try:
        coms = [(wide_vec(rng, tn), wide_vec(rng, 2)[:2]) for _ in range(K)]
        p, A, D, e = run_table(nat, ctx, f"wide cols={cols} K={K}", WIDE, table, tn, exps, coms, tn)
    finally:
        ctx.set_short_path(True)
    assert (p["wide"], p["chunks_per_row"], p["W"], p["period"], p["c"]) == (1, cpr, K, 1, 20)
    assert p["row_stride"] == 8192 * cpr and A["digits"].dtype == np.int32 and p["fine_cap"] == 16384
    for k, (x, ex) in enumerate(coms):              # the digits are recode_wide's, scalar by scalar
        for i in list(range(min(tn, 12))) + [tn - 1]:
            assert list(A["digits"][k, i::p["row_stride"]]) == ref.recode_wide(x[i], i), (k, i)
        assert list(A["digits"][k, tn + 1::p["row_stride"]]) == ref.recode_wide(ex[1], tn + 1)


@pytest.mark.parametrize("shape", ["three_rows", "short_row_0"])
def test_wide_table_tiled_bin(nat, ctxs, shape):
    """8192 columns, every scalar v (1 + 2^20 + 2^40): 24576 entries of table rows 0 .. 2 in ONE bucket, a bin beyond
    the wide window's 16384-entry stage - its tile boundary falls between table rows 1 and 2.  short_row_0: only the
    first 5000 scalars have the digit of row 0, which moves the boundary INTO table row 2 (sort_row_offset must tell
    the rows apart inside a tile)."""
    ctx = ctxs[False]
    rng = random.Random(8192)
    v = rng.randrange(1, 1 << 19)
    x = [v * (1 + (1 << 20) + (1 << 40))] * 8192
    if shape == "short_row_0":
        x[5000:] = [v * ((1 << 20) + (1 << 40))] * (8192 - 5000)
    exps, table = build_table(nat, ctx, rng, 8192, 0, WIDE)
    ctx.set_short_path(False)
    try:
        p, A, D, e = run_table(nat, ctx, f"wide 8192 cols one bucket {shape}", WIDE, table, 8192, exps, [(x, [])], 8192)
    finally:
        ctx.set_short_path(True)
    fill = 24576 if shape == "three_rows" else 5000 + 2 * 8192
    assert (p["wide"], p["chunks_per_row"]) == (1, 1) and e.counts[v] == fill > p["fine_cap"]
    assert A["ctrl"][3] == 1 and A["ctrl"][4] == 1
    pos = np.sort(A["sorted"] & 0x7fffffff)
    rows_of = np.bincount(pos // p["row_stride"], minlength=3)
    assert list(rows_of) == ([8192] * 3 if shape == "three_rows" else [5000, 8192, 8192])   # row * row_stride + column


# ---- BN-256, G1 -----------------------------------------------------------------------------------------------------
def bn_setup():
    from oracle import bn256_ref as bn
    from tests import bn256_msm_inputs as mi
    from tests.test_gpu_bn256 import walk_points
    from tests.test_gpu_bn256_edges import arr32, assert_jac, dot, host_points
    return bn, mi, walk_points, arr32, assert_jac, dot, host_points


@pytest.mark.parametrize("n,heavy,seg64", [(17, 0, False), (300, 0, False), (300, 70, False), (300, 70, True)])
def test_bn256_msm(nat, ctxs, n, heavy, seg64):
    bn, mi, walk_points, arr32, _, dot, host_points = bn_setup()
    ctx = ctxs[seg64]
    rng = random.Random(256 + n + heavy)
    c, W = mi.make_plan(n)
    exps, pts = walk_points(bn.E1, bn.G1, rng, n)
    if heavy:
        x = heavy_vector(rng, heavy, 9, c, W, False, order=bn.N, n_random=n - heavy)
    else:
        x = rand_vec(rng, n, c, bn.N)
    dp, ds, out = ctx.upload(host_points(1, pts)), ctx.upload(arr32(x)), ctx.alloc(64)
    ctx.bn256_msm(1, ds.ptr, dp.ptr, n, out.ptr)
    p, A, D, e = checked_view(ctx, f"bn256_msm n={n} heavy={heavy} seg64={int(seg64)}", "msm", [(x, [])], order=bn.N)
    assert ctx.download(out.ptr, 64).tobytes() == bn.g1_to_bytes(bn.E1.mul(dot(x, exps), bn.G1))
    assert (p["c"], p["W"], p["balanced"], p["top_row"]) == (c, W, 0, W - 1)
    assert p["top_max_b"] == (bn.N - 1) >> (c * (W - 1))
    if heavy:
        assert e.counts[9] == 70 and e.seg == (64 if seg64 else 8)
        mine = A["tasks"][(A["tasks"][:, 0] >= e.starts[9]) & (A["tasks"][:, 0] < e.starts[9] + 70)]
        assert sorted(mine[:, 1]) == ([6, 64] if seg64 else [6] + [8] * 8)      # full segments plus a remainder
        assert (mine[:, 3] == 1).all()


def test_bn256_table_msm_and_multi(nat, ctxs):
    """the 17-row BN-256 table is one digit row [window][column]; the K-key pass sorts once for all its keys"""
    bn, mi, walk_points, arr32, assert_jac, dot, host_points = bn_setup()
    ctx = ctxs[False]
    rng = random.Random(40)
    n, K = 40, 3
    keys = [walk_points(bn.E1, bn.G1, rng, n) for _ in range(K)]
    dps = [ctx.upload(host_points(1, pts)) for _, pts in keys]
    tables = [ctx.bn256_table_build(1, dp.ptr, n) for dp in dps]
    x = rand_vec(rng, n, 16, bn.N)
    ds, out, jac = ctx.upload(arr32(x)), ctx.alloc(64), ctx.alloc(96 * K)
    for m in (n, 33):
        ctx.bn256_table_msm(1, tables[0].ptr, n, ds.ptr, m, out.ptr, None)
        p, A, D, e = checked_view(ctx, f"bn256_table_msm n=40 m={m}", "rows", [(x[:m], [])], order=bn.N, table_n=n,
                                  rows=17, windows=17)
        assert ctx.download(out.ptr, 64).tobytes() == bn.g1_to_bytes(bn.E1.mul(dot(x[:m], keys[0][0]), bn.G1))
        assert (p["c"], p["W"], p["n_pad"], p["balanced"], p["top_row"]) == (16, 1, 17 * 40, 0, -1)
        ctx.bn256_table_msm_multi(1, [t.ptr for t in tables], n, ds.ptr, m, jac.ptr)
        p2, A2, _, _ = checked_view(ctx, f"bn256_table_msm_multi K=3 m={m}", "rows", [(x[:m], [])], order=bn.N,
                                    table_n=n, rows=17, windows=17)
        assert p2 == p and np.array_equal(np.sort(A2["sorted"]), np.sort(A["sorted"]))
        raw = ctx.download(jac.ptr, 96 * K).tobytes()
        for k in range(K):
            assert_jac(1, raw[96 * k:96 * k + 96], bn.E1.mul(dot(x[:m], keys[k][0]), bn.G1), (k, m))
