"""vmpc_bn256_table_msm_rows_dev: one fixed-base table, several scalar rows (csrc/bn256.hip).

Table point i is e_i * g for known exponents e_i, so row r must come out as (sum_i s[r][i] e_i mod n) * g by
oracle/bn256_ref.py: one oracle scalar multiplication per checked row (55 ms each, which is why the shape sweep takes the
oracle to the rows around the group boundary and to the first and last row, and holds every row of every call byte for
byte against vmpc_bn256_table_msm_dev, the single-row entry, as well).  The table's points themselves are made by
vmpc_bn256_fixed_base_dev from the exponents; were they wrong, the oracle comparison would fail."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bn256_ref as bn

pytestmark = pytest.mark.gpu
N = bn.N
WIDTH = {1: 64, 2: 128}
ROWS = (1, 2, 15, 16, 17, 33)
MAX_ROWS = 33


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as v
    return v.get_context()


def oracle_point(group, e, _cache={}):
    """canonical bytes of e * g"""
    key = (group, e % N)
    if key not in _cache:
        _cache[key] = bn.g1_to_bytes(bn.E1.mul(e % N, bn.G1)) if group == 1 else bn.g2_to_bytes(bn.E2.mul(e % N, bn.G2))
    return _cache[key]


def to_arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)


_TABLES = {}


def table_of(ctx, group, n, seed=0):
    """(exponents, table buffer) of n points e_i * g; the first two exponents are equal (a row can cancel on them)"""
    key = (group, n, seed)
    if key not in _TABLES:
        rng = random.Random(31000 + 10 * n + group + seed)
        exps = [rng.randrange(1, N) for _ in range(n)]
        if n > 1:
            exps[1] = exps[0]
        base = bn.g1_to_bytes(bn.G1) if group == 1 else bn.g2_to_bytes(bn.G2)
        dbase, dexps = ctx.upload(np.frombuffer(base, np.uint8)), ctx.upload(to_arr(exps))
        pts = ctx.alloc(WIDTH[group] * n)
        ctx.bn256_fixed_base(group, dbase.ptr, dexps.ptr, n, pts.ptr)
        table = ctx.bn256_table_build(group, pts.ptr, n)
        ctx.sync()
        _TABLES[key] = (exps, table)
    return _TABLES[key]


def matrix_bytes(rows_of_ints, stride):
    """(rows, stride, 32) uint8: the rows' scalars, then 0xEE filler a call must not read as scalars of the row"""
    out = np.full((len(rows_of_ints), stride, 32), 0xEE, np.uint8)
    for r, row in enumerate(rows_of_ints):
        out[r, :len(row)] = to_arr(row)
    return out


def run_rows(ctx, group, table, table_n, mat, m, rows=None):
    rows = len(mat) if rows is None else rows
    d = ctx.upload(mat)
    out = ctx.alloc(WIDTH[group] * max(rows, 1))
    ctx.bn256_table_msm_rows(group, table.ptr, table_n, d.ptr, mat.shape[1], m, rows, out.ptr)
    ctx.sync()
    return ctx.download(out.ptr, WIDTH[group] * rows).reshape(rows, WIDTH[group])


def run_single(ctx, group, table, table_n, row, m, sync=True):
    d, out = ctx.upload(to_arr(row[:m]) if m else np.zeros((1, 32), np.uint8)), ctx.alloc(WIDTH[group])
    ctx.bn256_table_msm(group, table.ptr, table_n, d.ptr, m, out.ptr)
    if sync:
        ctx.sync()
    return out


def expected(group, exps, row, m):
    return oracle_point(group, sum(s * e for s, e in zip(row[:m], exps[:m])))


@pytest.mark.parametrize("table_n", [1, 9, 65, 300])
@pytest.mark.parametrize("group", [1, 2])
def test_shapes_against_the_exponent_oracle_and_the_single_row_entry(ctx, group, table_n):
    exps, table = table_of(ctx, group, table_n)
    rng = random.Random(77 * table_n + group)
    scal = [[rng.randrange(N) for _ in range(table_n)] for _ in range(MAX_ROWS)]
    for m in sorted({v for v in (1, 7, 8, 9, table_n) if v <= table_n}):
        single = [bytes(ctx.download(run_single(ctx, group, table, table_n, row, m).ptr, WIDTH[group])) for row in scal]
        for k, rows in enumerate(ROWS):
            strides = (m, m + 3) if rows == 17 else ((m, m + 3)[k % 2],)
            for stride in strides:
                got = run_rows(ctx, group, table, table_n, matrix_bytes([row[:m] for row in scal[:rows]], stride), m)
                for r in range(rows):
                    assert bytes(got[r]) == single[r], (m, rows, stride, r)
                for r in {0, 14, 15, 16, rows - 1} & set(range(rows)):
                    assert bytes(got[r]) == expected(group, exps, scal[r], m), (m, rows, stride, r)


def special_rows(exps, rng):
    n = len(exps)
    ordinary = [rng.randrange(N) for _ in range(n)]
    twin = [rng.randrange(N) for _ in range(n)]
    s = rng.randrange(1, N)
    return [ordinary,
            [0] * n,                                                  # all zero: infinity
            twin, list(twin),                                         # two identical rows
            [N - 1 if i % 3 == 0 else rng.randrange(N) for i in range(n)],
            [s] * n,                                                  # one heavy bucket per digit row
            [s, N - s] + [0] * (n - 2),                               # cancels on the two equal columns: infinity
            [rng.randrange(N) for _ in range(n)]]


@pytest.mark.parametrize("group", [1, 2])
def test_special_rows_beside_ordinary_ones(ctx, group):
    exps, table = table_of(ctx, group, 300)
    rows = special_rows(exps, random.Random(5 + group))
    got = run_rows(ctx, group, table, 300, matrix_bytes(rows, 300), 300)
    for r, row in enumerate(rows):
        assert bytes(got[r]) == expected(group, exps, row, 300), r
        assert bytes(got[r]) == bytes(ctx.download(run_single(ctx, group, table, 300, row, 300).ptr, WIDTH[group])), r
    assert not got[1].any() and not got[6].any()
    assert bytes(got[2]) == bytes(got[3]) and got[0].any()


@pytest.mark.parametrize("group", [1, 2])
def test_a_value_not_below_the_order_is_treated_as_by_the_single_row_entry(ctx, nat, group):
    """a 32-byte value >= n counts as zero and the next synchronisation says VMPC_E_NONCANON - in both entries"""
    exps, table = table_of(ctx, group, 300)
    rng = random.Random(9 + group)
    rows = [[rng.randrange(N) for _ in range(300)] for _ in range(3)]
    rows[1][4], rows[1][250] = N, (1 << 256) - 1
    d, out = ctx.upload(matrix_bytes(rows, 300)), ctx.alloc(WIDTH[group] * 3)
    ctx.bn256_table_msm_rows(group, table.ptr, 300, d.ptr, 300, 300, 3, out.ptr)
    with pytest.raises(nat.VmpcError) as ei:
        ctx.sync()
    assert ei.value.code == nat.E_NONCANON
    got = ctx.download(out.ptr, WIDTH[group] * 3).reshape(3, -1)
    one = run_single(ctx, group, table, 300, rows[1], 300, sync=False)
    with pytest.raises(nat.VmpcError) as ei:
        ctx.sync()
    assert ei.value.code == nat.E_NONCANON
    assert bytes(got[1]) == bytes(ctx.download(one.ptr, WIDTH[group]))
    as_zero = list(rows[1])
    as_zero[4] = as_zero[250] = 0
    for r, row in enumerate([rows[0], as_zero, rows[2]]):
        assert bytes(got[r]) == expected(group, exps, row, 300), r


@pytest.mark.parametrize("group", [1, 2])
def test_rows_at_the_group_boundary_do_not_depend_on_their_place(ctx, group):
    exps, table = table_of(ctx, group, 65)
    rng = random.Random(3 + group)
    scal = [[rng.randrange(N) for _ in range(65)] for _ in range(33)]
    got = run_rows(ctx, group, table, 65, matrix_bytes(scal, 65), 65)
    for r in (15, 16, 17):
        alone = run_rows(ctx, group, table, 65, matrix_bytes([scal[r]], 65), 65)
        assert bytes(alone[0]) == bytes(got[r]) == expected(group, exps, scal[r], 65), r


def call(ctx, group, table, table_n, scal_ptr, stride, m, rows, scratch_ptr, scratch_bytes, out_ptr):
    p = ctypes.c_void_p
    return ctx.lib.vmpc_bn256_table_msm_rows_dev(ctx.handle, group, p(table), table_n, p(scal_ptr), stride, m, rows,
                                                 p(scratch_ptr), scratch_bytes, p(out_ptr))


@pytest.mark.parametrize("group", [1, 2])
def test_output_does_not_depend_on_what_the_scratch_held(ctx, group):
    exps, table = table_of(ctx, group, 65)
    rng = random.Random(13 + group)
    scal = [[rng.randrange(N) for _ in range(65)] for _ in range(17)]
    scal[5] = [scal[5][0]] * 65                                   # a split bucket's partial sums live in the scratch too
    d = ctx.upload(matrix_bytes(scal, 68))
    nbytes = int(ctx.lib.vmpc_bn256_table_msm_rows_scratch_bytes(group, 65, 17))
    scratch, out = ctx.alloc(nbytes), ctx.alloc(WIDTH[group] * 17)
    got = []
    for fill in (0xA5, 0x00):
        ctx.upload_into(scratch.ptr, np.full(nbytes, fill, np.uint8))
        assert call(ctx, group, table.ptr, 65, d.ptr, 68, 65, 17, scratch.ptr, nbytes, out.ptr) == 0
        ctx.sync()
        got.append(ctx.download(out.ptr, WIDTH[group] * 17).reshape(17, -1))
    assert (got[0] == got[1]).all()
    for r in (0, 5, 16):
        assert bytes(got[0][r]) == expected(group, exps, scal[r], 65), r


def stage_counts(ctx, fn):
    """tests.test_gpu_wide_table.stages, keeping the number of brackets per stage instead of the set of names"""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    fn()
    ctx.sync()
    counts = {k: launches for k, (_, launches) in ctx.profile_read(reset=True).items() if launches}
    ctx.profile(False)
    return counts


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("rows,groups", [(16, 1), (17, 2)])
def test_one_bucket_stage_one_reduction_and_one_recombination_per_group(ctx, group, rows, groups):
    from tests.test_gpu_wide_table import stages
    _, table = table_of(ctx, group, 9)
    rng = random.Random(rows)
    d = ctx.upload(matrix_bytes([[rng.randrange(N) for _ in range(9)] for _ in range(rows)], 9))
    out = ctx.alloc(WIDTH[group] * rows)
    fn = lambda: ctx.bn256_table_msm_rows(group, table.ptr, 9, d.ptr, 9, 9, rows, out.ptr)      # noqa: E731
    assert {"bn_bucket", "bn_reduce", "bn_final", "msm_recode"} <= stages(ctx, fn)
    counts = stage_counts(ctx, fn)
    assert (counts["bn_bucket"], counts["bn_reduce"], counts["bn_final"]) == (groups,) * 3
    assert counts["msm_recode"] == rows                           # every row has its own recoding and its own sort


@pytest.mark.parametrize("group", [1, 2])
def test_argument_rules(ctx, nat, group):
    exps, table = table_of(ctx, group, 9)
    w = WIDTH[group]
    scal = [[3 + r + i for i in range(9)] for r in range(2)]
    d = ctx.upload(matrix_bytes(scal, 9))
    nbytes = int(ctx.lib.vmpc_bn256_table_msm_rows_scratch_bytes(group, 9, 2))
    scratch = ctx.alloc(nbytes)
    mark = np.full(2 * w, 0x5C, np.uint8)
    out = ctx.upload(mark)
    args = dict(table=table.ptr, table_n=9, scal_ptr=d.ptr, stride=9, m=9, rows=2, scratch_ptr=scratch.ptr,
                scratch_bytes=nbytes, out_ptr=out.ptr)
    bad = [dict(m=10, stride=10), dict(stride=8), dict(table=None), dict(scal_ptr=None), dict(scratch_ptr=None),
           dict(scratch_bytes=nbytes - 1), dict(table_n=0)]
    for change in bad:
        assert call(ctx, group, **{**args, **change}) == nat.E_INVAL, change
        ctx.sync()
        assert (ctx.download(out.ptr, 2 * w) == mark).all(), change
    assert call(ctx, group, **{**args, "out_ptr": None}) == nat.E_INVAL
    assert call(ctx, 3, **args) == nat.E_INVAL
    # rows == 0: nothing is written; m == 0: every output is infinity, with no scalars and no scratch
    assert call(ctx, group, **{**args, "rows": 0}) == 0
    ctx.sync()
    assert (ctx.download(out.ptr, 2 * w) == mark).all()
    assert call(ctx, group, **{**args, "m": 0, "stride": 0, "scal_ptr": None, "scratch_ptr": None, "scratch_bytes": 0}) == 0
    ctx.sync()
    assert not ctx.download(out.ptr, 2 * w).any()
    # and the honest call
    assert call(ctx, group, **args) == 0
    ctx.sync()
    got = ctx.download(out.ptr, 2 * w).reshape(2, w)
    for r in range(2):
        assert bytes(got[r]) == expected(group, exps, scal[r], 9)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("table_n", [1, 300, 1 << 16])
def test_scratch_query_grows_to_sixteen_rows_and_stays(ctx, group, table_n):
    q = [int(ctx.lib.vmpc_bn256_table_msm_rows_scratch_bytes(group, table_n, rows)) for rows in range(1, 40)]
    assert q[0] > 0 and all(a <= b for a, b in zip(q, q[1:]))
    assert len(set(q[15:])) == 1 and q[14] < q[15]
    assert int(ctx.lib.vmpc_bn256_table_msm_rows_scratch_bytes(group, table_n, 1 << 20)) == q[15]
    assert int(ctx.lib.vmpc_bn256_table_msm_rows_scratch_bytes(3, table_n, 1)) == 0
    assert int(ctx.lib.vmpc_bn256_table_msm_rows_scratch_bytes(group, 0, 1)) == 0


@pytest.mark.parametrize("group", [1, 2])
def test_ppvector_msm_rows_tabulated_and_not(ctx, group):
    """knowledge_of_exponent.PPVector.msm_rows over a table and, for an untabulated vector, one sum at a time"""
    from verifiable_mpc_amd import knowledge_of_exponent as koe
    n = 9
    exps, _ = table_of(ctx, group, n)
    base = bn.g1_to_bytes(bn.G1) if group == 1 else bn.g2_to_bytes(bn.G2)
    pts = ctx.alloc(WIDTH[group] * n)
    ctx.bn256_fixed_base(group, ctx.upload(np.frombuffer(base, np.uint8)).ptr, ctx.upload(to_arr(exps)).ptr, n, pts.ptr)
    ctx.sync()
    rng = random.Random(41 + group)
    scal = [[rng.randrange(N) for _ in range(n)] for _ in range(3)]
    want = [expected(group, exps, row, 7) for row in scal]
    for tabulate in (True, False):
        vec = koe.PPVector(ctx, group, pts, n, tabulate=tabulate)
        got = vec.msm_rows(ctx.upload(matrix_bytes(scal, n)), 7, 3, row_stride=n)
        assert got.shape == (3, WIDTH[group]) and [bytes(r) for r in got] == want, tabulate
        assert vec.msm_rows(ctx.upload(matrix_bytes(scal, n)), 7, 0, row_stride=n).shape == (0, WIDTH[group])
