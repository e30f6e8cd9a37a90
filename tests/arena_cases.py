"""One case per library function that takes scratch memory from a context's arena (vmpc_ws_reserve, csrc/common.h):
the rule under test is that a call's result is a function of its arguments, never of what the arena held before it
(DESIGN.md "Arena independence").  tests/test_gpu_arena_independence.py runs every case on a fresh context, then over
an arena filled with 0, 1 and 0x0100 (vmpc_ctx_debug_arena_fill), then after ANOTHER case of this table has used the
same arena; tests/test_arena_cases_inventory.py (no GPU) checks that the table names every function of csrc/ that
reserves the arena.

A case:
  name      the test id
  targets   the ("file", "function") pairs of csrc/ that the case reaches and that reserve the arena
  source    the existing test whose shape the case copies: the smallest one there that reaches every stage of the target
            that takes arena memory
  foreign   the case that runs first on the same context in the "foreign" state: a different one that needs at least as
            large an arena, so that what this case takes has been written by other code (the largest case takes the
            second largest; the sizes as measured are in EXPERIMENTS.md A.1)
  run(ctx)  uploads the inputs, calls the public entry, synchronises and returns the output as canonical bytes
  want()    the same bytes from an oracle the suite already has (oracle/*.py, tests/*_ref.py, Python integers); None for
            the prover, whose run verifies the proof it made

Inputs and expected bytes are made once per process (memo) and never changed.  No fill value, here or in the test, is
above 0xFFFF: a kernel that trusts a stale count or index then computes a wrong value, not a far address.
"""
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# functions that reserve the arena and return timings, not values: no arena state can make them "wrong"
EXEMPT = {
    ("msm.hip", "vmpc_ed25519_madd_rate"): "rate probe: returns a timing",
    ("bn256_probe.hip", "bn_madd_rate"): "rate probe: returns a timing",
    ("probe.hip", "vmpc_gather_probe_dev"): "gather probe: returns a timing",
}

_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def nat():
    from verifiable_mpc_amd import _native
    return _native


def le32(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def arr32(vals):
    return nat().ints_to_array([int(v) for v in vals], 32)


def rand32(seed, n):
    """(n, 32) uint8 of any 32-byte values"""
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


def ints_of(a):
    import numpy as np
    raw = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def get(ctx, buf, nbytes):
    ctx.sync()
    return ctx.download(buf.ptr, nbytes).tobytes()


def stages(ctx, fn):
    """the names of the profile stages that ran inside fn()"""
    from tests.test_gpu_wide_table import stages as st
    return st(ctx, fn)


# ---- Ed25519: canonical forms ----------------------------------------------------------------------------------------

def ed_aff(pt):
    """an affine (x, y, ..) tuple as x || y, 32-byte little-endian each"""
    return int(pt[0]).to_bytes(32, "little") + int(pt[1]).to_bytes(32, "little")


def ed_ext_canon(raw):
    """extended (X, Y, Z, T) outputs, 128 bytes each -> the affine points (the representative is not the contract)"""
    from tests.test_gpu_wide_table import ext_affine
    return b"".join(ed_aff(ext_affine(raw[o:o + 128])) for o in range(0, len(raw), 128))


def ed_aff_canon(raw):
    from oracle import ed25519_ref as ed
    return b"".join(ed_aff(ed.affine_from_bytes(raw[o:o + 64])) for o in range(0, len(raw), 64))


def ed_exp_point(total):
    """(total mod l) B as canonical affine bytes: the exponent identity over points e_i B"""
    from oracle import ed25519_ref as ed
    return ed_aff(ed.pt_affine(ed.pt_repeat(ed.BASE, total % ed.ELL)))


def ed_dot(x, exps):
    return sum(a * b for a, b in zip(x, exps))


def ed_inputs(seed, n):
    from oracle import ed25519_ref as ed
    rng = random.Random(seed)
    return rng, [rng.randrange(1, ed.ELL) for _ in range(n)]


# ---- msm.hip -----------------------------------------------------------------------------------------------------------
# tests/test_gpu_bucket_runs.py: L = 300 entries in ONE bucket beside 40 uniform scalars.  With the planner's 8-entry
# segments that is 38 partial sums, summed by the workgroup tree (DEFAULT = [7, 8, 9, 300] there)
HEAVY_L, HEAVY_RANDOM = 300, 40


def _heavy(key, v, c, W, one_set):
    def make():
        from tests.test_gpu_bucket_runs import heavy_vector
        rng, exps = ed_inputs(6400 + HEAVY_L + v, HEAVY_L + HEAVY_RANDOM)
        return exps, heavy_vector(rng, HEAVY_L, v, c, W, one_set)
    return memo(key, make)


def ed_msm_run(ctx):
    from tests.test_gpu_cabi import gpu_points, sc_bytes
    n = HEAVY_L + HEAVY_RANDOM
    c, W = ctx.msm_plan(n)
    assert c == 11                              # variable base below 2^13 terms: every window its own bucket set
    exps, x = _heavy("ed_msm", 5, c, W, False)
    dp, ds, out = gpu_points(nat(), ctx, exps), ctx.upload(sc_bytes(nat(), x)), ctx.alloc(128)
    st = stages(ctx, lambda: ctx.msm(ds.ptr, dp.ptr, n, None, None, 0, out.ptr, None))
    assert "msm_bucket" in st, st
    return ed_ext_canon(get(ctx, out, 128))


def ed_msm_want():
    exps, x = _MEMO["ed_msm"]                   # (made by the first run: the plan is the context's to state)
    return ed_exp_point(ed_dot(x, exps))


WIDE, WIDE_VALUES = 13, (2, 300001, (1 << 19) - 1)


def ed_wide_run(ctx):
    """three commitments in one pass over the 13-row wide-window table, their heavy buckets at different values"""
    from tests.test_gpu_cabi import gpu_points, sc_bytes
    n = HEAVY_L + HEAVY_RANDOM
    exps = _heavy(("ed_wide", WIDE_VALUES[0]), WIDE_VALUES[0], 20, 13, True)[0]
    dp = gpu_points(nat(), ctx, exps)
    wide = ctx.msm_table_build(dp.ptr, n, None, 0, WIDE)
    ds = [ctx.upload(sc_bytes(nat(), _heavy(("ed_wide", v), v, 20, 13, True)[1])) for v in WIDE_VALUES]
    out = ctx.alloc(128 * 3)
    st = stages(ctx, lambda: ctx.msm_table_batch(wide.ptr, n, 0, [d.ptr for d in ds], n, None, out.ptr, None, WIDE))
    assert "msm_bucket" in st and "short_bins" not in st, st
    return ed_ext_canon(get(ctx, out, 128 * 3))


def ed_wide_want():
    # (every vector of the pass has its own exponents' seed; the points are the first vector's)
    exps = _heavy(("ed_wide", WIDE_VALUES[0]), WIDE_VALUES[0], 20, 13, True)[0]
    return b"".join(ed_exp_point(ed_dot(_heavy(("ed_wide", v), v, 20, 13, True)[1], exps)) for v in WIDE_VALUES)


# tests/test_gpu_cabi.py test_table_batch_equals_single_commitments: 700 points, 2 extras, tables of 1, 4 and 16 rows
TB_N, TB_ROWS = 700, (1, 4, 16)


def _tb_inputs():
    def make():
        from oracle import ed25519_ref as ed
        rng, exps = ed_inputs(700, TB_N + 2)
        vecs = [[rng.randrange(ed.ELL) for _ in range(TB_N)],
                [rng.randrange(ed.ELL) if i % 2 else 0 for i in range(TB_N)],      # half-populated (A_i / B_i shape)
                [ed.ELL - 1 - i for i in range(TB_N)]]
        exs = [[rng.randrange(ed.ELL), 0], None, [ed.ELL - 1, ed.ELL - 2]]
        return exps, vecs, exs
    return memo("ed_table_batch", make)


def ed_table_batch_run(ctx):
    from tests.test_gpu_cabi import gpu_points, sc_bytes
    exps, vecs, exs = _tb_inputs()
    dp = gpu_points(nat(), ctx, exps)
    dv = [ctx.upload(sc_bytes(nat(), v)) for v in vecs]
    dx = [ctx.upload(sc_bytes(nat(), e)) if e is not None else None for e in exs]
    out, got = ctx.alloc(128 * 3), b""
    ctx.set_short_path(False)           # 16 rows over <= 2^17 columns would take the fused path (its own case below)
    try:
        for rows in TB_ROWS:
            table = ctx.msm_table_build(dp.ptr, TB_N, dp.ptr + 64 * TB_N, 2, rows)
            st = stages(ctx, lambda: ctx.msm_table_batch(table.ptr, TB_N, 2, [v.ptr for v in dv], TB_N,
                                                         [e.ptr if e is not None else None for e in dx], out.ptr, None,
                                                         rows=rows))
            assert "msm_bucket" in st and "short_bins" not in st, (rows, st)
            got += ed_ext_canon(get(ctx, out, 128 * 3))
    finally:
        ctx.set_short_path(True)
    return got


def ed_table_batch_want():
    exps, vecs, exs = _tb_inputs()
    one = b"".join(ed_exp_point(ed_dot(v, exps) + (ed_dot(e, exps[TB_N:]) if e else 0)) for v, e in zip(vecs, exs))
    return one * len(TB_ROWS)


# tests/test_gpu_short_path.py test_short_path_matches_oracle (1100, 2): one commitment (two workgroups a bin), a pair
SHORT_N = 1100


def _short_inputs():
    def make():
        from oracle import ed25519_ref as ed
        ELL = ed.ELL
        rng, exps = ed_inputs(900 + SHORT_N, SHORT_N + 2)
        x = [[rng.randrange(ELL) for _ in range(SHORT_N)] for _ in range(2)]
        for i, v in enumerate([0, 1, ELL - 1, 2, ELL // 2, ELL // 2 + 1, (1 << 252) + 5, 0x8000, 0x7fff, 0x18000]):
            x[0][i] = v
        gam = [[rng.randrange(ELL) for _ in range(2)] for _ in range(2)]
        return exps, x, gam
    return memo("ed_short", make)


def ed_short_run(ctx):
    from tests.test_gpu_cabi import gpu_points, sc_bytes
    from tests.test_gpu_short_path import ran_short
    exps, x, gam = _short_inputs()
    dp = gpu_points(nat(), ctx, exps)
    table = ctx.msm_table_build(dp.ptr, SHORT_N, dp.ptr + 64 * SHORT_N, 2, 16)
    ds, dg = [ctx.upload(sc_bytes(nat(), v)) for v in x], [ctx.upload(sc_bytes(nat(), v)) for v in gam]
    out = ctx.alloc(256)
    assert ran_short(ctx, lambda: ctx.msm_table(table.ptr, SHORT_N, 2, ds[0].ptr, SHORT_N, dg[0].ptr, out.ptr, None, 16))
    got = ed_ext_canon(get(ctx, out, 128))
    assert ran_short(ctx, lambda: ctx.msm_table_batch(table.ptr, SHORT_N, 2, [d.ptr for d in ds], SHORT_N,
                                                      [d.ptr for d in dg], out.ptr, None, 16))
    return got + ed_ext_canon(get(ctx, out, 256))


def ed_short_want():
    exps, x, gam = _short_inputs()
    w = [ed_exp_point(ed_dot(x[k], exps) + ed_dot(gam[k], exps[SHORT_N:])) for k in range(2)]
    return w[0] + w[0] + w[1]


# tests/test_gpu_cabi.py test_fixed_base_comb_matches_oracle: the digit-recoding edges and 40 random scalars
def _fb_inputs():
    def make():
        from oracle import ed25519_ref as ed
        ELL = ed.ELL
        rng = random.Random(31)
        base = ed.pt_repeat(ed.BASE, rng.randrange(1, ELL))
        sc = [0, 1, 2, 127, 128, 129, 255, 256, 257, 0x8080, 0x7f7f7f7f, (1 << 252) - 1, 1 << 252, ELL - 1, ELL - 2,
              int.from_bytes(bytes([0x80] * 31 + [0x0f]), "little"), int.from_bytes(bytes([0x81] * 31 + [0x0f]), "little"),
              int.from_bytes(bytes([0xff] * 31 + [0x0f]), "little")] + [rng.randrange(ELL) for _ in range(40)]
        return base, sc
    return memo("ed_fixed_base", make)


def ed_fixed_base_run(ctx):
    from tests.test_gpu_cabi import aff_bytes, sc_bytes
    base, sc = _fb_inputs()
    db, ds = ctx.upload(aff_bytes([base])), ctx.upload(sc_bytes(nat(), sc))
    out = ctx.alloc(64 * len(sc))
    ctx.fixed_base(db.ptr, ds.ptr, len(sc), out.ptr)
    return ed_aff_canon(get(ctx, out, 64 * len(sc)))


def ed_fixed_base_want():
    from oracle import ed25519_ref as ed
    base, sc = _fb_inputs()
    return b"".join(ed_aff(ed.pt_affine(ed.pt_repeat(base, v))) for v in sc)


# tests/test_gpu_cabi.py test_normalize_and_lift: off-curve and non-canonical encodings are counted; 300 points here
# (more than one workgroup), three of them bad, then the clean vector
VAL_N, VAL_BAD = 300, (0, 151, 299)


def ed_validate_run(ctx):
    import numpy as np
    from oracle import ed25519_ref as ed
    from tests.test_gpu_cabi import gpu_points
    _, exps = ed_inputs(391, VAL_N)
    dp = gpu_points(nat(), ctx, exps)
    clean = ctx.download(dp.ptr, 64 * VAL_N).reshape(VAL_N, 64)
    bad = clean.copy()
    bad[VAL_BAD[0], 0] ^= 1                                                                  # off the curve
    bad[VAL_BAD[1], 32:64] = np.frombuffer((ed.P + 1).to_bytes(32, "little"), dtype=np.uint8)  # y = p + 1: not canonical
    bad[VAL_BAD[2], 33] ^= 4
    counts = [ctx.validate_points(ctx.upload(bad).ptr, VAL_N), ctx.validate_points(dp.ptr, VAL_N)]
    return b"".join(int(c).to_bytes(8, "little") for c in counts)


def ed_validate_want():
    return (3).to_bytes(8, "little") + (0).to_bytes(8, "little")


# ---- exact.hip: tests/test_gpu_cabi.py test_tree_reduce_order, n = 65 (an odd level in the tree) ----------------------
def _tr_points():
    def make():
        from oracle import ac20_ref as ac
        from oracle import ed25519_ref as ed
        rng = random.Random(13 + 65)
        return ac.create_generators([rng.randrange(1, ed.ELL) for _ in range(65)])["g"]
    return memo("ed_tree_reduce", make)


def ed_tree_reduce_run(ctx):
    from tests.test_gpu_cabi import proj_bytes
    pts, got = _tr_points(), b""
    for append in (True, False):
        d, out = ctx.upload(proj_bytes(pts)), ctx.alloc(96)
        ctx.tree_reduce(d.ptr, len(pts), append, out.ptr)
        got += get(ctx, out, 96)            # the projective representative IS the contract (pivot.list_mul's tree)
    return got


def ed_tree_reduce_want():
    from oracle import ed25519_ref as ed
    pts = _tr_points()
    return b"".join(ed.proj_to_bytes(ed.tree_reduce(ed.pt_add, pts, ed.IDENTITY if append else None))
                    for append in (True, False))


# ---- fold_jump.hip: tests/test_gpu_cabi.py test_table_fold_equals_k_reference_folds (4, 300, 5, 2) and (16, 31, 1, 5) --
FOLD_SHAPES = ((4, 300, 5, 2), (16, 31, 1, 5))


def _fold_inputs(shape):
    def make():
        from oracle import ac20_ref as ac
        from oracle import ed25519_ref as ed
        from tests.test_gpu_cabi import make_points
        rows, n_main, n_extra, k = shape
        rng = random.Random(rows * 1000 + n_main)
        _, pts = make_points(rng, n_main + n_extra)
        n_cols = 1 << ((n_main + n_extra).bit_length() - 1)
        cs = [rng.randrange(ed.ELL) for _ in range(k)]
        g = list(pts[:n_cols])
        for c in cs:
            half = len(g) // 2
            g = ac.fold_generators(g[:half], g[half:], c)
        s = []
        for b in range(1 << k):             # s_b = prod over rounds i (first round = top bit of b) of c_i where that bit is 0
            v = 1
            for i, c in enumerate(cs):
                if not (b >> (k - 1 - i)) & 1:
                    v = v * c % ed.ELL
            s.append(v)
        return pts, n_cols, s, b"".join(ed_aff(ed.pt_affine(p)) for p in g)
    return memo(("ed_table_fold", shape), make)


def ed_table_fold_run(ctx):
    from tests.test_gpu_cabi import aff_bytes
    got = b""
    for shape in FOLD_SHAPES:
        rows, n_main, n_extra, k = shape
        pts, n_cols, s, _ = _fold_inputs(shape)
        dp, de = ctx.upload(aff_bytes(pts[:n_main])), ctx.upload(aff_bytes(pts[n_main:]))
        table = ctx.msm_table_build(dp.ptr, n_main, de.ptr, n_extra, rows)
        out = ctx.alloc(64 * (n_cols >> k))
        ctx.msm_table_fold(table.ptr, n_main, n_extra, rows, n_cols, s, out.ptr)
        got += ed_aff_canon(get(ctx, out, 64 * (n_cols >> k)))
    return got


def ed_table_fold_want():
    return b"".join(_fold_inputs(shape)[3] for shape in FOLD_SHAPES)


# ---- format.hip: tests/test_gpu_cabi.py test_transcript_text ----------------------------------------------------------
def _fmt_inputs():
    def make():
        from oracle import ac20_ref as ac
        from oracle import ed25519_ref as ed
        rng = random.Random(16)
        pts = ac.create_generators([rng.randrange(1, ed.ELL) for _ in range(60)])["g"]
        pts += [ed.IDENTITY, ed.BASE, (0, 5, 7), (10**76, 1, 10**9)]
        sc = [rng.randrange(ed.ELL) for _ in range(2500)] + [0, 1, ed.ELL - 1, ed.ELL // 2, ed.ELL // 2 + 1, 10**9, 10**9 - 1]
        text = "".join(ed.pt_repr(p) + ", " for p in pts) + "".join(ed.scalar_repr(v) + ", " for v in sc) + \
            "".join(str(v) + ", " for v in sc)
        return pts, sc, text.encode()
    return memo("format", make)


def format_run(ctx):
    from tests.test_gpu_cabi import proj_bytes, sc_bytes
    pts, sc, _ = _fmt_inputs()
    d = ctx.upload(sc_bytes(nat(), sc))
    return ctx.format_points(ctx.upload(proj_bytes(pts)).ptr, len(pts)).tobytes() + \
        ctx.format_scalars(d.ptr, len(sc), True).tobytes() + ctx.format_scalars(d.ptr, len(sc), False).tobytes()


def format_async_run(ctx):
    """the same text through the asynchronous entries (Context.format_begin), whole and delivered in pieces"""
    from tests.test_gpu_cabi import proj_bytes, sc_bytes
    pts, sc, _ = _fmt_inputs()
    dp, ds = ctx.upload(proj_bytes(pts)), ctx.upload(sc_bytes(nat(), sc))
    got = bytes(ctx.format_begin("points", dp.ptr, len(pts)).result())
    got += bytes(ctx.format_begin("scalars", ds.ptr, len(sc), True).result())
    return got + bytes(ctx.format_begin("scalars", ds.ptr, len(sc), False, own_signal=True).result())


def format_want():
    return _fmt_inputs()[2]


# ---- frvec.hip: tests/test_gpu_frvec.py test_dot_and_dot_to_dev, n = 65537 (the first length with a second block) ------
DOT_N = 65537


def _dot_inputs():
    def make():
        from oracle import ed25519_ref as ed
        a, b = rand32(65, DOT_N), rand32(66, DOT_N)
        a[:, 31] &= 0x0f
        b[:, 31] &= 0x0f
        ai, bi = ints_of(a), ints_of(b)
        ai[0] = bi[0] = ai[-1] = bi[-1] = ed.ELL - 1
        return arr32(ai), arr32(bi), le32([ed_dot(ai, bi) % ed.ELL])
    return memo("fr_dot", make)


def fr_dot_run(ctx):
    a, b, _ = _dot_inputs()
    da, db = ctx.upload(a), ctx.upload(b)
    return le32([ctx.fr_dot(da.ptr, db.ptr, DOT_N)])


def fr_dot_to_dev_run(ctx):
    a, b, _ = _dot_inputs()
    da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(32)
    ctx.fr_dot_into(da.ptr, db.ptr, DOT_N, out.ptr)
    return get(ctx, out, 32)


def fr_dot_want():
    return _dot_inputs()[2]


# ---- nullity.hip ------------------------------------------------------------------------------------------------------
# tests/test_gpu_nullity.py test_combine_tall_shapes_take_the_segmented_path: n = 5, s = 100 rows (segments of rows,
# partial sums in the arena); test_rows_dot_matches_the_restatement: 17 rows of (n, stride) = (4097, 4097)
def _rows_inputs(s, n):
    def make():
        from tests.test_gpu_nullity import raw_matrix
        return raw_matrix(random.Random(1718 + s), s, n)
    return memo(("rows", s, n), make)


def _rho():
    from oracle import ed25519_ref as ed
    return random.Random(100).randrange(2, ed.ELL - 1)


def fr_rows_combine_run(ctx):
    rows, arr = _rows_inputs(100, 5)
    buf, out = ctx.upload(arr), ctx.alloc(32 * 5)
    st = stages(ctx, lambda: ctx.fr_rows_combine(buf.ptr, 100, 5, 5, _rho(), out.ptr))
    assert "nl_combine_seg" in st, st
    return get(ctx, out, 32 * 5)


def fr_rows_combine_want():
    from tests import nullity_ref as nr
    return le32(nr.combine(_rows_inputs(100, 5)[0], _rho()))


def _rows_x(n):
    from oracle import ed25519_ref as ed
    rng = random.Random(n + 1)
    x = [rng.randrange(ed.ELL) for _ in range(n)]
    x[0], x[n - 1] = ed.ELL - 1, ed.ELL - 1
    return x


def fr_rows_dot_run(ctx):
    rows, arr = _rows_inputs(17, 4097)
    buf, xs, out = ctx.upload(arr), ctx.upload(arr32(_rows_x(4097))), ctx.alloc(32 * 17)
    first = ctx.fr_rows_dot(buf.ptr, 17, 4097, 4097, xs.ptr, out.ptr)
    return get(ctx, out, 32 * 17) + int(-1 if first is None else first).to_bytes(4, "little", signed=True)


def fr_rows_dot_want():
    from tests import nullity_ref as nr
    vals = nr.values(_rows_inputs(17, 4097)[0], _rows_x(4097))
    first = next((i for i, v in enumerate(vals) if v), -1)
    return le32(vals) + first.to_bytes(4, "little", signed=True)


# ---- batch_verify.hip: tests/test_gpu_batch_products.py test_matches_reference (3, 7, 1) --------------------------------
def _bp_case():
    def make():
        from tests.test_gpu_batch_products import Case
        return Case(3, 7, 1, 1000 * 3 + 10 * 7 + 1)
    return memo("batch_products", make)


def fr_batch_products_run(ctx):
    u, dots = _bp_case().run(ctx)
    return u.tobytes() + dots.tobytes()


def fr_batch_products_want():
    from tests import batch_verify_ref as ref
    c = _bp_case()
    u, dots = ref.batch_products(c.cs, c.lb, c.zs, c.ws, c.forms, c.n)
    return le32(u) + le32(dots)


# ---- circuit_sat.hip, fr_colsum.h ---------------------------------------------------------------------------------------
# tests/test_gpu_p8_primitives.py: test_factorial_tables K = 8193 (the first K past a scan block of 8192),
# test_lagrange_vector (8193, table 2 * 8193 + 1), test_extension m = 258 (a second correlation segment)
CS_K = 8193


def cs_tables_run(ctx):
    fact, ifact = ctx.alloc(32 * (CS_K + 1)), ctx.alloc(32 * (CS_K + 1))
    ctx.cs_tables(CS_K, fact.ptr, ifact.ptr)
    return get(ctx, fact, 32 * (CS_K + 1)) + get(ctx, ifact, 32 * (CS_K + 1))


def cs_tables_want():
    from tests import p8_ref as ref
    f, i = memo(("p8_tables", CS_K), lambda: ref.tables(CS_K))
    return le32(f) + le32(i)


def _lag_c():
    from tests import p8_ref as ref
    return random.Random(7000 + CS_K).randrange(ref.ELL)


def cs_lagrange_run(ctx):
    from tests import p8_ref as ref
    table_k = 2 * CS_K + 1
    ifact = ctx.upload(arr32(memo(("p8_tables", table_k), lambda: ref.tables(table_k))[1]))     # from the host
    out, got = ctx.alloc(32 * (CS_K + 1)), b""
    for c in (_lag_c(), CS_K // 2):             # off the nodes, and on one
        ctx.cs_lagrange(c, CS_K, ifact.ptr, out.ptr)
        got += get(ctx, out, 32 * (CS_K + 1))
    return got


def cs_lagrange_want():
    from tests import p8_ref as ref
    return le32(ref.lagrange_bary(CS_K, _lag_c())) + le32([int(j == CS_K // 2) for j in range(CS_K + 1)])


EXT_M = 258


def _ext_inputs():
    def make():
        from tests import p8_ref as ref
        rng = random.Random(9000 + EXT_M)
        a, b = ([rng.randrange(ref.ELL) for _ in range(EXT_M + 1)] for _ in range(2))
        want = ref.z_tail_bary(a[:EXT_M], b[:EXT_M], a[EXT_M], b[EXT_M])
        for p in range(3, 3 + EXT_M):           # the gammas' places are not the entry's to write: zero going in
            want[p] = 0
        return a, b, le32(want)
    return memo("cs_extend", make)


def cs_extend_run(ctx):
    import numpy as np
    from tests import p8_ref as ref
    a, b, _ = _ext_inputs()
    K = 2 * EXT_M + 1
    fact, ifact = (ctx.upload(arr32(t)) for t in memo(("p8_tables", K), lambda: ref.tables(K)))
    da, db = ctx.upload(arr32(a)), ctx.upload(arr32(b))
    z = ctx.upload(np.zeros((2 * EXT_M + 3, 32), np.uint8))
    ctx.cs_extend(da.ptr, db.ptr, EXT_M, fact.ptr, ifact.ptr, z.ptr)
    return get(ctx, z, 32 * (2 * EXT_M + 3))


def cs_extend_want():
    return _ext_inputs()[2]


# tests/test_gpu_colsum.py test_one_plan_through_both_fields: one plan with more than 256 partial sums, both fields
def _colsum_inputs():
    def make():
        import numpy as np
        from oracle import bn256_ref as bn
        from oracle import ed25519_ref as ed
        from tests import test_gpu_colsum as T
        from verifiable_mpc_amd import sparse
        rng = np.random.default_rng(5)
        col_ptr = np.concatenate([[0], np.cumsum(T.LENS)])
        rows = rng.integers(0, T.N_ROWS + 40, size=col_ptr[-1])
        rows[col_ptr[T.WORST]:col_ptr[T.WORST + 1]] = np.arange(64)
        items, longs, n_partial = sparse.colsum_plan(col_ptr, T.DST)
        assert n_partial > 256
        items = np.vstack([items, np.array([[5, 5, T.EMPTY_AT]], np.uint32)])
        fields = {}
        for entry, order in (("bn256_qap_colsum", bn.N), ("cs_colsum", ed.ELL)):
            prng = random.Random(order)
            vals = [prng.randrange(order) for _ in range(len(rows))]
            weights = [prng.randrange(order) for _ in range(T.N_ROWS)]
            vals[col_ptr[T.WORST]:col_ptr[T.WORST + 1]] = [order - 1] * 64
            weights[:64] = [order - 1] * 64
            want = [0] * T.N_OUT                # (the buffer is zero going in: positions no item writes stay zero)
            for c, d in enumerate(T.DST):
                if T.LENS[c]:
                    want[d] = sum(vals[e] * weights[rows[e]] for e in range(col_ptr[c], col_ptr[c + 1])
                                  if rows[e] < T.N_ROWS) % order
            fields[entry] = (arr32(vals), arr32(weights), le32(want))
        return rows.astype(np.uint32), items, longs, n_partial, fields
    return memo("colsum", make)


def colsum_run(ctx):
    import numpy as np
    from tests import test_gpu_colsum as T
    rows, items, longs, n_partial, fields = _colsum_inputs()
    d_rows, d_items, d_longs = ctx.upload(rows), ctx.upload(items), ctx.upload(longs)
    got = b""
    for entry, (vals, weights, _) in fields.items():
        d_vals, d_w, out = ctx.upload(vals), ctx.upload(weights), ctx.upload(np.zeros((T.N_OUT, 32), np.uint8))
        getattr(ctx, entry)(d_w.ptr, T.N_ROWS, d_rows.ptr, d_vals.ptr, len(rows), d_items.ptr, len(items), d_longs.ptr,
                            len(longs), n_partial, out.ptr, T.N_OUT)
        got += get(ctx, out, 32 * T.N_OUT)
    return got


def colsum_want():
    return b"".join(f[2] for f in _colsum_inputs()[4].values())


# ---- bn256.hip ----------------------------------------------------------------------------------------------------------
def bn_groups(grp):
    from tests.test_gpu_bn256_edges import GROUPS
    return GROUPS[grp]


def bn_jac_canon(grp, raw):
    """Jacobian outputs -> affine bytes (tests/test_gpu_bn256_edges.py assert_jac: Z = 0 exactly at infinity)"""
    from verifiable_mpc_amd import pynocchio as pn
    jw = 3 * bn_groups(grp)[4] // 2
    return b"".join(pn._from_jacobian(grp, raw[o:o + jw]).to_bytes() for o in range(0, len(raw), jw))


# tests/test_gpu_bucket_runs.py test_bn256_heavy_bucket_full_segment_plus_remainder: G1, n = 300 (c = 6), 70 entries in
# one bucket of window 0; and 60 points of the twist with uniform scalars (the other instantiation of bn_msm_dev)
def _bn_msm_inputs():
    def make():
        from oracle import bn256_ref as bn
        from tests import bn256_msm_inputs as mi
        from tests.test_gpu_bn256 import walk_points
        from tests.test_gpu_bucket_runs import heavy_vector
        from tests.test_gpu_bn256_edges import dot, host_points
        rng = random.Random(7006)
        c, W = mi.make_plan(300)
        assert c == 6
        e1, p1 = walk_points(bn.E1, bn.G1, rng, 300)
        x1 = heavy_vector(rng, 70, 9, c, W, False, order=bn.N, n_random=230)
        e2, p2 = walk_points(bn.E2, bn.G2, rng, 60)
        x2 = [rng.randrange(bn.N) for _ in range(60)]
        x2[:3] = [0, 1, bn.N - 1]
        want = bn.g1_to_bytes(bn.E1.mul(dot(x1, e1), bn.G1)) + bn.g2_to_bytes(bn.E2.mul(dot(x2, e2), bn.G2))
        return (host_points(1, p1), arr32(x1), 300), (host_points(2, p2), arr32(x2), 60), want
    return memo("bn_msm", make)


def bn_msm_run(ctx):
    got = b""
    for grp, (pts, sc, n) in zip((1, 2), _bn_msm_inputs()[:2]):
        width = bn_groups(grp)[4]
        dp, ds, out = ctx.upload(pts), ctx.upload(sc), ctx.alloc(width)
        ctx.bn256_msm(grp, ds.ptr, dp.ptr, n, out.ptr)
        got += get(ctx, out, width)
    return got


def bn_msm_want():
    return _bn_msm_inputs()[2]


# tests/test_gpu_bn256_edges.py test_table_extreme_buckets, G1, tn = 297 (padding columns in the stride), the "mixed"
# vector, whole and a prefix; the single-key pass (affine and Jacobian out) and the multi-key pass over two tables
BN_TN = 297


def _bn_table_inputs():
    def make():
        from oracle import bn256_ref as bn
        from tests import bn256_msm_inputs as mi
        from tests.test_gpu_bn256 import walk_points
        from tests.test_gpu_bn256_edges import dot, host_points
        rng = random.Random(BN_TN * 3 + 1)
        keys = [walk_points(bn.E1, bn.G1, rng, BN_TN) for _ in range(2)]
        mixed = [mi.extreme(16), bn.N - 1, 0, 1, (1 << 15) - 1, 1 << 15, (1 << 15) + 1] * 8
        mixed += [rng.randrange(bn.N) for _ in range(BN_TN - len(mixed))]
        want = {m: [bn.g1_to_bytes(bn.E1.mul(dot(mixed[:m], exps[:m]), bn.G1)) for exps, _ in keys]
                for m in (BN_TN, BN_TN - 5)}
        return [host_points(1, pts) for _, pts in keys], arr32(mixed), want
    return memo("bn_table", make)


def bn_table_msm_run(ctx):
    from tests.test_gpu_bn256_edges import table_msm
    pts, sc, _ = _bn_table_inputs()
    table = ctx.bn256_table_build(1, ctx.upload(pts[0]).ptr, BN_TN)
    ds, got = ctx.upload(sc), b""
    for m in (BN_TN, BN_TN - 5):
        aff, jac = table_msm(ctx, 1, table, BN_TN, ds, m)
        got += aff + bn_jac_canon(1, jac)
    return got


def bn_table_msm_want():
    want = _bn_table_inputs()[2]
    return b"".join(want[m][0] * 2 for m in (BN_TN, BN_TN - 5))


def bn_table_msm_multi_run(ctx):
    from tests.test_gpu_bn256_edges import multi_msm
    pts, sc, _ = _bn_table_inputs()
    tables = [ctx.bn256_table_build(1, ctx.upload(p).ptr, BN_TN) for p in pts]
    ds = ctx.upload(sc)
    return b"".join(bn_jac_canon(1, raw) for m in (BN_TN, BN_TN - 5) for raw in multi_msm(ctx, 1, tables, BN_TN, ds, m))


def bn_table_msm_multi_want():
    want = _bn_table_inputs()[2]
    return b"".join(b"".join(want[m]) for m in (BN_TN, BN_TN - 5))


# tests/test_gpu_bn256.py test_full_size_exponent_identity validates its device-made points (count 0); here 300 host
# points of each group with three spoilt, then the clean vector
def bn_validate_run(ctx):
    import numpy as np
    from oracle import bn256_ref as bn
    got = b""
    for grp, (pts, _, n) in zip((1, 2), _bn_msm_inputs()[:2]):
        bad = np.array(pts, copy=True)
        for i in (0, n // 2, n - 1):
            bad[i, 40] ^= 1                     # a bit of y: off the curve
        bad[1, 32:64] = np.frombuffer((bn.P + 2).to_bytes(32, "little"), np.uint8)      # y >= p: not canonical
        for arr in (bad, pts):
            got += int(ctx.bn256_validate(grp, ctx.upload(arr).ptr, n)).to_bytes(8, "little")
    return got


def bn_validate_want():
    return b"".join(int(c).to_bytes(8, "little") for c in (4, 0, 4, 0))


# ---- bn256_keygen.hip: tests/test_gpu_pinocchio_keygen.py test_special_s_sparse_and_dense, d = 1000 ---------------------
LAG_D = 1000


def _lag_s():
    from tests import keygen_ref as K
    return [random.Random(6000 + LAG_D).randrange(LAG_D + 1, K.N), 517]


def bn_qap_lagrange_run(ctx):
    from tests import keygen_ref as K
    ell, t, got = ctx.alloc(32 * LAG_D), ctx.alloc(32), b""
    for s in _lag_s():
        sb = ctx.upload(K.to_array([s]))
        ctx.bn256_qap_lagrange(sb.ptr, LAG_D, ell.ptr, t.ptr)
        got += get(ctx, ell, 32 * LAG_D) + get(ctx, t, 32)
    return got


def bn_qap_lagrange_want():
    from tests import keygen_ref as K
    out = b""
    for s in _lag_s():
        ell, t = K.lagrange_at(s, LAG_D)
        out += le32(ell) + le32([t])
    return out


# ---- polynomial products ------------------------------------------------------------------------------------------------
def _product(a, b):
    from tests.test_gpu_poly_mul_ntt import product
    return le32(product(ints_of(a), ints_of(b)))


# tests/test_gpu_pinocchio_batch_primitives.py test_product_batch_windows n = 513: tiles cut into three segments, the
# partial sums through the arena (any 32-byte values, reduced on load)
def _koe_inputs():
    return memo("koe", lambda: (lambda a, b: (a, b, _product(a, b)))(rand32(513, 513), rand32(514, 513)))


def koe_poly_mul_run(ctx):
    a, b, _ = _koe_inputs()
    assert ctx.get_poly_product() == 0          # a new context's: the schoolbook product
    da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(32 * 1025)
    ctx.bn256_fr_poly_mul(da.ptr, 513, db.ptr, 513, out.ptr)
    return get(ctx, out, 32 * 1025)


def koe_poly_mul_want():
    return _koe_inputs()[2]


# tests/test_gpu_poly_mul_ntt.py test_one_workgroup_two_pass_boundary (na + nb - 1 = BN256_FR_NTT_LDS_LEN: one workgroup
# in LDS; one more: a column pass) and test_every_pass_plan_against_schoolbook (131073, 5): two column passes
NTT_SHAPES = ((2046, 3), (2047, 3), (131073, 5))


def _ntt_inputs(shape):
    def make():
        a, b = rand32(shape[0], shape[0]), rand32(shape[1] + 1, shape[1])
        return a, b, _product(a, b)
    return memo(("ntt", shape), make)


def ntt_poly_mul_run(ctx):
    assert nat().BN256_FR_NTT_LDS_LEN == NTT_SHAPES[0][0] + NTT_SHAPES[0][1] - 1
    got = b""
    for na, nb in NTT_SHAPES:
        a, b, _ = _ntt_inputs((na, nb))
        da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(32 * (na + nb - 1))
        ctx.bn256_fr_poly_mul_ntt(da.ptr, na, db.ptr, nb, out.ptr)
        got += get(ctx, out, 32 * (na + nb - 1))
    return got


def ntt_poly_mul_want():
    return b"".join(_ntt_inputs(s)[2] for s in NTT_SHAPES)


# ---- bn256_qap_mtree.hip: tests/test_gpu_moments_tree.py SHAPES, d = n_out = 4 S + 1 = 513 (three levels over the
# leaves, a padded last leaf) --------------------------------------------------------------------------------------------
MT_D = 513


def _mt_inputs():
    def make():
        from tests import keygen_ref as K
        from tests import moments_tree_ref as R
        u0 = rand32(MT_D + MT_D, MT_D)
        u1 = K.to_array([R.N - 1] * MT_D)
        want = b"".join(K.to_array(R.moments(ints_of(u), MT_D)).tobytes() for u in (u0, u1))
        return u0, u1, want
    return memo("mtree", make)


def _mt_moments(ctx, plan):
    u0, u1, _ = _mt_inputs()
    d0, d1, o0, o1 = ctx.upload(u0), ctx.upload(u1), ctx.alloc(32 * MT_D), ctx.alloc(32 * MT_D)
    scratch = ctx.alloc(nat().bn256_qap_moments_tree_scratch_bytes(MT_D, 1))
    ctx.bn256_qap_moments_tree_batch(plan.ptr, MT_D, MT_D, d0.ptr, d1.ptr, MT_D, MT_D, o0.ptr, o1.ptr, MT_D, scratch.ptr, 1)
    return get(ctx, o0, 32 * MT_D) + get(ctx, o1, 32 * MT_D)


def mtree_build_run(ctx):
    """the plan built over this arena state, judged by the moments it gives"""
    plan = ctx.alloc(nat().bn256_qap_mtree_bytes(MT_D, MT_D))
    ctx.bn256_qap_mtree_build(MT_D, MT_D, plan.ptr)
    ctx.sync()
    return _mt_moments(ctx, plan)


def mtree_moments_run(ctx):
    """the plan is built on the context's first run and kept: every later run is the moments alone over its arena state"""
    plan = getattr(ctx, "_arena_case_mtree_plan", None)
    if plan is None:
        plan = ctx.alloc(nat().bn256_qap_mtree_bytes(MT_D, MT_D))
        ctx.bn256_qap_mtree_build(MT_D, MT_D, plan.ptr)
        ctx.sync()
        ctx._arena_case_mtree_plan = plan
    return _mt_moments(ctx, plan)


def mtree_want():
    return _mt_inputs()[2]


# ---- bn256_pairing.hip: tests/test_gpu_bn256_pairing.py test_pairing_batches (13 pairs: a partial wave; 65: a second
# one), e(k G1, G2) = e(G1, G2)^k, one point at infinity in the middle ----------------------------------------------------
PAIR_NS = (13, 65)


def _pair_inputs(n):
    def make():
        import numpy as np
        from oracle import bn256_ref as bn
        from tests import bn256_pairing_ref as R
        rng = random.Random(n)
        k0, inf_j = rng.randrange(1, bn.N), n // 2
        e = memo("pairing_e", lambda: R.pairing(bn.G1, bn.G2))
        p, g1, gts, cur = bn.E1.mul(k0, bn.G1), [], [], R.gt_pow(e, k0)
        for j in range(n):
            g1.append(bn.g1_to_bytes(p if j != inf_j else None))
            gts.append(cur if j != inf_j else R.GT_ONE)
            p, cur = bn.E1.add(p, bn.G1), R.gt_mul(cur, e)
        g1 = np.frombuffer(b"".join(g1), np.uint8).reshape(n, 64)
        g2 = np.tile(np.frombuffer(bn.g2_to_bytes(bn.G2), np.uint8), (n, 1))
        return g1, g2, gts
    return memo(("pairing", n), make)


def bn_pairing_run(ctx):
    got = b""
    for n in PAIR_NS:
        g1, g2, _ = _pair_inputs(n)
        d1, d2, out = ctx.upload(g1), ctx.upload(g2), ctx.alloc(384 * n)
        ctx.bn256_pairing(d1.ptr, d2.ptr, n, out.ptr)
        got += get(ctx, out, 384 * n)
    return got


def bn_pairing_want():
    return b"".join(le32(gt) for n in PAIR_NS for gt in _pair_inputs(n)[2])


def _pair_offsets(n):
    """products of 0 .. 12 pairs and the rest (tests/test_gpu_bn256_pairing.py test_pairing_product_lengths_and_offsets)"""
    cuts = [0, 1, 1, 4, 6] + ([13] if n == 13 else [18, 33, 65])
    return cuts


def bn_pairing_product_run(ctx):
    import numpy as np
    got = b""
    for n in PAIR_NS:
        g1, g2, _ = _pair_inputs(n)
        off = np.array(_pair_offsets(n), np.uint32)
        k = len(off) - 1
        d1, d2, doff = ctx.upload(g1), ctx.upload(g2), ctx.upload(off)
        ones, gt = ctx.alloc(k), ctx.alloc(384 * k)
        ctx.bn256_pairing_product(d1.ptr, d2.ptr, n, doff.ptr, k, ones.ptr, gt.ptr)
        got += get(ctx, ones, k) + get(ctx, gt, 384 * k)
    return got


def bn_pairing_product_want():
    from tests import bn256_pairing_ref as R
    out = b""
    for n in PAIR_NS:
        gts, off = _pair_inputs(n)[2], _pair_offsets(n)
        prods = []
        for lo, hi in zip(off[:-1], off[1:]):
            w = R.GT_ONE
            for j in range(lo, hi):
                w = R.gt_mul(w, gts[j])
            prods.append(w)
        out += bytes(int(p == R.GT_ONE) for p in prods) + b"".join(le32(p) for p in prods)
    return out


# ---- bn256_qap_h.hip ----------------------------------------------------------------------------------------------------
# tests/test_gpu_pinocchio_h.py test_moments_primitive (4097, 8): five ranges of j, summed through the arena
MOM_D, MOM_OUT = 4097, 8


def _mom_inputs():
    def make():
        from tests import keygen_ref as K
        from tests.test_gpu_pinocchio_h import _moments_ref
        rnd, top = rand32(MOM_D, MOM_D), K.to_array([K.N - 1] * MOM_D)
        want = le32(_moments_ref([x % K.N for x in ints_of(rnd)], MOM_OUT)) + le32(_moments_ref([K.N - 1] * MOM_D, MOM_OUT))
        return rnd, top, want
    return memo("qh_moments", make)


def qh_moments_run(ctx):
    rnd, top, _ = _mom_inputs()
    du, dt, o0, o1 = ctx.upload(rnd), ctx.upload(top), ctx.alloc(32 * MOM_OUT), ctx.alloc(32 * MOM_OUT)
    ctx.bn256_qap_moments(du.ptr, dt.ptr, MOM_D, MOM_OUT, o0.ptr, o1.ptr)
    return get(ctx, o0, 32 * MOM_OUT) + get(ctx, o1, 32 * MOM_OUT)


def qh_moments_want():
    return _mom_inputs()[2]


# tests/test_gpu_pinocchio_h.py test_weights_at_scan_boundaries d = 16385: 257 scan lanes, two to a thread
WEI_D = 16385


def _wei_inputs():
    def make():
        from tests import keygen_ref as K
        from tests.test_gpu_pinocchio_h import _weights
        rng = random.Random(8000 + WEI_D)
        a, b = [rng.randrange(K.N) for _ in range(WEI_D)], [K.N - 1] * WEI_D
        inv_w = K.batch_inverse(_weights(WEI_D))
        want = le32([x * f % K.N for x, f in zip(a, inv_w)]) + le32([x * f % K.N for x, f in zip(b, inv_w)])
        return K.to_array(a), K.to_array(b), want
    return memo("qh_weights", make)


def qh_weights_run(ctx):
    a, b, _ = _wei_inputs()
    da, db, ua, ub = ctx.upload(a), ctx.upload(b), ctx.alloc(32 * WEI_D), ctx.alloc(32 * WEI_D)
    ctx.bn256_qap_h_weights(da.ptr, db.ptr, WEI_D, ua.ptr, ub.ptr)
    return get(ctx, ua, 32 * WEI_D) + get(ctx, ub, 32 * WEI_D)


def qh_weights_want():
    return _wei_inputs()[2]


# tests/test_gpu_qap_residual_batch.py test_batch_against_the_reference_and_the_single_entry, d = 1025
RES_D = 1025


def _res_inputs():
    def make():
        from tests import keygen_ref as K
        rng = random.Random(RES_D)
        a, b, y = ([rng.randrange(K.N) for _ in range(RES_D)] for _ in range(3))
        a[0] = b[0] = a[-1] = b[-1] = K.N - 1
        rho, acc, p = rng.randrange(2, K.N), 0, 1
        for i in range(RES_D):
            acc = (acc + p * (a[i] * b[i] - y[i])) % K.N
            p = p * rho % K.N
        return K.to_array(a), K.to_array(b), K.to_array(y), rho, le32([acc])
    return memo("qh_residual", make)


def qh_residual_run(ctx):
    a, b, y, rho, _ = _res_inputs()
    da, db, dy, out = ctx.upload(a), ctx.upload(b), ctx.upload(y), ctx.alloc(32)
    ctx.bn256_qap_residual(da.ptr, db.ptr, dy.ptr, RES_D, rho, out.ptr)
    return get(ctx, out, 32)


def qh_residual_want():
    return _res_inputs()[4]


# tests/test_gpu_pinocchio_batch_primitives.py test_combine_batch d = 513 with the deltas: the two d x d products' tiles
# are cut into segments whose partial sums go through the arena.  Oracle: tests/h_ref.py moment_h's last two lines on
# the moments A_k, B_k (k = 1 .. d) the case feeds in
COMB_D = 513


def _comb_inputs():
    def make():
        from tests import h_ref as H
        from tests import keygen_ref as K
        N, d = K.N, COMB_D
        rng = random.Random(2 * d + 1)
        A = [0] + [rng.randrange(N) for _ in range(d)]
        B = [0] + [rng.randrange(N) for _ in range(d)]
        A[1] = B[d] = N - 1
        dv, dw, dy = (rng.randrange(N) for _ in range(3))
        t = H.t_coeffs(d)
        C = [(sum(A[i] * B[k - i] for i in range(1, k)) + dv * B[k] + dw * A[k]) % N for k in range(d + 1)]
        h = [(sum(t[i] * C[i - e] for i in range(e + 1, d + 1)) + dv * dw * t[e] - (dy if e == 0 else 0)) % N
             for e in range(d + 1)]
        return K.to_array(A[1:]), K.to_array(B[1:]), K.to_array([dv, dw, dy]), le32(h)
    return memo("qh_combine", make)


def qh_combine_run(ctx):
    A, B, deltas, _ = _comb_inputs()
    d = COMB_D
    t, t_scratch = ctx.alloc(32 * (d + 1)), ctx.alloc(64 * (d + (d + 127) // 128))
    ctx.bn256_qap_t_coeffs(d, t_scratch.ptr, t.ptr)
    dA, dB, dd = ctx.upload(A), ctx.upload(B), ctx.upload(deltas)
    scratch, out = ctx.alloc(32 * 5 * d), ctx.alloc(32 * (d + 1))
    ctx.bn256_qap_h_combine(dA.ptr, dB.ptr, t.ptr, d, dd.ptr, scratch.ptr, out.ptr)
    return get(ctx, out, 32 * (d + 1))


def qh_combine_want():
    return _comb_inputs()[3]


# ---- prover.hip: a whole compact Protocol-5 proof over a 16-column table (the rounds' pairs by k_p4_direct, whose block
# sums go through the arena; the round context's own pool is kept between proofs), judged by the verifier.
# Shape: tests/test_gpu_batch_verify.py's statements (n = 15, transcript "compact") -------------------------------------
def prover_run(ctx):
    import verifiable_mpc_amd as vm
    from oracle import ed25519_ref as ed
    cp = vm.compressed_pivot
    n, rng = 15, random.Random(88)
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    h = group.generator
    g = vm.PointVector.fixed_base(h, [rng.randrange(1, ed.ELL) for _ in range(n)], ctx, keep_proj=False)
    k = vm.Ed25519Point.repeat(h, rng.randrange(1, ed.ELL))
    g.precompute([h, k])
    gens = {"g": g, "h": h, "k": k}
    x = vm.ScalarVector.from_ints([rng.randrange(ed.ELL) for _ in range(n)], ctx)
    L = vm.pivot.LinearForm(vm.ScalarVector.from_ints([rng.randrange(ed.ELL) for _ in range(n)], ctx))
    gamma = rng.randrange(1, ed.ELL)
    r, rho = [rng.randrange(ed.ELL) for _ in range(n)], rng.randrange(ed.ELL)
    P = vm.pivot.vector_commitment(x, gamma, g, h)
    y = gf(L(x))
    made = []
    st = stages(ctx, lambda: made.append(cp.protocol_5_prover(gens, P, L, y, x, gamma, gf, r=r, rho=rho,
                                                             transcript="compact")))
    assert "p4_direct" in st, st                # the round context ran the rounds on THIS context
    proof = made[0]
    assert cp.protocol_5_verifier(gens, P, L, y, proof, gf, transcript="compact") is True
    out = b""
    for key in sorted(proof):
        v = proof[key]
        if isinstance(v, (list, tuple)):
            out += le32([int(e) % ed.ELL for e in v])
        elif hasattr(v, "to_affine_bytes"):
            out += v.to_affine_bytes()
        else:
            out += le32([int(v) % ed.ELL])
    return out


class Case:
    def __init__(self, name, targets, source, foreign, run, want):
        self.name, self.targets, self.source, self.foreign, self.run, self._want = name, targets, source, foreign, run, want

    def want(self):
        return None if self._want is None else memo(("want", self.name), self._want)

    def __repr__(self):
        return self.name


T_CABI, T_RUNS = "tests/test_gpu_cabi.py", "tests/test_gpu_bucket_runs.py"
T_P8, T_H = "tests/test_gpu_p8_primitives.py", "tests/test_gpu_pinocchio_h.py"
T_PB, T_NL = "tests/test_gpu_pinocchio_batch_primitives.py", "tests/test_gpu_nullity.py"
T_PAIR, T_NTT = "tests/test_gpu_bn256_pairing.py", "tests/test_gpu_poly_mul_ntt.py"

# (the `foreign` column is ordered by the arena bytes each case takes, measured on an MI355X: EXPERIMENTS.md A.1)
CASES = [
    Case("ed_msm", [("msm.hip", "vmpc_msm_dev")], T_RUNS + "::test_heavy_bucket_with_the_planners_segments",
         "ed_short", ed_msm_run, ed_msm_want),
    Case("ed_table_wide", [("msm.hip", "msm_table_batch_wide")], T_RUNS + "::test_heavy_bucket_with_64_entry_segments",
         "ed_table_batch", ed_wide_run, ed_wide_want),
    Case("ed_table_batch", [("msm.hip", "msm_table_batch")], T_CABI + "::test_table_batch_equals_single_commitments",
         "ed_table_wide", ed_table_batch_run, ed_table_batch_want),
    Case("ed_short", [("msm_short.hip", "msm_short_batch")], "tests/test_gpu_short_path.py::test_short_path_matches_oracle",
         "ntt_poly_mul", ed_short_run, ed_short_want),
    Case("ed_fixed_base", [("msm.hip", "vmpc_fixed_base_dev")], T_CABI + "::test_fixed_base_comb_matches_oracle",
         "cs_tables", ed_fixed_base_run, ed_fixed_base_want),
    Case("ed_validate", [("msm.hip", "vmpc_points_validate_dev")], T_CABI + "::test_normalize_and_lift",
         "bn_validate", ed_validate_run, ed_validate_want),
    Case("ed_tree_reduce", [("exact.hip", "vmpc_tree_reduce_dev")], T_CABI + "::test_tree_reduce_order",
         "ed_fixed_base", ed_tree_reduce_run, ed_tree_reduce_want),
    Case("ed_table_fold", [("fold_jump.hip", "table_fold")], T_CABI + "::test_table_fold_equals_k_reference_folds",
         "ed_fixed_base", ed_table_fold_run, ed_table_fold_want),
    Case("format", [("format.hip", "fmt_common")], T_CABI + "::test_transcript_text",
         "format_async", format_run, format_want),
    Case("format_async", [("format.hip", "fmt_async")], "tests/test_gpu_formats.py::test_text_delivered_in_pieces_equals_the_whole",
         "format", format_async_run, format_want),
    Case("fr_dot", [("frvec.hip", "vmpc_fr_dot_dev")], "tests/test_gpu_frvec.py::test_dot_and_dot_to_dev",
         "fr_dot_to_dev", fr_dot_run, fr_dot_want),
    Case("fr_dot_to_dev", [("frvec.hip", "vmpc_fr_dot_to_dev")], "tests/test_gpu_frvec.py::test_dot_and_dot_to_dev",
         "fr_dot", fr_dot_to_dev_run, fr_dot_want),
    Case("fr_rows_combine", [("nullity.hip", "vmpc_fr_rows_combine_dev")],
         T_NL + "::test_combine_tall_shapes_take_the_segmented_path", "fr_rows_dot", fr_rows_combine_run, fr_rows_combine_want),
    Case("fr_rows_dot", [("nullity.hip", "vmpc_fr_rows_dot_dev")], T_NL + "::test_rows_dot_matches_the_restatement",
         "cs_extend", fr_rows_dot_run, fr_rows_dot_want),
    Case("fr_batch_products", [("batch_verify.hip", "vmpc_fr_batch_products_dev")],
         "tests/test_gpu_batch_products.py::test_matches_reference", "cs_extend", fr_batch_products_run, fr_batch_products_want),
    Case("cs_tables", [("circuit_sat.hip", "vmpc_fr_cs_tables_dev")], T_P8 + "::test_factorial_tables",
         "cs_lagrange", cs_tables_run, cs_tables_want),
    Case("cs_lagrange", [("circuit_sat.hip", "vmpc_fr_cs_lagrange_dev")], T_P8 + "::test_lagrange_vector",
         "cs_tables", cs_lagrange_run, cs_lagrange_want),
    Case("cs_extend", [("circuit_sat.hip", "cs_extend")], T_P8 + "::test_extension",
         "cs_tables", cs_extend_run, cs_extend_want),
    Case("colsum", [("fr_colsum.h", "fr_colsum")], "tests/test_gpu_colsum.py::test_one_plan_through_both_fields",
         "cs_tables", colsum_run, colsum_want),
    Case("bn_msm", [("bn256.hip", "bn_msm_dev")], T_RUNS + "::test_bn256_heavy_bucket_full_segment_plus_remainder",
         "bn_table_msm", bn_msm_run, bn_msm_want),
    Case("bn_table_msm", [("bn256.hip", "bn_table_msm_dev")], "tests/test_gpu_bn256_edges.py::test_table_extreme_buckets",
         "bn_table_msm_multi", bn_table_msm_run, bn_table_msm_want),
    Case("bn_table_msm_multi", [("bn256.hip", "bn_table_msm_multi_dev")],
         "tests/test_gpu_bn256_edges.py::test_table_extreme_buckets", "ed_short", bn_table_msm_multi_run,
         bn_table_msm_multi_want),
    Case("bn_validate", [("bn256.hip", "vmpc_bn256_validate_dev")], "tests/test_gpu_bn256.py::test_full_size_exponent_identity",
         "ed_validate", bn_validate_run, bn_validate_want),
    Case("bn_qap_lagrange", [("bn256_keygen.hip", "vmpc_bn256_qap_lagrange_dev")],
         "tests/test_gpu_pinocchio_keygen.py::test_special_s_sparse_and_dense", "qh_weights", bn_qap_lagrange_run,
         bn_qap_lagrange_want),
    Case("koe_poly_mul", [("bn256_koe.hip", "koe_poly_mul")], T_PB + "::test_product_batch_windows",
         "mtree_build", koe_poly_mul_run, koe_poly_mul_want),
    Case("ntt_poly_mul", [("bn256_ntt.hip", "vmpc_ntt_poly_mul")], T_NTT + "::test_every_pass_plan_against_schoolbook",
         "ed_table_batch", ntt_poly_mul_run, ntt_poly_mul_want),
    Case("mtree_build", [("bn256_qap_mtree.hip", "mt_build")],
         "tests/test_gpu_moments_tree.py::test_primitive_random_unreduced_and_all_n_minus_1", "qh_weights", mtree_build_run,
         mtree_want),
    Case("mtree_moments", [("bn256_qap_mtree.hip", "mt_moments"), ("bn256_ntt.hip", "vmpc_ntt_tree_level")],
         "tests/test_gpu_moments_tree.py::test_primitive_random_unreduced_and_all_n_minus_1", "cs_tables", mtree_moments_run,
         mtree_want),
    Case("bn_pairing", [("bn256_pairing.hip", "vmpc_bn256_pairing_dev")], T_PAIR + "::test_pairing_batches",
         "bn_pairing_product", bn_pairing_run, bn_pairing_want),
    Case("bn_pairing_product", [("bn256_pairing.hip", "vmpc_bn256_pairing_product_dev")],
         T_PAIR + "::test_pairing_product_lengths_and_offsets", "bn_pairing", bn_pairing_product_run, bn_pairing_product_want),
    Case("qh_moments", [("bn256_qap_h.hip", "qh_moments")], T_H + "::test_moments_primitive",
         "qh_weights", qh_moments_run, qh_moments_want),
    Case("qh_weights", [("bn256_qap_h.hip", "qh_weights")], T_H + "::test_weights_at_scan_boundaries",
         "cs_tables", qh_weights_run, qh_weights_want),
    Case("qh_residual", [("bn256_qap_h.hip", "qh_residual")],
         "tests/test_gpu_qap_residual_batch.py::test_batch_against_the_reference_and_the_single_entry", "qh_moments",
         qh_residual_run, qh_residual_want),
    Case("qh_combine", [("bn256_qap_h.hip", "qh_combine")], T_PB + "::test_combine_batch",
         "koe_poly_mul", qh_combine_run, qh_combine_want),
    Case("prover", [("prover.hip", "p4_round_enqueue")], "tests/test_gpu_batch_verify.py::test_valid_proofs_one_combined_check",
         "ed_short", prover_run, None),
]
BY_NAME = {c.name: c for c in CASES}


def arena_users():
    """{(file, function)} for every function of csrc/*.hip and *.h whose body calls vmpc_ws_reserve (comments dropped;
    a function is a top-level `name(...) {` block, blocks of `extern "C"` and namespaces looked through)"""
    import glob
    import re
    found = set()
    src_dir = os.path.join(ROOT, "verifiable_mpc_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(src_dir, "*.hip")) + glob.glob(os.path.join(src_dir, "*.h"))):
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)
        for m in re.finditer(r"\bvmpc_ws_reserve\s*\(", text):
            open_braces = []
            for j, ch in enumerate(text[:m.start()]):
                if ch == "{":
                    open_braces.append(j)
                elif ch == "}":
                    open_braces.pop()
            for b in open_braces:               # the outermost enclosing block that follows a parameter list
                head = text[:b].rstrip()
                if not head.endswith(")"):
                    continue
                depth, k = 0, len(head) - 1
                while k >= 0:
                    depth += (head[k] == ")") - (head[k] == "(")
                    if depth == 0:
                        break
                    k -= 1
                found.add((os.path.basename(path), re.search(r"([A-Za-z_]\w*)\s*$", head[:k]).group(1)))
                break
    return found
