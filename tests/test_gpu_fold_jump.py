"""The fold jump (csrc/fold_jump.hip) kernel by kernel at its digit, share and group edges.

Every case is ONE call of vmpc_msm_table_fold_dev or vmpc_msm_table_fold_table_dev over points g_i = e_i B made on the
device, so that output j must be ((sum_b s_b e[j + b m_out]) mod l) B.  All outputs are compared byte for byte with
vmpc_fixed_base_dev of those exponents (pinned by test_gpu_cabi.py::test_fixed_base_comb_matches_oracle), a sample -
outputs 0, 1, 63, 64, 65, m_out - 1 and three random ones - with oracle/ed25519_ref.py.  Before the call the case reads
the plan (Context.msm_table_fold_plan, csrc/fold_jump_plan.h - the code table_fold() itself calls) and asserts WHICH
path it is about to take: digit width, O, the share count S, n_blocks and the grid against the table in
tests/fold_jump_ref.py (SHAPES), every field and the schedule against the restatement there.  A case prints one
`FOLDVIEW` line (EXPERIMENTS.md keeps the table).

Shapes: more than one group of 64 outputs (the block-to-output remap with per_xcd = 2 and more), more than one offset
group, S = 1 .. 16 at both ends of the lane cap and of the 8-entries rule, one output, k_fold_jump (4-bit digits) at
rows = 16 and - in a context created under VMPC_FOLD_JUMP_DIGITS=4 - at rows <= 8, where it has several offset groups.
Scalars (fold_jump_ref.patterns): random, all zero, one-hot (the output is a column itself), one power of the digit
base per digit position, the recoding edges (+-128 / +-127, +-8 / +-7, a carry through every position, l - 1, 2^252),
all entries of an offset on one |digit|, and columns that repeat or cancel so that `run` doubles and passes through the
neutral element.  The table form runs at m_out = 1, 2, 128, 256 against vmpc_msm_table_build_dev of the fold's own
vector, and the prover's prebuilt-extras path (k_copy_columns) through _native.P4Rounds.

144 tests, 4.5 s on an MI355X.  Each of these arithmetic-only changes of the library makes cases of this file fail
(EXPERIMENTS.md section J.3 has the lists): the closing entry's step-down skipped (89 tests); the negate bit ignored
(46); k_fold_jump_combine doubling digit_bits - 1 times (111); k_fold_jump_table leaving out the S slots of the last
offset (39).  The two host-side ones - the recoding dropping the carry out of a digit equal to half, an ascending
sort - already fail tests/test_native_fold_jump_plan_host.py on the CPU."""
import random

import numpy as np
import pytest

from oracle import ed25519_ref as ed
from tests import fold_jump_ref as ref
from tests.test_gpu_cabi import aff_bytes, gpu_points, sc_bytes
from tests.test_gpu_msm_sort import env_ctx

pytestmark = pytest.mark.gpu
ELL, P = ed.ELL, ed.P
SMALL = [key for key, want in ref.SHAPES.items() if want[3] <= 256]
LANE_CAP = [key for key, want in ref.SHAPES.items() if want[3] > 256]
NEUTRAL = (0).to_bytes(32, "little") + (1).to_bytes(32, "little")
# table form: m_out = 1, 2, 128, 256 (a lone quad, then one, two and four workgroups of 64 quads); the two shapes that
# are not in ref.SHAPES with (digit_bits, O, S, m_out, n_blocks) worked out by hand from the rules
TABLE_SHAPES = {(1, 6, 64, 8): ref.SHAPES[1, 6, 64, 8], (16, 6, 64, 8): ref.SHAPES[16, 6, 64, 8],
                (4, 5, 64, 8): (8, 8, 16, 2, 2), (1, 1, 256, 8): ref.SHAPES[1, 1, 256, 8],
                (16, 1, 256, 8): ref.SHAPES[16, 1, 256, 8], (16, 2, 1024, 8): ref.SHAPES[16, 2, 1024, 8],
                (8, 2, 1024, 8): (8, 4, 4, 256, 4)}      # 32 entries an offset: S = 4 leaves 8 a share


def shape_id(key):
    return "rows%d-k%d-n%d-%dbit" % (key[0], key[1], key[2], ref.geometry(key[0], key[2], key[1], key[3])["digit_bits"]) \
        + ("-knob4" if key[3] == 4 else "")


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


@pytest.fixture(scope="module")
def ctxs(nat):
    """8: the default context; 4: one created under VMPC_FOLD_JUMP_DIGITS=4 (k_fold_jump at every row count)"""
    c = {8: env_ctx(nat), 4: env_ctx(nat, VMPC_FOLD_JUMP_DIGITS=4)}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module")
def tables(nat, ctxs):
    """(ctx, exponents, points, table, base point) per shape, made once: the two 64-MiB tables among them"""
    cache = {}

    def get(key, variant="plain"):
        if (key, variant) not in cache:
            rows, k, n_cols, knob = key
            ctx = ctxs[knob]
            rng = random.Random(hash((rows, k, n_cols, knob)) & 0xffff)
            exps = [rng.randrange(1, ELL) for _ in range(n_cols)]
            if variant == "dup":
                m_out = n_cols >> k
                exps = ref.dup_opposite(exps, m_out, k, sorted({0, m_out // 2, m_out - 1}))
            pts = gpu_points(nat, ctx, exps)
            table = ctx.msm_table_build(pts.ptr, n_cols, None, 0, rows)
            ctx.sync()
            cache[key, variant] = (ctx, exps, pts, table, ctx.upload(aff_bytes([ed.BASE])))
        return cache[key, variant]
    yield get
    cache.clear()


def check_plan(ctx, key, want, scalars, label, full=True):
    """the plan of the call that follows: the path facts against `want`, the rest against the restatement"""
    rows, k, n_cols, knob = key
    geo, sched = ctx.msm_table_fold_plan(rows, n_cols, scalars)
    if label:
        print("\nFOLDVIEW | %s | %s | %d | %d | %d | %d | %d | %d | %d | %d x %d | %d |" % (
            shape_id(key), label, rows, k, n_cols, geo["digit_bits"], geo["O"], geo["S"], geo["m_out"],
            geo["grid_x"], geo["grid_y"], geo["n_blocks"]))
    assert (geo["digit_bits"], geo["O"], geo["S"], geo["m_out"], geo["n_blocks"]) == want
    assert (geo["grid_x"], geo["grid_y"]) == ((want[4] + 7) // 8 * 8, want[2])
    assert geo == ref.geometry(rows, n_cols, k, knob)
    if full:
        assert np.array_equal(sched, ref.schedule(geo, rows, scalars))
    return geo


def sample(m_out, rng):
    js = {j for j in (0, 1, 63, 64, 65, m_out - 1) if j < m_out}
    js.update(rng.randrange(m_out) for _ in range(3))
    return sorted(js)


def check_fold(nat, entry, key, scalars, rng, label=None, want_bytes=None):
    ctx, exps, pts, table, dbase = entry
    rows, k, n_cols, knob = key
    geo = check_plan(ctx, key, ref.SHAPES[key], scalars, label, full=key in SMALL)
    m_out = geo["m_out"]
    out, fb = ctx.alloc(64 * m_out), ctx.alloc(64 * m_out)
    ctx.msm_table_fold(table.ptr, n_cols, 0, rows, n_cols, scalars, out.ptr)
    want_exp = ref.fold_exponents(scalars, exps, m_out)
    dw = ctx.upload(sc_bytes(nat, want_exp))
    ctx.fixed_base(dbase.ptr, dw.ptr, m_out, fb.ptr)
    ctx.sync()
    got, want = ctx.download(out.ptr, 64 * m_out).tobytes(), ctx.download(fb.ptr, 64 * m_out).tobytes()
    if got != want:
        bad = [j for j in range(m_out) if got[64 * j:64 * j + 64] != want[64 * j:64 * j + 64]]
        raise AssertionError("%d of %d outputs differ from vmpc_fixed_base_dev, the first at %s" % (len(bad), m_out, bad[:8]))
    for j in sample(m_out, rng):
        assert ed.affine_from_bytes(got[64 * j:64 * j + 64])[:2] == ed.pt_affine(ed.pt_repeat(ed.BASE, want_exp[j])), j
    if want_bytes is not None:
        assert got == want_bytes
    return got


def pattern_calls(key, name):
    rows, k, n_cols, knob = key
    bits = ref.geometry(rows, n_cols, k, knob)["digit_bits"]
    return [sc for _, sc in ref.patterns(k, bits, random.Random(k * 64 + rows + len(name)), names=(name,))]


@pytest.mark.parametrize("name", ["random", "zero", "onehot", "powers", "edges", "level"])
@pytest.mark.parametrize("key", SMALL, ids=shape_id)
def test_fold_small_shapes_every_pattern(nat, tables, key, name):
    entry = tables(key)
    ctx, exps, pts, table, dbase = entry
    rows, k, n_cols, knob = key
    m_out = n_cols >> k
    rng = random.Random(len(name) + rows)
    for i, scalars in enumerate(pattern_calls(key, name)):
        want_bytes = None
        if name == "zero":
            want_bytes = NEUTRAL * m_out
        elif name == "onehot":                       # the column itself: no arithmetic of any reference
            b = scalars.index(1)
            want_bytes = ctx.download(pts.ptr + 64 * b * m_out, 64 * m_out).tobytes()
        check_fold(nat, entry, key, scalars, rng, label=name if i == 0 else None, want_bytes=want_bytes)


@pytest.mark.parametrize("key", SMALL, ids=shape_id)
def test_fold_duplicate_and_opposite_columns(nat, tables, key):
    """e[j + m_out] = e[j] and e[j + 2 m_out] = l - e[j] for the first, a middle and the last output: with equal
    scalars `run` adds a point to itself, with s = (1, 0, 1, 0, ..) it passes through the neutral element"""
    entry = tables(key, "dup")
    rng = random.Random(key[0] + 5)
    for i, scalars in enumerate(ref.dup_opposite_scalars(key[1], rng)):
        check_fold(nat, entry, key, scalars, rng, label="dup/opposite" if i == 0 else None)


@pytest.mark.parametrize("name", ["random", "onehot"])
@pytest.mark.parametrize("key", LANE_CAP, ids=shape_id)
def test_fold_at_the_lane_cap(nat, tables, key, name):
    """m_out O S = 2^17 lanes and the first size beyond, where S halves: 32 and 64 workgroups, per_xcd = 4 and 8"""
    entry = tables(key)
    ctx, exps, pts, table, dbase = entry
    m_out = key[2] >> key[1]
    rng = random.Random(key[2] + len(name))
    calls = pattern_calls(key, name)
    for i, scalars in enumerate(calls):
        want_bytes = None
        if name == "onehot":
            want_bytes = ctx.download(pts.ptr + 64 * scalars.index(1) * m_out, 64 * m_out).tobytes()
        check_fold(nat, entry, key, scalars, rng, label=name if i == 0 else None, want_bytes=want_bytes)


def fe_limbs(words):
    """csrc/fe25519.h: ten limbs, limb i at bit ceil(25.5 i)"""
    return sum(int(w) << ((51 * i + 1) // 2) for i, w in enumerate(words)) % P


def niels_affine(line):
    """(x, y) of a 128-byte table entry (y - x, y + x, 2 d x y; csrc/ptio.h), with its third field checked"""
    w = np.frombuffer(line, np.uint32)
    ymx, ypx, t2d = fe_limbs(w[0:10]), fe_limbs(w[10:20]), fe_limbs(w[20:30])
    inv2 = (P + 1) // 2
    x, y = (ypx - ymx) * inv2 % P, (ypx + ymx) * inv2 % P
    assert t2d == 2 * ed.D * x * y % P and not w[30:].any()
    return x, y


@pytest.mark.parametrize("n_extra", [0, 2])
@pytest.mark.parametrize("out_rows", [1, 4, 16])
@pytest.mark.parametrize("key", list(TABLE_SHAPES), ids=shape_id)
def test_fold_table_form(nat, tables, key, out_rows, n_extra):
    """vmpc_msm_table_fold_table_dev (k_fold_jump_table: the S shares, Horner, the rows' doublings and the shared
    inversion by a quad of lanes per output) leaves byte for byte the table vmpc_msm_table_build_dev makes of
    vmpc_msm_table_fold_dev's vector; its row 0 is that vector; with all scalars zero every entry is the neutral
    element's."""
    ctx, exps, pts, table, dbase = tables(key)
    rows, k, n_cols, knob = key
    m_out = n_cols >> k
    rng = random.Random(out_rows * 10 + n_extra + rows)
    extras = gpu_points(nat, ctx, [rng.randrange(1, ELL) for _ in range(n_extra)]) if n_extra else None
    stride = (m_out + n_extra + 7) // 8 * 8
    edge = [ref.EDGE_SCALARS[(i + out_rows) % len(ref.EDGE_SCALARS)] for i in range(1 << k)]
    for label, scalars in (("table random", [rng.randrange(ELL) for _ in range(1 << k)]), ("table edges", edge),
                           ("table zero", [0] * (1 << k))):
        check_plan(ctx, key, TABLE_SHAPES[key], scalars, label if (out_rows, n_extra) == (1, 0) else None)
        folded = ctx.alloc(64 * m_out)
        ctx.msm_table_fold(table.ptr, n_cols, 0, rows, n_cols, scalars, folded.ptr)
        want = ctx.msm_table_build(folded.ptr, m_out, extras.ptr if extras else None, n_extra, out_rows)
        got = ctx.msm_table_fold_table(table.ptr, n_cols, 0, rows, n_cols, scalars, extras.ptr if extras else None,
                                       n_extra, out_rows)
        ctx.sync()
        nbytes = out_rows * stride * 128
        g, w = ctx.download(got.ptr, nbytes).tobytes(), ctx.download(want.ptr, nbytes).tobytes()
        if g != w:
            bad = [(i // stride, i % stride) for i in range(out_rows * stride) if g[128 * i:128 * i + 128] != w[128 * i:128 * i + 128]]
            raise AssertionError("%s: %d entries differ from vmpc_msm_table_build_dev, the first (row, column) %s" %
                                 (label, len(bad), bad[:6]))
        vec = ctx.download(folded.ptr, 64 * m_out).tobytes()
        fb = ctx.alloc(64 * m_out)                    # the vector itself, for the shapes no other test of the file runs
        dw = ctx.upload(sc_bytes(nat, ref.fold_exponents(scalars, exps, m_out)))
        ctx.fixed_base(dbase.ptr, dw.ptr, m_out, fb.ptr)
        ctx.sync()
        assert vec == ctx.download(fb.ptr, 64 * m_out).tobytes(), label
        for j in range(m_out):                        # row 0 is the vector
            assert niels_affine(g[128 * j:128 * j + 128]) == ed.affine_from_bytes(vec[64 * j:64 * j + 64])[:2], j
        if label == "table zero":
            assert vec == NEUTRAL * m_out
            for r in range(out_rows):
                for j in range(m_out):
                    assert niels_affine(g[128 * (r * stride + j):128 * (r * stride + j) + 128]) == (0, 1), (r, j)


@pytest.mark.parametrize("rows,jump_k", [(16, 5), (4, 5), (4, 3)])
def test_prebuilt_extras_round_after_the_fold(monkeypatch, rows, jump_k):
    """_native.P4Rounds at N = 2^9 under VMPC_P4_JUMP_MIN_LOG2=3: the fold leaves 2^9 >> jump_k columns, a multiple
    of 8, so k's columns of the new table are copied from the prebuilt block (k_copy_columns).  Every round - the one
    right after the fold in particular - equals the same round of a context that never folds."""
    import verifiable_mpc_amd as vm
    monkeypatch.setenv("VMPC_P4_JUMP_MIN_LOG2", "3")
    ctx = vm.get_context()
    group = vm.EllipticCurve("Ed25519", "projective")
    h = group.generator
    rng = random.Random(rows + jump_k)
    k = vm.Ed25519Point.repeat(h, rng.randrange(1, ELL))
    n = (1 << 9) - 1
    g = vm.PointVector.fixed_base(h, [rng.randrange(1, ELL) for _ in range(n)])
    g.precompute([h, k], rows=rows)
    z = vm.ScalarVector.from_ints([rng.randrange(ELL) for _ in range(n + 1)])
    L = vm.ScalarVector.from_ints([rng.randrange(ELL) for _ in range(n + 1)])
    cs = [None] + [rng.randrange(1, ELL) for _ in range(7)]
    last = rng.randrange(1, ELL)
    assert ((n + 1) >> jump_k) % 8 == 0

    def rounds(jk):
        ctx.profile(True)
        r = vm._native.P4Rounds(ctx, g._table, 1, 1, z.ptr, L.ptr, jump_k=jk)
        out = [r.round(c) for c in cs]
        out.append(r.finish(last))
        r.close()
        stages = {name: cnt for name, (ms, cnt) in ctx.profile_read(reset=True).items() if cnt}
        ctx.profile(False)
        return out, stages
    want, plain_stages = rounds(0)
    got, stages = rounds(jump_k)
    assert "table_fold" not in plain_stages and stages.get("table_fold", 0) >= 1
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "round %d (the fold is made at the start of round %d)" % (i, jump_k)
