"""The NTT route of Protocol 8's extension (csrc/circuit_sat.hip cs_extend under vmpc_ctx_set_cs_extension;
csrc/bn256_ntt.hip k_ntt_crt<fr>) through the three entries, against tests/p8_ref.py and against
the direct kernel on the same device buffers.  Every comparison is exact (integer lists mod l, or the bytes).

What the shapes stand for, restated here (nothing is imported from the code under test but the AUTO threshold, which is
a measured figure): l = 2^252 + 27742317777372353535851937790883648493; the route multiplies the 2K rows u_f, u_g
(M = m + 1 terms) with T (2m + 2 terms) cyclically at L = the smallest power of two >= 2m + 2 and keeps the coefficients
m+1 .. 2m-1, modulo 18 primes below 2^31; NTT_LDS_LEN = 2048 points run in one workgroup's LDS, longer transforms add
one column pass of up to 6 stages (up to L = 2^17) or two; a group of rows is at most 65535 (a grid dimension) and at
most what the NTT's arena cap holds beside T's row, a row being 18 x L x 4 bytes.
    m = 0, 1          no correlation: nothing new is launched, the mode changes nothing
    m = 2             L = 8, one output
    m = 3             L = 8 = 2m + 2: the alias bound met with equality
    m = 4, 63, 64, 255, 256, 257    L = 16 .. 1024, around the direct kernel's chunk, segment and tile edges
    m = 1023          L = 2048 = 2m + 2: the longest one-kernel transform, bound tight
    m = 1024, 1025    L = 4096: the first column pass, one stage
    m = 4097          L = 16384: three column stages
    m = 32767, 65535  L = 2^16, 2^17 tight (5 and 6 column stages: the longest single pass); m = 32768: L = 2^17;
    m = 65536         L = 2^18: two column passes.  These against the direct kernel - the host reference is too slow.
    "top"             every value l - 1: u = (l - 1) w_j, the largest integer coefficients the sizes allow
    (2, 40000)        80000 rows: two groups, the boundary at row 65535 = u_g of witness 25535
"""
import functools
import os
import random
import re

import numpy as np
import pytest

from tests import p8_ref as ref

pytestmark = pytest.mark.gpu

ELL = ref.ELL
MAX_M = 1 << 20                             # VMPC_FR_CS_MAX_M of include/vmpc.h
PAT_BYTE = 0xA5
PAT = int.from_bytes(bytes([PAT_BYTE]) * 32, "little")      # above l: no kernel here can write it
DIRECT_STAGES = ["cs_extend_prep", "cs_extend_corr", "cs_extend_finish"]
NTT_STAGES = ("cs_extend_ntt_split", "cs_extend_ntt_fwd", "cs_extend_ntt_inv", "cs_extend_ntt_crt")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def ctx(vm):
    c = vm.get_context()
    assert c.get_cs_extension() == 0        # a new context's: the direct kernel
    return c


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _ints(a):
    raw = a.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _pattern(ctx, n):
    return ctx.upload(np.full((n, 32), PAT_BYTE, np.uint8))


def _get(ctx, buf, n):
    ctx.sync()
    return _ints(ctx.download(buf.ptr, 32 * n))


def _written(m):
    return [0, 1, 2] + ([2 + m + 1] if m else []) + [2 + x for x in range(m + 2, 2 * m + 1)]


def launches(ctx, fn):
    """stage name -> launches recorded while fn() ran"""
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        fn()
        ctx.sync()
        return {k: v[1] for k, v in ctx.profile_read(reset=True).items() if v[1]}
    finally:
        ctx.profile(False)


@functools.lru_cache(maxsize=None)
def case(m, kind):
    """(a, b, the reference's z tail): computed once, shared by the tests that use the shape"""
    M = m + 1
    rng = random.Random(9000 + m)
    if kind == "top":
        a, b = [ELL - 1] * M, [ELL - 1] * M
    else:
        a, b = [rng.randrange(ELL) for _ in range(M)], [rng.randrange(ELL) for _ in range(M)]
        if kind == "zero_a":
            a = [0] * M
    return a, b, ref.z_tail_bary(a[:m], b[:m], a[m], b[m])


def _device_tables(ctx, m):
    K = max(2 * m + 1, 1)
    fact, ifact = ctx.alloc(32 * (K + 1)), ctx.alloc(32 * (K + 1))
    ctx.cs_tables(K, fact.ptr, ifact.ptr)
    return fact, ifact


# ---- vmpc_fr_cs_extend_dev against the host reference ----------------------------------------------------------------
SMALL_M = [0, 1, 2, 3, 4, 63, 64, 255, 256, 257, 1023, 1024, 1025, 4097]
SMALL_CASES = [(m, "random") for m in SMALL_M] + [(m, "top") for m in (3, 1023, 1024, 4097)] + \
              [(m, "zero_a") for m in (2, 1023)]


@pytest.mark.parametrize("m,kind", SMALL_CASES, ids=[f"m{m}_{k}" for m, k in SMALL_CASES])
def test_extension_under_the_ntt(vm, ctx, m, kind):
    a, b, want = case(m, kind)
    K = max(2 * m + 1, 1)
    fact, ifact = (ctx.upload(_bytes(t)) for t in ref.tables(K))      # the tables from the host
    d_a, d_b = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
    n_z = 2 * m + 3
    written = _written(m)
    assert len(want) == n_z
    runs = []
    with vm.device.cs_extension("ntt"):
        for _ in range(2):
            z = _pattern(ctx, n_z + 1)
            ctx.cs_extend(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, z.ptr)
            runs.append(_get(ctx, z, n_z + 1))
    got = runs[0]
    assert [got[p] for p in written] == [want[p] for p in written]
    # the gammas' places and the scalar past the end keep the pattern
    assert got[3:3 + m] == [PAT] * m and got[n_z] == PAT
    if kind == "zero_a":
        assert all(got[p] == 0 for p in written if p != 1) and got[1] != 0
    assert runs[1] == got                       # integer sums in a fixed order: the same bytes every time


# ---- large m against the direct kernel on the same buffers ------------------------------------------------------------
LARGE_CASES = [(m, k) for m in (32767, 32768, 65535, 65536) for k in ("random", "top")]


@pytest.mark.parametrize("m,kind", LARGE_CASES, ids=[f"m{m}_{k}" for m, k in LARGE_CASES])
def test_large_extension_against_the_direct_kernel(vm, ctx, m, kind):
    M, n_z = m + 1, 2 * m + 3
    fact, ifact = _device_tables(ctx, m)
    if kind == "top":
        img = np.broadcast_to(_bytes([ELL - 1])[0], (2, M, 32)).copy()
    else:
        img = np.random.default_rng(9200 + m).integers(0, 256, size=(2, M, 32), dtype=np.uint8)
        img[:, :, 31] &= 0x0f                   # below 2^252 < l: canonical
    d_a, d_b = ctx.upload(img[0]), ctx.upload(img[1])
    out = {}
    for mode in ("direct", "ntt"):
        z = _pattern(ctx, n_z + 1)
        with vm.device.cs_extension(mode):
            seen = launches(ctx, lambda: ctx.cs_extend(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, z.ptr))
        assert ("cs_extend_corr" in seen) == (mode == "direct") and ("cs_extend_ntt_crt" in seen) == (mode == "ntt"), seen
        ctx.sync()
        out[mode] = ctx.download(z.ptr, 32 * (n_z + 1)).reshape(-1, 32).copy()
    assert np.array_equal(out["ntt"], out["direct"])
    got = out["ntt"]
    assert (got[3:3 + m] == PAT_BYTE).all() and (got[n_z] == PAT_BYTE).all()
    assert (got[_written(m), 31] <= 0x10).all()          # every place of the entry's was written
    if kind == "top":                           # f and g are the constant l - 1 = -1: h = 1 wherever it is evaluated
        assert _ints(got[m + 4:m + 4 + 64]) == [1] * 64 and _ints(got[:3]) == [ELL - 1, ELL - 1, 1]
    else:
        assert len({bytes(r) for r in got[m + 4:m + 4 + 64]}) == 64


# ---- vmpc_fr_cs_extend_fg_dev -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 257, 4097])
def test_share_variant_under_the_ntt(vm, ctx, m):
    a, b, want = case(m, "random")
    fact, ifact = _device_tables(ctx, m)
    d_a, d_b = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
    out = {}
    for mode in ("direct", "ntt"):
        f, g = _pattern(ctx, m + 1), _pattern(ctx, m + 1)
        with vm.device.cs_extension(mode):
            ctx.cs_extend_fg(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, f.ptr, g.ptr)
        out[mode] = (_get(ctx, f, m + 1), _get(ctx, g, m + 1))
    assert out["ntt"] == out["direct"]
    f, g = out["ntt"]
    assert f[m] == PAT and g[m] == PAT and PAT not in f[:m] + g[:m]
    # f(x) g(x) = h(x): the reference's z tail at 0 and m+2 .. 2m
    assert [x * y % ELL for x, y in zip(f[:m], g[:m])] == [want[2]] + [want[2 + x] for x in range(m + 2, 2 * m + 1)]
    assert (f[0], g[0]) == (want[0], want[1])


# ---- vmpc_fr_cs_extend_batch_dev --------------------------------------------------------------------------------------
N_IN = 2                                    # z_tail starts inside the row


def _batch(vm, ctx, m, n_wit, modes=("direct", "ntt"), top_last=True, seed=0):
    """one batch per mode on the same device buffers, strides above the minimum -> ({mode: the z image as rows of 32
    bytes}, the row values, (zs, N)); after each mode's call the arena is checked against what the context reports"""
    M = m + 1
    N = N_IN + 2 * m + 3
    zs, abs_ = N + 5, m + 6
    fact, ifact = _device_tables(ctx, m)
    rng = np.random.default_rng(9300 + m + n_wit + seed)
    imgs = []
    for _ in range(2):
        img = np.full((n_wit, abs_, 32), PAT_BYTE, np.uint8)
        img[:, :M] = rng.integers(0, 256, size=(n_wit, M, 32), dtype=np.uint8)
        img[:, :M, 31] &= 0x0f
        if top_last:
            img[n_wit - 1, :M] = _bytes([ELL - 1])[0]
        imgs.append(img)
    d_a, d_b = ctx.upload(imgs[0]), ctx.upload(imgs[1])
    out = {}
    for mode in modes:
        with vm.device.cs_extension(mode):
            for attempt in range(2):            # the second call finds the arena the first one left
                z = _pattern(ctx, n_wit * zs + 1)
                before = ctx.debug_arena_info()
                ctx.cs_extend_batch(d_a.ptr, d_b.ptr, abs_, m, fact.ptr, ifact.ptr, z.ptr + 32 * N_IN, zs, n_wit)
                ctx.sync()
                size, used, gen = ctx.debug_arena_info()
                assert 0 < used <= ctx.cs_extend_batch_bytes(m, n_wit) <= size, (mode, used, size)
            assert gen == before[2] and size == before[0], "the arena grew during a call it was large enough for"
        out[mode] = ctx.download(z.ptr, 32 * (n_wit * zs + 1)).reshape(-1, 32).copy()
    return out, imgs, (zs, N)


def _check_batch_image(got, m, n_wit, zs):
    written = _written(m)
    untouched = np.ones(n_wit * zs + 1, bool)
    for w in range(n_wit):
        untouched[[w * zs + N_IN + p for p in written]] = False
    assert (got[untouched] == PAT_BYTE).all()           # the x part, the gammas' places, the gaps, the scalar past the end
    assert (got[~untouched, 31] <= 0x10).all()


def _check_witness(got, imgs, m, w, zs, N):
    a, b = _ints(imgs[0][w, :m + 1]), _ints(imgs[1][w, :m + 1])
    want = ref.z_tail_bary(a[:m], b[:m], a[m], b[m])
    mine = _ints(got[w * zs + N_IN:w * zs + N])
    assert [mine[p] for p in _written(m)] == [want[p] for p in _written(m)], w


BATCH_CASES = [(3, 1), (257, 5), (1025, 3)]


@pytest.mark.parametrize("m,n_wit", BATCH_CASES, ids=[f"m{m}_K{k}" for m, k in BATCH_CASES])
def test_batch_under_the_ntt(vm, ctx, m, n_wit):
    out, imgs, (zs, N) = _batch(vm, ctx, m, n_wit)
    assert np.array_equal(out["ntt"], out["direct"])
    _check_batch_image(out["ntt"], m, n_wit, zs)
    for w in range(n_wit):
        _check_witness(out["ntt"], imgs, m, w, zs, N)


def test_batch_rows_across_an_arena_group_boundary(vm, ctx):
    """m = 1025, K = 3: six rows of 18 x 4096 x 4 bytes; a cap of three rows holds T's and two of them, so the rows go
    in three groups"""
    m, n_wit, row_bytes = 1025, 3, 18 * 4096 * 4
    whole = ctx.cs_extend_batch_bytes(m, n_wit)
    ctx.set_ntt_arena_cap(3 * row_bytes)
    try:
        with vm.device.cs_extension("ntt"):
            capped = ctx.cs_extend_batch_bytes(m, n_wit)
        assert ctx.cs_extend_batch_bytes(m, n_wit) == whole         # the direct route does not know the cap
        out, imgs, (zs, N) = _batch(vm, ctx, m, n_wit)
    finally:
        ctx.set_ntt_arena_cap(0)
    with vm.device.cs_extension("ntt"):
        uncapped = ctx.cs_extend_batch_bytes(m, n_wit)
    assert uncapped - capped == 4 * row_bytes           # 1 + 6 rows against 1 + 2
    assert np.array_equal(out["ntt"], out["direct"])
    _check_batch_image(out["ntt"], m, n_wit, zs)
    for w in range(n_wit):
        _check_witness(out["ntt"], imgs, m, w, zs, N)
    # the same rows in one group
    again, _, _ = _batch(vm, ctx, m, n_wit, modes=("ntt",))
    assert np.array_equal(again["ntt"], out["ntt"])


def test_batch_of_more_rows_than_a_grid_dimension(vm, ctx):
    m, n_wit = 2, 40000
    out, imgs, (zs, N) = _batch(vm, ctx, m, n_wit)
    assert np.array_equal(out["ntt"], out["direct"])
    _check_batch_image(out["ntt"], m, n_wit, zs)
    for w in (0, 25534, 25535, 25536, 32767, 32768, n_wit - 1):     # 65535 - 40000 = 25535: u_g's row at the boundary
        _check_witness(out["ntt"], imgs, m, w, zs, N)


# ---- the mode ---------------------------------------------------------------------------------------------------------
def _single(ctx, m, seed=1):
    fact, ifact = _device_tables(ctx, m)
    img = np.random.default_rng(9400 + m + seed).integers(0, 256, size=(2, m + 1, 32), dtype=np.uint8)
    img[:, :, 31] &= 0x0f
    d_a, d_b = ctx.upload(img[0]), ctx.upload(img[1])
    z = _pattern(ctx, 2 * m + 4)
    keep = (fact, ifact, d_a, d_b)

    def run():
        ctx.cs_extend(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, z.ptr)
    return run, lambda: _get(ctx, z, 2 * m + 4), keep


def test_stage_lists(vm, ctx):
    run, read, _ = _single(ctx, 300)
    seen = launches(ctx, run)
    assert sorted(seen) == sorted(DIRECT_STAGES), seen          # the default mode: exactly today's stages
    want = read()
    with vm.device.cs_extension("ntt"):
        seen = launches(ctx, run)
    assert "cs_extend_corr" not in seen and all(s in seen for s in NTT_STAGES), seen
    assert sorted(seen) == sorted(["cs_extend_prep", "cs_extend_finish", *NTT_STAGES]), seen
    # T and the two rows: two splits and two forward transforms, one fused product and inverse, one reconstruction
    assert (seen["cs_extend_ntt_split"], seen["cs_extend_ntt_fwd"], seen["cs_extend_ntt_inv"],
            seen["cs_extend_ntt_crt"]) == (2, 2, 1, 1), seen
    assert read() == want
    # no correlation, nothing new: m = 0 and m = 1 under "ntt"
    for m in (0, 1):
        run, _, _ = _single(ctx, m)
        with vm.device.cs_extension("ntt"):
            seen = launches(ctx, run)
        assert sorted(seen) == ["cs_extend_finish", "cs_extend_prep"], (m, seen)
    # a poly_product block alone does not touch the extension
    run, read, _ = _single(ctx, 300)
    with vm.device.poly_product("ntt"):
        assert ctx.get_cs_extension() == 0
        seen = launches(ctx, run)
    assert sorted(seen) == sorted(DIRECT_STAGES), seen
    with vm.device.cs_extension("ntt"):
        assert ctx.get_poly_product() == 0


def test_auto_chooses_by_the_threshold(vm, ctx):
    t = vm._native.FR_CS_EXT_NTT_MIN
    assert t >= 4 and t & (t - 1) == 0
    for m, ntt in ((t - 1, False), (t, True)):
        run, read, _ = _single(ctx, m)
        run()
        want = read()
        with vm.device.cs_extension("auto"):
            assert ctx.get_cs_extension() == 1
            seen = launches(ctx, run)
        assert ("cs_extend_ntt_crt" in seen) == ntt and ("cs_extend_corr" in seen) == (not ntt), (m, seen)
        assert read() == want


def test_contracts(vm, ctx):
    nat = vm._native
    lib = ctx.lib
    for start in (0, 2):
        ctx.set_cs_extension(start)
        try:
            for bad in (-1, 3, 100):
                with pytest.raises(nat.VmpcError) as ei:
                    ctx.set_cs_extension(bad)
                assert ei.value.code == nat.E_INVAL
                assert ctx.get_cs_extension() == start
        finally:
            ctx.set_cs_extension(0)
    assert lib.vmpc_ctx_set_cs_extension(None, 0) == nat.E_INVAL
    assert lib.vmpc_ctx_get_cs_extension(ctx.handle, None) == nat.E_INVAL
    # the block restores what it found, also after an exception and inside another block
    with pytest.raises(RuntimeError, match="left by an exception"):
        with vm.device.cs_extension("auto"):
            assert ctx.get_cs_extension() == 1
            raise RuntimeError("left by an exception")
    assert ctx.get_cs_extension() == 0
    with vm.device.cs_extension("ntt"):
        with vm.device.cs_extension("direct"):
            assert ctx.get_cs_extension() == 0
        assert ctx.get_cs_extension() == 2
    assert ctx.get_cs_extension() == 0
    with pytest.raises(ValueError):
        with vm.device.cs_extension("fft"):
            pass
    assert ctx.get_cs_extension() == 0
    # the transform length, and where the direct kernel is taken whatever the mode
    ms = [0, 1, 2, 3, 1023, 1024, (1 << 20) - 1, 1 << 20]
    assert [ctx.cs_extend_ntt_len(m) for m in ms] == [0, 0, 8, 8, 2048, 4096, 1 << 21, 0]
    assert ctx.cs_extend_ntt_len(MAX_M + 1) == 0
    # the constants of the header are the binding's
    header = open(os.path.join(ROOT, "include", "vmpc.h")).read()

    def macro(name):
        return int(re.search(r"#define %s \(?(?:\(size_t\))?(\d+)\)?\s" % name, header).group(1))
    assert (nat.CS_EXTENSION_DIRECT, nat.CS_EXTENSION_AUTO, nat.CS_EXTENSION_NTT) == \
        (macro("VMPC_CS_EXTENSION_DIRECT"), macro("VMPC_CS_EXTENSION_AUTO"), macro("VMPC_CS_EXTENSION_NTT")) == (0, 1, 2)
    assert nat.FR_CS_EXT_NTT_MIN == macro("VMPC_FR_CS_EXT_NTT_MIN")
    # the arena a call reserves: the direct figure in the default mode, more under "ntt", the direct one again where
    # the direct kernel is taken anyway
    direct = ctx.cs_extend_batch_bytes(1000, 4)
    assert direct == lib.vmpc_fr_cs_extend_batch_bytes(1000, 4)
    with vm.device.cs_extension("ntt"):
        assert ctx.cs_extend_batch_bytes(1000, 4) > direct
        assert ctx.cs_extend_batch_bytes(1, 4) == lib.vmpc_fr_cs_extend_batch_bytes(1, 4)
        assert ctx.cs_extend_batch_bytes(MAX_M, 1) == lib.vmpc_fr_cs_extend_batch_bytes(MAX_M, 1)
        assert ctx.cs_extend_batch_bytes(MAX_M + 1, 1) == 0 and ctx.cs_extend_batch_bytes(8, 0) == 0


# ---- arena independence -----------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_arena(vm):
    """the means of tests/test_gpu_arena_independence.py: a fresh context, then the whole arena filled with 0, 1 and
    0x0100 (nothing above 0xFFFF) before the same call"""
    nat = vm._native
    m = 1025
    a, b, want = case(m, "random")
    c = nat.Context(0)
    try:
        c.set_cs_extension(nat.CS_EXTENSION_NTT)
        fact, ifact = (c.upload(_bytes(t)) for t in ref.tables(2 * m + 1))
        d_a, d_b = c.upload(_bytes(a)), c.upload(_bytes(b))

        def run():
            z = _pattern(c, 2 * m + 4)
            c.cs_extend(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, z.ptr)
            return _get(c, z, 2 * m + 4)
        fresh = run()
        size, used, gen = c.debug_arena_info()
        assert used > 18 * 4096 * 4 * 3                 # the residues are in the arena
        assert [fresh[p] for p in _written(m)] == [want[p] for p in _written(m)]
        for word in (0, 1, 0x0100):
            c.debug_arena_fill(word)
            got = run()
            assert c.debug_arena_info() == (size, used, gen), word      # over the arena that was filled
            assert got == fresh, word
    finally:
        c.close()
