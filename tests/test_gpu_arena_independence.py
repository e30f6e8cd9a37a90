"""No entry point depends on what the scratch arena held (DESIGN.md "Arena independence"; the cases are
tests/arena_cases.py, one per function of csrc/ that reserves the arena).

Every public call carves its histograms, cursors, counters, flags and partial sums out of one arena per context that
never shrinks, is handed out again from offset 0 and is never cleared.  Each case runs on a fresh context in five arena
states and must give the oracle's bytes in all of them:
  fresh         the arena is allocated during this call
  fill 0, 1, 0x0100   the whole arena (and the prover's idle pool) filled with that 32-bit word first
                (vmpc_ctx_debug_arena_fill; never above 0xFFFF: a kernel that trusts a stale count or index then computes a
                wrong value, not a far address)
  foreign       another case of the table has just used the same arena
A state in which the arena was reallocated during the run (the fill thrown away) or the run took no arena memory proves
nothing: such a case is BLIND and fails.  After every run the short path's cursor words are zero (vmpc_ctx_debug_rearmed).

Shown to see something (EXPERIMENTS.md A.2: by hand on an MI355X, not committed), each mutation removing one zeroing of
a count that lives in the arena:
  - vmpc_bn256_validate_dev without the hipMemsetAsync of its offender counter: bn_validate fails in every state, the
    fresh one included - the case calls the entry four times on one context and the count of the first call is carried
    into the next; fill 1 and fill 0x0100 change the counts again (24 instead of 28 of 32 bytes differ).
  - k_sort_fine's sort_row_lb (csrc/msm_sort.hip) without `counts[...] = 0` for the top row's buckets that no digit of
    a canonical scalar reaches: ed_msm fails in fill 1 and fill 0x0100 and passes fresh, fill 0 and foreign (after
    ed_short); bn_msm fails in every state - its run is two commitments on one context, the second over the first's
    leftovers, and its 1.8-MB "fresh" arena was memory the allocator had recycled from an earlier context of the
    process.  The table passes, which do not go through that branch, and the short path pass, as they must.
37 tests, 4.5 s on an MI355X (the slowest case 0.75 s).  Freshly allocated arena memory: the 396-MB arena of the hook
test read back all zero beyond what the call wrote; small arenas are recycled memory and are not (above).  Neither is
asserted, and nothing may rely on it.
"""
import numpy as np
import pytest

from tests import arena_cases as A

pytestmark = pytest.mark.gpu

FILLS = (0, 1, 0x0100)
FILL_MAX = 0xFFFF


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


class Blind(AssertionError):
    pass


def run_state(ctx, case, state, may_grow=False):
    """one run of `case` over the arena as it is now -> (its bytes, the arena bytes its last call took); blind unless the
    arena it ran over is the one that was prepared (may_grow: the fresh run, and the OTHER case of the foreign state,
    which may need a larger arena than this context has) and the call took memory from it"""
    before = ctx.debug_arena_info()
    got = case.run(ctx)
    ctx.sync()
    size, used, gen = ctx.debug_arena_info()
    if not may_grow and gen != before[2]:
        raise Blind(f"{case.name} / {state}: the arena was reallocated during the run ({before} -> {(size, used, gen)}): "
                    "what had been prepared was thrown away")
    if used == 0:
        raise Blind(f"{case.name} / {state}: the run took no arena memory")
    assert ctx.debug_rearmed(), f"{case.name} / {state}: the short path's cursors were left non-zero"
    return got, used


def differs(got, want):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if len(a) != len(b):
        return f"{len(a)} bytes, expected {len(b)}"
    bad = np.flatnonzero(a != b)
    return f"{len(bad)} of {len(a)} bytes differ, the first at {int(bad[0])}"


@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_result_does_not_depend_on_the_arena(nat, case):
    foreign = A.BY_NAME[case.foreign]
    assert foreign is not case
    ctx = nat.Context(0)
    try:
        results = {}
        results["fresh"], used = run_state(ctx, case, "fresh", may_grow=True)
        want = case.want()
        if want is not None:                    # (None: the run itself judged its result - the prover's verifier)
            assert results["fresh"] == want, f"{case.name} / fresh: {differs(results['fresh'], want)}"
        for word in FILLS:
            ctx.debug_arena_fill(word)
            results[f"fill {word:#x}"], _ = run_state(ctx, case, f"fill {word:#x}")
        other, foreign_used = run_state(ctx, foreign, "foreign (the other case)", may_grow=True)
        assert foreign.want() is None or other == foreign.want()
        results["foreign"], _ = run_state(ctx, case, f"foreign ({foreign.name})")
        print(f"{case.name}: arena {ctx.debug_arena_info()[0]} bytes, takes {used}, after {foreign.name} which takes "
              f"{foreign_used}")
        for state, got in results.items():
            assert got == results["fresh"], f"{case.name} / {state}: {differs(got, results['fresh'])} from the fresh run"
    finally:
        ctx.close()


def arena_base(nat, ctx):
    """the arena's device address, right after a table commitment on the general path: such a call lays the sort's
    arrays out from the arena's first byte, the digit rows first (csrc/msm_sort.hip msm_layout), and vmpc_msm_sort_view
    names them"""
    import ctypes
    v = nat.SortView()
    nat._check(ctx.lib.vmpc_msm_sort_view(ctx.handle, ctypes.byref(v)), "vmpc_msm_sort_view")
    return int(v.digits)


def test_hooks(nat):
    import ctypes
    lib = nat.load_library()
    # a null context
    assert lib.vmpc_ctx_debug_arena_fill(None, 0) == nat.E_INVAL
    assert lib.vmpc_ctx_debug_arena_info(None, None, None, None) == nat.E_INVAL
    assert lib.vmpc_ctx_debug_rearmed(None, ctypes.byref(ctypes.c_int(0))) == nat.E_INVAL
    small, large = A.BY_NAME["fr_dot"], A.BY_NAME["ed_table_wide"]
    ctx = nat.Context(0)
    try:
        # no arena yet: nothing to fill, nothing queued; a short path that was never set up counts as re-armed
        assert ctx.debug_arena_info() == (0, 0, 0)
        ctx.debug_arena_fill(1)
        assert ctx.done() and ctx.debug_arena_info() == (0, 0, 0)
        assert ctx.debug_rearmed()
        # the generation: the first call allocates, the same call again leaves the arena alone, a larger call
        # reallocates it once, a smaller one after that leaves it alone
        for _ in range(2):
            assert small.run(ctx) == small.want()
            size, used, gen = ctx.debug_arena_info()
            assert size >= used > 0 and gen == 1
        assert large.run(ctx) == large.want()
        size2, used2, gen2 = ctx.debug_arena_info()
        assert gen2 == 2 and size2 > size and size2 >= used2 > used
        base = arena_base(nat, ctx)
        # (informational, EXPERIMENTS.md A.3: is freshly allocated arena memory zero where the call did not write?)
        tail = ctx.download(base + used2, min(size2 - used2, 8 << 20))
        print(f"fresh arena of {size2} bytes, beyond the {used2} the call took: "
              f"{'all zero' if not tail.any() else 'NOT all zero'} ({len(tail)} bytes read)")
        # the fill reaches the first and the last word; 0xFFFF is served, anything above is refused and fills nothing
        last = base + (size2 & ~3) - 4096
        ctx.debug_arena_fill(FILL_MAX)
        ctx.sync()
        # (one above the cap and no further: were the refusal broken, the arena would still hold a small value)
        with pytest.raises(nat.VmpcError) as ei:
            ctx.debug_arena_fill(FILL_MAX + 1)
        assert ei.value.code == nat.E_RANGE
        ctx.sync()
        for at in (base, base + used2 // 2 // 4 * 4, last):
            assert (ctx.download(at, 4096).view("<u4") == FILL_MAX).all(), at - base
        assert small.run(ctx) == small.want()
        assert ctx.debug_arena_info()[0::2] == (size2, 2)
        # while a prover round is held nothing may be queued between its kernels: the fill is refused (and so is the
        # synchronising read of the cursors), and what the stream was doing comes out intact
        a, b, want = A._dot_inputs()
        da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(32)
        ctx.debug_arena_fill(0)
        ctx.fr_dot_into(da.ptr, db.ptr, A.DOT_N, out.ptr)          # queued, its partial sums in the arena
        lib.vmpc_ctx_debug_hold_wait(ctx.handle, 1)
        try:
            with pytest.raises(nat.VmpcError) as ei:
                ctx.debug_arena_fill(1)
            assert ei.value.code == nat.E_INVAL
            with pytest.raises(nat.VmpcError) as ei:
                ctx.debug_rearmed()
            assert ei.value.code == nat.E_INVAL
        finally:
            lib.vmpc_ctx_debug_hold_wait(ctx.handle, 0)
        assert A.get(ctx, out, 32) == want
    finally:
        ctx.close()


# tests/test_gpu_short_path.py test_short_path_exponent_identity_and_general_path, lg = 16, "bits": 2^15 entries and
# more in ONE bucket, beyond the fused path's fixed capacities
def test_short_path_overflow_rearms_its_cursors(nat):
    import random
    from oracle import ed25519_ref as ed
    from tests.test_gpu_cabi import gpu_points, sc_bytes
    from tests.test_gpu_short_path import ran_short
    n = (1 << 16) - 3
    rng = random.Random(16)
    exps = [rng.randrange(1, ed.ELL) for _ in range(n + 2)]
    bits = [rng.randrange(2) for _ in range(n)]
    uniform = [rng.randrange(ed.ELL) for _ in range(n)]
    gam = [rng.randrange(ed.ELL), rng.randrange(ed.ELL)]
    want = {name: A.ed_exp_point(A.ed_dot(x, exps) + gam[0] * exps[n] + gam[1] * exps[n + 1])
            for name, x in (("bits", bits), ("uniform", uniform))}
    ctx = nat.Context(0)
    try:
        pts = gpu_points(nat, ctx, exps)
        table = ctx.msm_table_build(pts.ptr, n, pts.ptr + 64 * n, 2, 16)
        dg, out = ctx.upload(sc_bytes(nat, gam)), ctx.alloc(128)
        d_bits, d_uni = ctx.upload(sc_bytes(nat, bits)), ctx.upload(sc_bytes(nat, uniform))

        def launch(ds):
            ctx.msm_table(table.ptr, n, 2, ds.ptr, n, dg.ptr, out.ptr, None, 16)
        launch(d_bits)
        with pytest.raises(nat.VmpcError) as ei:
            ctx.sync()
        assert ei.value.code == nat.E_AGAIN
        assert ctx.debug_rearmed(), "the overflowing call left its cursors"
        ctx.on_general_path(lambda: (launch(d_bits), ctx.sync()))
        assert A.ed_ext_canon(A.get(ctx, out, 128)) == want["bits"]
        assert ctx.debug_rearmed()
        # the next short-path call on this context, over an arena of ones
        ctx.set_short_path(True, forget_overflow=True)
        before = ctx.debug_arena_info()
        ctx.debug_arena_fill(1)
        assert ran_short(ctx, lambda: launch(d_uni))
        assert A.ed_ext_canon(A.get(ctx, out, 128)) == want["uniform"]
        size, used, gen = ctx.debug_arena_info()
        assert gen == before[2] and used > 0
        assert ctx.debug_rearmed()
    finally:
        ctx.close()
