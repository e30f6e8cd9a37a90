"""vmpc_bn256_fr_cs_extend_fg_dev reaches the scratch arena through cs_extend, the template tests/arena_cases.py already
names: its GF(n) share form over a dirty arena, by the states and helpers of tests/test_gpu_arena_independence.py -
fresh, the three fill words, and after a foreign call - on the direct route and on the NTT route."""
import random

import numpy as np
import pytest

from tests import arena_cases as A
from tests import mpc_koe_ref as mref
from tests import p8_field_ref as fref
from tests.test_gpu_arena_independence import FILLS, differs, nat, run_state  # noqa: F401  (nat: a fixture)

pytestmark = pytest.mark.gpu

N = fref.BN_N
F = fref.P8(N)
M_EXT = 600             # M = 601: three segments of CS_MIN_SEG = 256, three tiles - partial sums in the arena


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _inputs():
    rng = random.Random(4400)
    return [rng.randrange(N) for _ in range(M_EXT + 1)], [rng.randrange(N) for _ in range(M_EXT + 1)]


def _run(mode):
    def run(ctx):
        from verifiable_mpc_amd import device
        a, b = A.memo("p8bn_fg_inputs", _inputs)
        fact, ifact = (ctx.upload(_bytes(t)) for t in A.memo("p8bn_fg_tables", lambda: F.tables(2 * M_EXT + 1)))
        f, g = ctx.upload(np.zeros((M_EXT, 32), np.uint8)), ctx.upload(np.zeros((M_EXT, 32), np.uint8))
        d_a, d_b = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
        with device.cs_extension(mode, ctx):
            ctx.cs_extend_fg(d_a.ptr, d_b.ptr, M_EXT, fact.ptr, ifact.ptr, f.ptr, g.ptr, bn=True)
        ctx.sync()
        return ctx.download(f.ptr, 32 * M_EXT).tobytes() + ctx.download(g.ptr, 32 * M_EXT).tobytes()
    return run


def _want():
    a, b = A.memo("p8bn_fg_inputs", _inputs)
    return _bytes(mref.extend_fg(a) + mref.extend_fg(b)).tobytes()


SOURCE = "tests/test_gpu_p8_bn256_fg.py::test_direct_route_against_the_interpolating_polynomials"
CASES = [
    A.Case("bn_cs_extend_fg", [("circuit_sat.hip", "cs_extend")], SOURCE, "fr_dot", _run("direct"), _want),
    A.Case("bn_cs_extend_fg_ntt", [("circuit_sat.hip", "cs_extend")], SOURCE, "fr_dot", _run("ntt"), _want),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_result_does_not_depend_on_the_arena(nat, case):  # noqa: F811
    foreign = A.BY_NAME[case.foreign]
    ctx = nat.Context(0)
    try:
        results = {}
        results["fresh"], used = run_state(ctx, case, "fresh", may_grow=True)
        want = case.want()
        assert results["fresh"] == want, f"{case.name} / fresh: {differs(results['fresh'], want)}"
        for word in FILLS:
            ctx.debug_arena_fill(word)
            results[f"fill {word:#x}"], _ = run_state(ctx, case, f"fill {word:#x}")
        other, _ = run_state(ctx, foreign, "foreign (the other case)", may_grow=True)
        assert other == foreign.want()
        results["foreign"], _ = run_state(ctx, case, f"foreign ({foreign.name})")
        for state, got in results.items():
            assert got == results["fresh"], f"{case.name} / {state}: {differs(got, results['fresh'])} from the fresh run"
    finally:
        ctx.close()


def test_the_scale_kernel_takes_no_arena(nat):  # noqa: F811
    """vmpc_bn256_scale_points_dev: the arena is as it was (here: none at all)"""
    ctx = nat.Context(0)
    try:
        pts, sc, out = ctx.upload(np.zeros((70, 64), np.uint8)), ctx.upload(np.ones((70, 32), np.uint8)), ctx.alloc(64 * 70)
        ctx.bn256_scale_points(1, pts.ptr, sc.ptr, 70, out.ptr)
        ctx.sync()
        assert ctx.debug_arena_info() == (0, 0, 0)
        assert not ctx.download(out.ptr, 64 * 70).any()              # infinity in, infinity out
    finally:
        ctx.close()
