"""The GF(n) entries of Protocol 8 that reach the scratch arena do so through templates that tests/arena_cases.py already
names (cs_extend, fr_colsum, koe_poly_mul / vmpc_ntt_poly_mul): their GF(n) instantiations over a dirty arena, by the
states and helpers of tests/test_gpu_arena_independence.py - fresh, the three fill words, and after a foreign call.
The entries that take their scratch from the caller (tables, lagrange, dot) never touch the arena and have no case."""
import random

import numpy as np
import pytest

from tests import arena_cases as A
from tests import p8_field_ref as fref
from tests.test_gpu_arena_independence import FILLS, differs, nat, run_state  # noqa: F401  (nat: a fixture)

pytestmark = pytest.mark.gpu

N = fref.BN_N
F = fref.P8(N)
M_EXT = 600             # M = 601: three segments of CS_MIN_SEG = 256, three tiles - partial sums in the arena
N_KOE = 700             # operands of 701 and 700 coefficients: tiles of more than one segment of KOE_MIN_SEG = 256


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _ext_inputs():
    rng = random.Random(4100)
    return [rng.randrange(N) for _ in range(M_EXT + 1)], [rng.randrange(N) for _ in range(M_EXT + 1)]


def _extend_run(mode):
    def run(ctx):
        from verifiable_mpc_amd import device
        a, b = A.memo("p8bn_ext_inputs", _ext_inputs)
        fact, ifact = (ctx.upload(_bytes(t)) for t in A.memo("p8bn_tables", lambda: F.tables(2 * M_EXT + 1)))
        z, d_a, d_b = ctx.upload(np.zeros((2 * M_EXT + 3, 32), np.uint8)), ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
        with device.cs_extension(mode, ctx):
            ctx.cs_extend(d_a.ptr, d_b.ptr, M_EXT, fact.ptr, ifact.ptr, z.ptr, bn=True)
        ctx.sync()
        return ctx.download(z.ptr, 32 * (2 * M_EXT + 3)).tobytes()
    return run


def _extend_want():
    a, b = A.memo("p8bn_ext_inputs", _ext_inputs)
    tail = F.z_tail_bary(a[:M_EXT], b[:M_EXT], a[M_EXT], b[M_EXT])
    tail[3:3 + M_EXT] = [0] * M_EXT                 # the gammas' places are not the entry's: the zeros uploaded
    return _bytes(tail).tobytes()


def _colsum_inputs():
    rng = random.Random(4200)
    n_rows = 500
    entries = [(0, r, rng.randrange(1, N)) for r in range(n_rows)] + [(1, r, N - 1) for r in range(130)] + \
              [(2, 7, rng.randrange(1, N))]
    return n_rows, entries, [rng.randrange(N) for _ in range(n_rows)]


def _colsum_run(ctx):
    from verifiable_mpc_amd import sparse
    n_rows, entries, weights = A.memo("p8bn_colsum_inputs", _colsum_inputs)
    plan = sparse.ColumnPlan(ctx, np.array([e[0] for e in entries], np.int64), np.array([e[1] for e in entries], np.int64),
                             _bytes([e[2] for e in entries]), 3, dst=[4, 0, 2], field="bn256_cs")
    assert plan.n_partial > 0
    out, d_w = ctx.upload(np.full((5, 32), 0xA5, np.uint8)), ctx.upload(_bytes(weights))
    plan.run(d_w.ptr, n_rows, out.ptr, 5)
    ctx.sync()
    return ctx.download(out.ptr, 32 * 5).tobytes()


def _colsum_want():
    _, entries, weights = A.memo("p8bn_colsum_inputs", _colsum_inputs)
    want, dst = [0] * 5, [4, 0, 2]
    for c, r, v in entries:
        want[dst[c]] = (want[dst[c]] + v * weights[r]) % N
    return _bytes(want).tobytes()


def _koe_inputs():
    rng = random.Random(4300)
    return [rng.randrange(N) for _ in range(N_KOE)], [rng.randrange(N) for _ in range(N_KOE)], rng.randrange(1, N)


def _koe_run(mode):
    def run(ctx):
        """the opening's scalar side as knowledge_of_exponent.opening_linear_form_prover runs it on device operands:
        stage, product, split -> c with c[n] zeroed, then u"""
        from verifiable_mpc_amd import device
        x, L, gamma = A.memo("p8bn_koe_inputs", _koe_inputs)
        n = N_KOE
        lhs, rhs, c, u = ctx.alloc(32 * (n + 1)), ctx.alloc(32 * n), ctx.alloc(32 * 2 * n), ctx.alloc(32)
        d_x, d_L = ctx.upload(_bytes(x)), ctx.upload(_bytes(L))
        ctx.bn256_koe_stage(d_x.ptr, gamma, d_L.ptr, n, lhs.ptr, rhs.ptr)
        with device.poly_product(mode, ctx):
            ctx.bn256_fr_poly_mul(lhs.ptr, n + 1, rhs.ptr, n, c.ptr)
        ctx.bn256_koe_split(c.ptr, n, u.ptr)
        ctx.sync()
        return ctx.download(c.ptr, 32 * 2 * n).tobytes() + ctx.download(u.ptr, 32).tobytes()
    return run


def _koe_want():
    x, L, gamma = A.memo("p8bn_koe_inputs", _koe_inputs)
    c = fref.KoeTrapdoor(1, 1, 1).product(L, x, gamma)
    u, c[N_KOE] = c[N_KOE], 0
    return _bytes(c + [u]).tobytes()


SOURCE = "tests/test_gpu_p8_bn256_primitives.py::test_extension_direct"
CASES = [
    A.Case("bn_cs_extend", [("circuit_sat.hip", "cs_extend")], SOURCE, "fr_dot", _extend_run("direct"), _extend_want),
    A.Case("bn_cs_extend_ntt", [("circuit_sat.hip", "cs_extend")], SOURCE, "fr_dot", _extend_run("ntt"), _extend_want),
    A.Case("bn_cs_colsum", [("fr_colsum.h", "fr_colsum")], SOURCE, "fr_dot", _colsum_run, _colsum_want),
    A.Case("bn_koe_opening", [("bn256_koe.hip", "koe_poly_mul")], SOURCE, "fr_dot", _koe_run("schoolbook"), _koe_want),
    A.Case("bn_koe_opening_ntt", [("bn256_ntt.hip", "vmpc_ntt_poly_mul")], SOURCE, "fr_dot", _koe_run("ntt"), _koe_want),
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


def test_the_caller_scratch_entries_take_no_arena(nat):  # noqa: F811
    """tables, lagrange and the dot product over GF(n): the arena is as it was (here: none at all)"""
    ctx = nat.Context(0)
    try:
        K = 300
        fact, ifact, lam, out = (ctx.alloc(32 * (K + 1)) for _ in range(4))
        ctx.cs_tables(K, fact.ptr, ifact.ptr, bn=True)
        ctx.cs_lagrange(N - 1, K, ifact.ptr, lam.ptr, bn=True)
        ctx.fr_dot_into(lam.ptr, fact.ptr, K + 1, out.ptr, bn=True)
        ctx.sync()
        assert ctx.debug_arena_info() == (0, 0, 0)
    finally:
        ctx.close()
