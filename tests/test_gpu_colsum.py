"""The column sum of csrc/fr_colsum.h through both of its entry points (vmpc_bn256_qap_colsum_dev over GF(n),
vmpc_fr_cs_colsum_dev over GF(l)): ONE plan of sparse.colsum_plan, each field's own values, against Python sums.  Exact."""
import numpy as np
import pytest

from oracle import bn256_ref as bn
from oracle import ed25519_ref as ed

pytestmark = pytest.mark.gpu

N_ROWS, N_OUT = 300, 40
WORST = 4                                   # the column whose 64 products are all (modulus - 1)^2
# an empty column, 64 and 65 entries, more than 256 partials for the finish kernel's stride loop, the worst case, short
LENS = [0, 64, 65, 64 * 256 + 1, 64, 1, 130, 0, 7]
DST = [3, 0, 17, 5, 39, 8, 21, 30, 2]       # scattered into N_OUT positions, gaps between them
EMPTY_AT = 11                               # an item without entries (what colsum_plan makes of an empty column without dst)


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as vm
    return vm.get_context()


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _ints(a):
    raw = a.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.fixture(scope="module")
def plan(ctx):
    from verifiable_mpc_amd import sparse
    rng = np.random.default_rng(5)
    col_ptr = np.concatenate([[0], np.cumsum(LENS)])
    rows = rng.integers(0, N_ROWS + 40, size=col_ptr[-1])      # rows >= N_ROWS add nothing
    rows[col_ptr[WORST]:col_ptr[WORST + 1]] = np.arange(64)
    items, longs, n_partial = sparse.colsum_plan(col_ptr, DST)
    assert n_partial > 256
    items = np.vstack([items, np.array([[5, 5, EMPTY_AT]], np.uint32)])
    return {"col_ptr": col_ptr, "rows": rows, "d_rows": ctx.upload(rows.astype(np.uint32)), "items": ctx.upload(items),
            "n_items": len(items), "longs": ctx.upload(longs), "n_long": len(longs), "n_partial": n_partial}


@pytest.mark.parametrize("entry,order", [("bn256_qap_colsum", bn.N), ("cs_colsum", ed.ELL)])
def test_one_plan_through_both_fields(ctx, plan, entry, order):
    import random
    rng = random.Random(order)
    nnz, col_ptr, rows = len(plan["rows"]), plan["col_ptr"], plan["rows"]
    vals = [rng.randrange(order) for _ in range(nnz)]
    weights = [rng.randrange(order) for _ in range(N_ROWS)]
    vals[col_ptr[WORST]:col_ptr[WORST + 1]] = [order - 1] * 64
    weights[:64] = [order - 1] * 64
    # positions that no item writes: Protocol 8's entry zero-fills them, key generation's leaves them alone
    untouched = 0 if entry == "cs_colsum" else 7
    want = [untouched] * N_OUT
    for c, d in enumerate(DST):
        if LENS[c]:                         # with a dst an empty column has no item
            want[d] = sum(vals[e] * weights[rows[e]] for e in range(col_ptr[c], col_ptr[c + 1]) if rows[e] < N_ROWS) % order
    want[EMPTY_AT] = 0                      # the item without entries writes 0
    d_vals, d_w = ctx.upload(_bytes(vals)), ctx.upload(_bytes(weights))
    out = ctx.upload(_bytes([7] * N_OUT))
    run = getattr(ctx, entry)
    run(d_w.ptr, N_ROWS, plan["d_rows"].ptr, d_vals.ptr, nnz, plan["items"].ptr, plan["n_items"], plan["longs"].ptr,
        plan["n_long"], plan["n_partial"], out.ptr, N_OUT)
    ctx.sync()
    assert _ints(ctx.download(out.ptr, 32 * N_OUT)) == want
    assert want[DST[WORST]] != 0
    # no columns at all: nothing is launched; Protocol 8's entry still zero-fills
    ctx.upload_into(out.ptr, _bytes([7] * N_OUT))
    run(d_w.ptr, N_ROWS, plan["d_rows"].ptr, d_vals.ptr, 0, plan["items"].ptr, 0, plan["longs"].ptr, 0, 0, out.ptr, N_OUT)
    ctx.sync()
    assert _ints(ctx.download(out.ptr, 32 * N_OUT)) == [untouched] * N_OUT
