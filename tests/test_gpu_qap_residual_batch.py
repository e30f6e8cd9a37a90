"""vmpc_bn256_qap_residual_batch_dev (csrc/bn256_qap_h.hip): out[w] = sum_j rho^j (a_w[j] b_w[j] -
y_w[j]) for n_wit rows under one rho, against tests/trinocchio_ref.py's residual on Python ints and byte for byte
against n_wit calls of the single entry (which is the batch entry with one witness).  d at the edges of a workgroup's
256 rows and past the 64 x 256 rows beyond which lanes share rows; rows a || b || y packed and 7 scalars apart with a
padding of values >= n that must not be read; rows of full-size residues, of n - 1 and of zeros; rho 0, 1 and random."""
import ctypes
import functools
import random

import numpy as np
import pytest

from tests import keygen_ref as K
from tests import trinocchio_ref as tr

pytestmark = pytest.mark.gpu
N = tr.N
MAX_WIT = 5
RHOS = [0, 1, random.Random(99).randrange(2, N)]


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as v
    return v.get_context()


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _rows(d):
    """MAX_WIT rows (a, b, y): random, zeros, every operand n - 1, random twice -> (rows, want[rho index][w]); made once"""
    rng = random.Random(d)
    draw = lambda: [rng.randrange(N) for _ in range(d)]
    rows = [(draw(), draw(), draw()), ([0] * d,) * 3, ([N - 1] * d,) * 3, (draw(), draw(), draw()), (draw(), draw(), draw())]
    return rows, [[tr.residual(a, b, y, rho) for a, b, y in rows] for rho in RHOS]


def _ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


@pytest.mark.parametrize("d", [1, 2, 255, 256, 257, 16385])
def test_batch_against_the_reference_and_the_single_entry(ctx, d):
    rows, want = _rows(d)
    packed = [K.to_array(a + b + y) for a, b, y in rows]
    single = []
    for r, rho in enumerate(RHOS):
        outs = []
        for w in range(MAX_WIT):
            buf, out = ctx.upload(packed[w]), ctx.alloc(32)
            ctx.bn256_qap_residual(buf.ptr, buf.ptr + 32 * d, buf.ptr + 64 * d, d, rho, out.ptr)
            ctx.sync()
            outs.append(ctx.download(out.ptr, 32).tobytes())
        assert [int.from_bytes(o, "little") for o in outs] == want[r], rho
        single.append(outs)
    for n_wit in (1, 2, MAX_WIT):
        for stride in (3 * d, 3 * d + 7):
            host = np.full((n_wit, stride, 32), 0xFF, np.uint8)              # the padding: 2^256 - 1 >= n
            for w in range(n_wit):
                host[w, :3 * d] = packed[w]
            buf = ctx.upload(host)
            for r, rho in enumerate(RHOS):
                out = ctx.upload(np.full((n_wit + 1, 32), 0x5A, np.uint8))
                ctx.bn256_qap_residual_batch(buf.ptr, buf.ptr + 32 * d, buf.ptr + 64 * d, stride, d, rho, out.ptr, n_wit)
                ctx.sync()
                got = ctx.download(out.ptr, 32 * (n_wit + 1), (n_wit + 1, 32))
                assert _ints(got[:n_wit]) == want[r][:n_wit], (n_wit, stride, rho)
                assert [g.tobytes() for g in got[:n_wit]] == single[r][:n_wit]
                assert (got[n_wit] == 0x5A).all()


def test_argument_rules(ctx, nat):
    f, h = ctx.lib.vmpc_bn256_qap_residual_batch_dev, ctx.handle
    p = ctypes.c_void_p
    rho = ctypes.create_string_buffer((5).to_bytes(32, "little"), 32)
    rho_n = ctypes.create_string_buffer(N.to_bytes(32, "little"), 32)
    x = ctx.upload(K.to_array([1] * 12))
    # (a, b, y, stride, d, rho, out, n_wit): VMPC_E_RANGE before any pointer is looked at
    assert f(h, None, None, None, 3, 1, rho, None, nat.BN256_QAP_MAX_WIT + 1) == nat.E_RANGE
    assert f(h, None, None, None, (1 << 31) + 1, 1, rho, None, 2) == nat.E_RANGE
    assert f(h, None, None, None, 3, 1 << 20, rho, None, 2) == nat.E_RANGE
    assert f(h, None, None, None, 1, 2, rho, None, 2) == nat.E_RANGE             # stride < d
    assert f(h, p(x.ptr), p(x.ptr + 32), p(x.ptr + 64), 3, 1, rho_n, p(x.ptr + 96), 2) == nat.E_NONCANON
    with pytest.raises(nat.VmpcError) as e:
        ctx.bn256_qap_residual_batch(x.ptr, x.ptr + 32, x.ptr + 64, 3, 1, N, x.ptr + 96, 2)
    assert e.value.code == nat.E_NONCANON
    assert f(h, None, p(x.ptr), p(x.ptr), 3, 1, rho, p(x.ptr), 2) == nat.E_INVAL
    assert f(h, p(x.ptr), p(x.ptr), p(x.ptr), 3, 1, None, p(x.ptr), 2) == nat.E_INVAL
    assert f(h, p(x.ptr), p(x.ptr), p(x.ptr), 3, 0, rho, p(x.ptr), 2) == nat.E_INVAL         # d = 0
    ctx.profile(True)
    try:
        ctx.profile_read()
        assert f(h, p(x.ptr), p(x.ptr), p(x.ptr), 3, 1, rho, p(x.ptr), 0) == nat.OK          # no witness: no launch
        ctx.sync()
        assert all(count == 0 for _, count in ctx.profile_read().values())
    finally:
        ctx.profile(False)
