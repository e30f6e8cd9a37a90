"""The GF(n) entries of Protocol 8 (csrc/circuit_sat.hip, csrc/frvec.hip, csrc/bn256_koe.hip instantiated at the BN-256
scalar field) one entry point at a time, against tests/p8_field_ref.py at p = n.  Every comparison is exact.

The shapes stand for the kernels' constants, restated here: CS_RUN = 32 (sequence elements per scan lane), CS_WG = 256,
one scanning workgroup takes 256 lanes = 8192 elements before a thread owns two runs, FR_CONV_CHUNK = 64 (elements of u
staged per step), CS_MIN_SEG = 256 (shortest segment of j), FR_BLOCK = 256 (the vector kernels' workgroup).
What differs from GF(l) is what is looked at hardest: n fills 256 bits, so a sum of two residues carries out of eight
limbs (values n - 1 everywhere), a 32-byte word may be >= n (reduced when it is loaded), and PAT, the fill of untouched
memory, is such a word.
"""
import ctypes
import random

import numpy as np
import pytest

from tests import p8_field_ref as fref

pytestmark = pytest.mark.gpu

N = fref.BN_N
F = fref.P8(N)
MAX_M = 1 << 20                             # VMPC_FR_CS_MAX_M of include/vmpc.h
PAT_BYTE = 0xA5
PAT = int.from_bytes(bytes([PAT_BYTE]) * 32, "little")      # above n: no kernel here can write it
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as vm
    return vm.get_context()


def _bytes(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32)


def _ints(a):
    raw = a.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _pattern(ctx, n):
    return ctx.upload(np.full((max(n, 1), 32), PAT_BYTE, np.uint8))


def _get(ctx, buf, n):
    ctx.sync()
    return _ints(ctx.download(buf.ptr, 32 * n))


def test_pat_is_not_a_residue():
    assert N <= PAT < 1 << 256


# ---- tables and Lagrange vectors ------------------------------------------------------------------------------------------
SCAN_K = [1, 2, 31, 32, 33, 255, 256, 257, 8193]


@pytest.fixture(scope="module")
def tables(ctx):
    """K -> (device fact, device ifact, host fact, host ifact), made once by the entry under test"""
    out = {}
    for K in SCAN_K:
        fact, ifact = _pattern(ctx, K + 2), _pattern(ctx, K + 2)
        ctx.cs_tables(K, fact.ptr, ifact.ptr, bn=True)
        out[K] = (fact, ifact, _get(ctx, fact, K + 2), _get(ctx, ifact, K + 2))
    return out


@pytest.mark.parametrize("K", SCAN_K)
def test_factorial_tables(tables, K):
    _, _, got_f, got_i = tables[K]
    assert got_f[K + 1] == PAT and got_i[K + 1] == PAT
    want_f, want_i = F.tables(K)
    assert got_f[:K + 1] == want_f
    assert got_i[:K + 1] == want_i
    assert all(f * i % N == 1 for f, i in zip(got_f[:K + 1], got_i[:K + 1]))


@pytest.mark.parametrize("K", SCAN_K)
def test_lagrange_vector(ctx, tables, K):
    ifact = tables[K][1]
    rng = random.Random(7100 + K)
    for c in (rng.randrange(K + 1, N), N - 1, K // 2, K):          # random, the largest residue, two nodes
        out = _pattern(ctx, K + 2)
        ctx.cs_lagrange(c, K, ifact.ptr, out.ptr, bn=True)
        got = _get(ctx, out, K + 2)
        assert got[K + 1] == PAT, c
        lam = got[:K + 1]
        assert lam == F.lagrange_bary(K, c), c
        if c <= K:
            assert lam == [int(j == c) for j in range(K + 1)], c
        else:
            assert sum(lam) % N == 1, c
            assert sum(v * pow(j, K, N) for j, v in enumerate(lam)) % N == pow(c, K, N), c
            if K <= 33:
                assert lam == F.lagrange_naive(K, c), c


# ---- extension --------------------------------------------------------------------------------------------------------------
EXTEND_M = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000]
NTT_M = [2, 3, 64, 65, 1000, 4096]


def _extend_inputs(m, kind="random"):
    rng = random.Random(9100 + m)
    M = m + 1
    if kind == "top":                   # every value n - 1: sums that carry out of 256 bits, the largest products
        return [N - 1] * M, [N - 1] * M
    return [rng.randrange(N) for _ in range(M)], [rng.randrange(N) for _ in range(M)]


@pytest.fixture(scope="module")
def extend_want():
    """m -> the CPU's z tail for the random inputs: once, shared by the direct and the NTT test (m <= 1000: O(m^2))"""
    out = {}
    for m in sorted(set(EXTEND_M + [m for m in NTT_M if m <= 1000])):
        a, b = _extend_inputs(m)
        out[m] = F.z_tail_bary(a[:m], b[:m], a[m], b[m])
    return out


def _extend(ctx, m, a, b, mode):
    from verifiable_mpc_amd import device
    K = max(2 * m + 1, 1)
    fact, ifact = (ctx.upload(_bytes(t)) for t in F.tables(K))     # host tables: a wrong element is the extension's own
    d_a, d_b = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
    z = _pattern(ctx, 2 * m + 4)
    with device.cs_extension(mode, ctx):
        ctx.cs_extend(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, z.ptr, bn=True)
    return _get(ctx, z, 2 * m + 4)


def _written(m):
    return [0, 1, 2] + ([2 + m + 1] if m else []) + [2 + x for x in range(m + 2, 2 * m + 1)]


@pytest.mark.parametrize("m", EXTEND_M)
def test_extension_direct(ctx, extend_want, m):
    a, b = _extend_inputs(m)
    got, want, n_z = _extend(ctx, m, a, b, "direct"), extend_want[m], 2 * m + 3
    assert len(want) == n_z
    assert [got[p] for p in _written(m)] == [want[p] for p in _written(m)]
    assert got[3:3 + m] == [PAT] * m and got[n_z] == PAT          # the gammas' places and the end are not the entry's
    if m <= 8:
        naive = F.z_tail_naive(a[:m], b[:m], a[m], b[m])
        assert [got[p] for p in _written(m)] == [naive[p] for p in _written(m)]


@pytest.mark.parametrize("m", [3, 65, 257])
def test_extension_at_the_largest_residues(ctx, m):
    a, b = _extend_inputs(m, "top")
    got, want = _extend(ctx, m, a, b, "direct"), F.z_tail_bary(a[:m], b[:m], a[m], b[m])
    assert [got[p] for p in _written(m)] == [want[p] for p in _written(m)]
    assert _extend(ctx, m, a, b, "ntt") == got


@pytest.mark.parametrize("m", NTT_M)
def test_extension_by_ntt_is_the_direct_kernel_bit_for_bit(ctx, extend_want, m):
    assert ctx.cs_extend_ntt_len(m) > 0
    a, b = _extend_inputs(m)
    direct, ntt = _extend(ctx, m, a, b, "direct"), _extend(ctx, m, a, b, "ntt")
    assert ntt == direct
    assert all(v < N for p, v in enumerate(ntt) if p in set(_written(m)))
    if m <= 1000:
        assert [ntt[p] for p in _written(m)] == [extend_want[m][p] for p in _written(m)]


# ---- triples ----------------------------------------------------------------------------------------------------------------
N_X, G_OFF, M_GATES = 7, 7 + 8, 600
LEVELS = [(0, 257), (257, 513), (513, 600)]          # 257, 256 and 87 gates: a second workgroup of one lane, a full one
N_Z = G_OFF + M_GATES + 3


def _circuit():
    rng = random.Random(610)
    A, B = [None] * M_GATES, [None] * M_GATES

    def row(limit):
        e = [(rng.randrange(limit), rng.choice([rng.randrange(1, N), N - 1, rng.randrange(1, 5)]))
             for _ in range(rng.randrange(1, 5))]
        return (e, rng.randrange(N) if rng.random() < 0.5 else 0)

    for lo, hi in LEVELS:
        for i in range(lo, hi):
            A[i], B[i] = row(N_X + lo), row(N_X + lo)
    A[3] = ([], rng.randrange(1, N))                                  # a constant wire
    A[550] = ([(c, N - 1) for c in range(N_X)] + [(N_X + g, N - 1) for g in range(293)], N - 1)   # 300 entries
    return A, B


def _csr(ctx, rows):
    ptr, col, vals, consts = [0], [], [], []
    for e, k in rows:
        for c, v in e:
            col.append(c)
            vals.append(v)
        ptr.append(len(col))
        consts.append(k)
    keep = [ctx.upload(np.array(ptr, np.uint32)), ctx.upload(np.array(col, np.uint32)), ctx.upload(_bytes(vals)),
            ctx.upload(_bytes(consts))]
    return keep, tuple(b.ptr for b in keep)


@pytest.fixture(scope="module")
def circuit(ctx):
    A, B = _circuit()
    rng = random.Random(611)
    gates = []
    for lo, hi in LEVELS:
        order = list(range(lo, hi))
        rng.shuffle(order)
        gates += order
    x = [rng.randrange(N) for _ in range(N_X - 1)] + [N - 1]
    keep_a, csr_a = _csr(ctx, A)
    keep_b, csr_b = _csr(ctx, B)
    return {"A": A, "B": B, "csr_a": csr_a, "csr_b": csr_b, "keep": (keep_a, keep_b), "x": x,
            "want": F.triples(N_X, A, B, x), "gates": ctx.upload(np.array(gates, np.uint32))}


def _z_image(x, gamma):
    return x + [PAT] * (G_OFF - N_X) + gamma + [PAT] * (N_Z - G_OFF - M_GATES)


def test_triples_level_by_level(ctx, circuit):
    x, (a, b, gamma) = circuit["x"], circuit["want"]
    z = ctx.upload(_bytes(_z_image(x, [PAT] * M_GATES)))
    a_out, b_out = _pattern(ctx, M_GATES + 1), _pattern(ctx, M_GATES + 1)
    for i, (lo, hi) in enumerate(LEVELS):
        ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], circuit["gates"].ptr + 4 * lo, hi - lo, N_X, G_OFF, z.ptr,
                       a_out.ptr, b_out.ptr, bn=True)
        assert _get(ctx, z, N_Z) == _z_image(x, gamma[:hi] + [PAT] * (M_GATES - hi)), i
        assert _get(ctx, a_out, M_GATES + 1) == a[:hi] + [PAT] * (M_GATES + 1 - hi), i
        assert _get(ctx, b_out, M_GATES + 1) == b[:hi] + [PAT] * (M_GATES + 1 - hi), i


@pytest.mark.parametrize("spoiled,first", [((), NONE), ((599, 300, 256, 255), 255), ((599,), 599)],
                         ids=["none", "four", "last"])
def test_triples_check_names_the_smallest_bad_gate(ctx, circuit, spoiled, first):
    x, (a, b, gamma) = circuit["x"], circuit["want"]
    gamma = list(gamma)
    for i in spoiled:
        gamma[i] = (gamma[i] + 1) % N
    image = _z_image(x, gamma)
    z = ctx.upload(_bytes(image))
    a_out, b_out, bad = _pattern(ctx, M_GATES), _pattern(ctx, M_GATES), ctx.upload(np.array([7], np.uint32))
    ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], None, M_GATES, N_X, G_OFF, z.ptr, a_out.ptr, b_out.ptr, 1, bad.ptr,
                   bn=True)
    ctx.sync()
    assert int(ctx.download(bad.ptr, 4).view(np.uint32)[0]) == first
    assert _get(ctx, z, N_Z) == image           # the gammas are the caller's: nothing is written to z


def test_triples_values_only(ctx, circuit):
    x, (a, b, gamma) = circuit["x"], circuit["want"]
    image = _z_image(x, gamma)
    z, out = ctx.upload(_bytes(image)), _pattern(ctx, M_GATES + 1)
    ctx.cs_triples(circuit["csr_a"], circuit["csr_a"], None, M_GATES, N_X, G_OFF, z.ptr, out.ptr, out.ptr, 2, None, bn=True)
    assert _get(ctx, out, M_GATES + 1) == a + [PAT]
    assert _get(ctx, z, N_Z) == image


def test_triples_reduce_words_above_n_when_they_load_them(ctx, circuit):
    """x_i + n where that fits 256 bits stands for x_i: the same a, b, gamma"""
    x, (a, b, gamma) = circuit["x"], circuit["want"]
    raised = [v + N if v + N < 1 << 256 else v for v in x]
    assert raised != x
    z = ctx.upload(_bytes(_z_image(raised, [PAT] * M_GATES)))
    a_out, b_out = _pattern(ctx, M_GATES), _pattern(ctx, M_GATES)
    for lo, hi in LEVELS:
        ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], circuit["gates"].ptr + 4 * lo, hi - lo, N_X, G_OFF, z.ptr,
                       a_out.ptr, b_out.ptr, bn=True)
    assert _get(ctx, z, N_Z)[G_OFF:G_OFF + M_GATES] == gamma and _get(ctx, a_out, M_GATES) == a


# ---- column sums ------------------------------------------------------------------------------------------------------------
def test_colsum_empty_long_and_duplicate_columns(ctx):
    from verifiable_mpc_amd import sparse
    rng = random.Random(77)
    n_rows, n_cols, n_out = 300, 6, 9
    entries = []                                    # (col, row, value)
    entries += [(0, r, rng.randrange(1, N)) for r in rng.sample(range(n_rows), 5)]
    # column 1: empty.  column 2: 200 entries, more than the 64 of one item.  column 3: one row three times
    entries += [(2, r, rng.choice([N - 1, rng.randrange(1, N)])) for r in range(200)]
    entries += [(3, 17, rng.randrange(1, N)) for _ in range(3)]
    entries += [(4, r, N - 1) for r in range(64)]                   # exactly one full item
    entries += [(5, r, rng.randrange(1, N)) for r in range(65)]     # one more than that
    weights = [rng.choice([N - 1, rng.randrange(N)]) for _ in range(n_rows)]
    dst = [8, 1, 0, 3, 5, 6]                        # positions 2, 4, 7 take no column: they stay zero
    cols = np.array([e[0] for e in entries], np.int64)
    rows = np.array([e[1] for e in entries], np.int64)
    plan = sparse.ColumnPlan(ctx, cols, rows, _bytes([e[2] for e in entries]), n_cols, dst=dst, field="bn256_cs")
    assert plan.n_long == 2 and plan.n_partial == 4 + 2
    out, d_w = _pattern(ctx, n_out + 1), ctx.upload(_bytes(weights))
    plan.run(d_w.ptr, n_rows, out.ptr, n_out)
    want = [0] * n_out
    for c, r, v in entries:
        want[dst[c]] = (want[dst[c]] + v * weights[r]) % N
    assert _get(ctx, out, n_out + 1) == want + [PAT]
    assert want[1] == 0 and want[2] == 0


# ---- comparison -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_first_difference(ctx, n):
    rng = np.random.default_rng(n + 5)
    host = rng.integers(0, 256, size=(n + 1, 32), dtype=np.uint8)
    host[:, 31] &= 0x3F                          # below 2^254 < n: canonical, also with one bit below that flipped
    a, b = ctx.upload(host), ctx.upload(host)
    assert ctx.cs_first_diff(a.ptr, b.ptr, n, bn=True) is None
    if n == 0:
        return
    for i in sorted({0, n // 2, n - 1}):
        e = host[i].copy()
        e[13] ^= 0x08
        ctx.upload_into(b.ptr + 32 * i, e)
        assert ctx.cs_first_diff(a.ptr, b.ptr, n, bn=True) == i
        ctx.upload_into(b.ptr + 32 * i, host[i])
    spots = sorted({n - 1, n // 2, min(n - 1, 255), min(n - 1, 256)})
    for i in spots:
        e = host[i].copy()
        e[7] ^= 0x10
        ctx.upload_into(b.ptr + 32 * i, e)
    assert ctx.cs_first_diff(a.ptr, b.ptr, n, bn=True) == spots[0]


def test_first_difference_compares_residues(ctx):
    vals = [5, N - 1, 0, 123456789]
    other = [v + N if v + N < 1 << 256 else v for v in vals]
    assert other[0] != vals[0]
    a, b = ctx.upload(_bytes(vals)), ctx.upload(_bytes(other))
    assert ctx.cs_first_diff(a.ptr, b.ptr, 4, bn=True) is None
    assert ctx.cs_first_diff(a.ptr, b.ptr, 4) == 0               # over GF(l) the words themselves are compared


# ---- vectors ----------------------------------------------------------------------------------------------------------------
VEC_N = [1, 255, 256, 257, 65537]


def _vec(seed, n):
    rng = random.Random(seed)
    v = [rng.randrange(N) for _ in range(n)]
    v[0], v[-1] = N - 1, N - 1 if n > 1 else v[-1]
    return v


@pytest.mark.parametrize("n", VEC_N)
def test_axpy_and_dot(ctx, n):
    from verifiable_mpc_amd.device import BnScalarVector
    x, y = _vec(1 + n, n), _vec(2 + n, n)
    X, Y = BnScalarVector.from_ints(x, ctx), BnScalarVector.from_ints(y, ctx)
    assert len(X) == n and X.to_ints() == x
    for c in (N - 1, 3, 0):
        assert X.axpy(c, Y).to_ints() == [(c * u + v) % N for u, v in zip(x, y)], c
    assert X.dot(Y) == sum(u * v for u, v in zip(x, y)) % N
    out = _pattern(ctx, 2)
    ctx.fr_dot_into(X.ptr, Y.ptr, n, out.ptr, bn=True)
    assert _get(ctx, out, 2) == [X.dot(Y), PAT]
    assert X[n // 2:].dot(Y[n // 2:]) == sum(u * v for u, v in zip(x[n // 2:], y[n // 2:])) % N


def test_vector_words_above_n_are_reduced_on_load(ctx):
    from verifiable_mpc_amd.device import BnScalarVector
    n = 300
    x, y = _vec(31, n), _vec(32, n)
    raised = [v + N if v + N < 1 << 256 else v for v in x]
    assert sum(u != v for u, v in zip(raised, x)) > 50
    R, X, Y = (BnScalarVector.from_array(_bytes(v), ctx) for v in (raised, x, y))
    assert R.to_ints() == raised                                # the words are stored as they came
    assert R.dot(Y) == X.dot(Y) == sum(u * v for u, v in zip(x, y)) % N
    assert R.axpy(7, Y).to_ints() == X.axpy(7, Y).to_ints()
    assert Y.axpy(7, R).to_ints() == [(7 * v + u) % N for u, v in zip(x, y)]       # canonical results


def test_dot_of_nothing_is_zero(ctx):
    out = _pattern(ctx, 1)
    ctx.fr_dot_into(None, None, 0, out.ptr, bn=True)
    assert _get(ctx, out, 1) == [0]


# ---- the opening's staging step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 14, 255, 256, 257])
def test_koe_stage_and_split(ctx, n):
    rng = random.Random(50 + n)
    x, L, gamma = [rng.randrange(N) for _ in range(n)], [rng.randrange(N) for _ in range(n)], rng.randrange(1, N)
    d_x, d_L = ctx.upload(_bytes(x)), ctx.upload(_bytes(L))
    lhs, rhs = _pattern(ctx, n + 2), _pattern(ctx, n + 1)
    ctx.bn256_koe_stage(d_x.ptr, gamma, d_L.ptr, n, lhs.ptr, rhs.ptr)
    assert _get(ctx, lhs, n + 2) == [gamma] + x + [PAT]
    assert _get(ctx, rhs, n + 1) == L[::-1] + [PAT]
    only = _pattern(ctx, n + 1)
    ctx.bn256_koe_stage(None, None, d_L.ptr, n, None, only.ptr)      # the verifier's half
    assert _get(ctx, only, n + 1) == L[::-1] + [PAT]
    c = [rng.randrange(N) for _ in range(2 * n)]
    d_c, u = ctx.upload(_bytes(c + [PAT])), _pattern(ctx, 2)
    ctx.bn256_koe_split(d_c.ptr, n, u.ptr)
    assert _get(ctx, u, 2) == [c[n], PAT]
    assert _get(ctx, d_c, 2 * n + 1) == c[:n] + [0] + c[n + 1:] + [PAT]


# ---- argument contracts (include/vmpc.h) ----------------------------------------------------------------------------------
def test_argument_contracts(ctx, tables):
    from verifiable_mpc_amd import _native as nat
    lib, h, p = ctx.lib, ctx.handle, ctypes.c_void_p
    assert lib.vmpc_bn256_fr_cs_extend_dev(None, None, None, MAX_M + 1, None, None, None) == nat.E_RANGE
    assert lib.vmpc_bn256_fr_cs_triples_dev(None, None, None, None, None, None, None, None, None, None, MAX_M + 1, 0, 0,
                                            None, None, None, 0, None) == nat.E_RANGE
    assert lib.vmpc_bn256_fr_cs_tables_dev(None, 2 * MAX_M + 2, None, None, None) == nat.E_RANGE
    assert lib.vmpc_bn256_fr_cs_lagrange_dev(None, None, 2 * MAX_M + 2, None, None, None) == nat.E_RANGE
    assert lib.vmpc_bn256_fr_cs_first_diff_dev(None, None, None, (1 << 31) + 1, None) == nat.E_RANGE
    assert lib.vmpc_bn256_fr_cs_extend_dev(h, None, None, MAX_M, None, None, None) == nat.E_INVAL
    assert lib.vmpc_bn256_fr_cs_tables_dev(h, 2 * MAX_M + 1, None, None, None) == nat.E_INVAL
    assert lib.vmpc_bn256_fr_cs_tables_scratch_bytes(0) == 0 == lib.vmpc_bn256_fr_cs_tables_scratch_bytes(2 * MAX_M + 2)
    assert lib.vmpc_bn256_fr_cs_tables_scratch_bytes(33) >= 32 * (2 * 34 + 2 * 2 + 1)
    # a table without scratch is refused, and nothing is written
    fact, ifact = _pattern(ctx, 6), _pattern(ctx, 6)
    assert lib.vmpc_bn256_fr_cs_tables_dev(h, 5, p(fact.ptr), p(ifact.ptr), None) == nat.E_INVAL
    assert _get(ctx, fact, 6) == [PAT] * 6
    # scalar arguments are canonical residues: n itself and 2^256 - 1 are refused, n - 1 is not
    K = 33
    table, lam, x = tables[K][1], _pattern(ctx, K + 1), ctx.upload(_bytes([1, 2, 3]))
    scratch = ctx.alloc(int(lib.vmpc_bn256_fr_cs_lagrange_scratch_bytes(K)))
    for c in (N, 2**256 - 1):
        cb = ctypes.create_string_buffer(c.to_bytes(32, "little"), 32)
        assert lib.vmpc_bn256_fr_cs_lagrange_dev(h, cb, K, p(table.ptr), p(lam.ptr), p(scratch.ptr)) == nat.E_NONCANON
        assert lib.vmpc_bn256_fr_axpy_dev(h, cb, p(x.ptr), None, 3, p(lam.ptr)) == nat.E_NONCANON
        assert lib.vmpc_bn256_koe_stage_dev(h, p(x.ptr), cb, p(x.ptr), 3, p(lam.ptr), p(lam.ptr)) == nat.E_NONCANON
        assert _get(ctx, lam, K + 1) == [PAT] * (K + 1)
    top = ctypes.create_string_buffer((N - 1).to_bytes(32, "little"), 32)
    assert lib.vmpc_bn256_fr_axpy_dev(h, top, p(x.ptr), None, 3, p(lam.ptr)) == nat.OK
    assert _get(ctx, lam, 4) == [N - 1, N - 2, N - 3, PAT]
    # the GF(l) entry still refuses what is canonical only mod n
    assert lib.vmpc_fr_axpy_dev(h, top, p(x.ptr), None, 3, p(lam.ptr)) == nat.E_NONCANON
