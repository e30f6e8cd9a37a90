"""A single call is a batch of one.  Every stage of csrc/circuit_sat.hip, csrc/bn256_qap_h.hip and csrc/bn256_koe.hip
that has a *_batch_dev entry runs ONE kernel and ONE host function for both entries; the single entry passes n_wit = 1.
For each pair this file calls the single entry and the batch entry with n_wit = 1 and tight strides (a stride equal to
the row's length) on the same inputs and asserts that
    the two outputs are the same bytes,
    both are the CPU restatement of that stage (tests/p8_ref.py, tests/h_ref.py, the formulas of include/vmpc.h),
    and GUARD sentinel scalars (or words) on both sides of every output buffer come back untouched.
The comparison with the CPU is what keeps "batch equals single" from being a statement about one kernel and itself.

Shapes: the smallest at which the witness offset, a tile edge or a second segment can go wrong.
    Protocol 8   m in {0, 1, 2, 257, 258}: n_out = m - 1 = 256 / 257 is one full 256-output tile / a tile and one output,
                 M = m + 1 = 258 / 259 lies above CS_MIN_SEG = 256 (two segments of j); m = 0, 1 launch no correlation;
                 for the triples 257 / 258 gates are two workgroups of CS_WG = 256
    h            d in {1, 2, 255, 257} (d = 1: the empty window P[0 .. d-2]; 257: a second tile and a second segment of
                 the two half products), and d = 1025 for the moments alone: a second QH_CHUNK = 1024 of j, hence two
                 groups of j and partial sums through the arena.  At d = 1025 n_out is 65 (a second QH_KB = 64 block
                 of k): the chunks cut j, not k, and the CPU sum over 1025 x 1025 terms would take a second.
    product      (na, nb) in {(1, 1), (256, 2), (257, 300)}: one output; a tile and one output straight to `out`;
                 segments of 256 through the arena
"""
import numpy as np
import pytest

from tests import h_ref as H
from tests import p8_ref as ref
from tests.test_gpu_koe import coeff
from tests.test_gpu_p8_batch_primitives import NONE, PAT, PAT_BYTE, _bytes, _csr, _ints, ctx  # noqa: F401 (ctx: fixture)
from tests.test_gpu_pinocchio_batch_primitives import _rand, _to_ints
from tests.test_gpu_pinocchio_h import _moments_ref, _weights

pytestmark = pytest.mark.gpu

ELL, N = ref.ELL, H.N
GUARD = 3                                   # sentinel scalars (words) before and after every output buffer
WORD = 0x5A5A5A5A


class Guarded:
    """a device buffer of GUARD + n + GUARD scalars; .ptr is the first of the n.  `fill`: the n scalars as ints
    (default: the sentinel, which is above both moduli - no kernel here can write it)"""

    def __init__(self, ctx, n, fill=None):
        self.ctx, self.n = ctx, n
        body = [PAT] * n if fill is None else list(fill)
        assert len(body) == n
        self.buf = ctx.upload(_bytes([PAT] * GUARD + body + [PAT] * GUARD))
        self.ptr = self.buf.ptr + 32 * GUARD

    def image(self):
        """all GUARD + n + GUARD scalars"""
        self.ctx.sync()
        return _ints(self.ctx.download(self.buf.ptr, 32 * (self.n + 2 * GUARD)))


def _framed(body):
    return [PAT] * GUARD + list(body) + [PAT] * GUARD


class GuardedWord:
    """one device uint32 between GUARD words on each side"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.buf = ctx.upload(np.full(2 * GUARD + 1, WORD, np.uint32))
        self.ptr = self.buf.ptr + 4 * GUARD

    def image(self):
        self.ctx.sync()
        return self.ctx.download(self.buf.ptr, 4 * (2 * GUARD + 1)).view(np.uint32).tolist()


def _framed_word(v):
    return [WORD] * GUARD + [v] + [WORD] * GUARD


def _residues(rng, n, mod):
    """n canonical residues, the first one mod - 1"""
    return [mod - 1] + [int.from_bytes(rng.bytes(32), "little") % mod for _ in range(n - 1)] if n else []


# ---- Protocol 8: triples ------------------------------------------------------------------------------------------------
N_X = 5
P8_M = [0, 1, 2, 257, 258]


def _two_level_circuit(rng, m):
    """m gates in two depth levels: gates below m // 2 read the inputs, the others the inputs and the first level"""
    def row(limit):
        e = [(int(rng.integers(limit)), [ELL - 1, 1, 2, int.from_bytes(rng.bytes(31), "little")][int(rng.integers(4))])
             for _ in range(int(rng.integers(1, 4)))]
        return (e, int.from_bytes(rng.bytes(31), "little") if rng.random() < 0.5 else 0)
    half = m // 2
    A = [row(N_X if i < half else N_X + half) for i in range(m)]
    B = [row(N_X if i < half else N_X + half) for i in range(m)]
    return A, B, [lv for lv in ((0, half), (half, m)) if lv[1] > lv[0]]


@pytest.mark.parametrize("check", [0, 1, 2])
@pytest.mark.parametrize("m", P8_M)
def test_triples(ctx, m, check):
    rng = np.random.default_rng(100 * m + check)
    A, B, levels = _two_level_circuit(rng, m)
    x = _residues(rng, N_X, ELL)
    a_want, b_want, gamma = ref.triples(N_X, A, B, x)
    n_z = N_X + m + 1                        # x, the gammas and one scalar of z that is nobody's to write
    keep_a, csr_a = _csr(ctx, A if m else [([(0, 1)], 0)])       # m = 0: the entries still want their pointers
    keep_b, csr_b = _csr(ctx, B if m else [([(0, 1)], 0)])
    spoiled = sorted({m - 1, 256} & set(range(m))) if check == 1 else []
    given = list(gamma)
    for i in spoiled:
        given[i] = (given[i] + 1) % ELL
    z_in = x + ([PAT] * m if check == 0 else given) + [PAT]
    got = []
    for batch in (False, True):
        z, bad = Guarded(ctx, n_z, z_in), GuardedWord(ctx)
        a_out = Guarded(ctx, m)
        b_out = a_out if check == 2 else Guarded(ctx, m)
        mats = (csr_a, csr_a) if check == 2 else (csr_a, csr_b)
        for lo, hi in (levels if check == 0 and m else [(0, m)]):      # m = 0: one call with no gates
            gates = ctx.upload(np.arange(lo, max(hi, 1), dtype=np.uint32))
            first_bad = bad.ptr if check == 1 else None
            if batch:
                ctx.cs_triples_batch(*mats, gates.ptr, hi - lo, N_X, N_X, z.ptr, n_z, a_out.ptr, b_out.ptr, max(m, 1), 1,
                                     check, first_bad)
            else:
                ctx.cs_triples(*mats, gates.ptr, hi - lo, N_X, N_X, z.ptr, a_out.ptr, b_out.ptr, check, first_bad)
        got.append((z.image(), a_out.image(), b_out.image(), bad.image()))
    assert got[0] == got[1]
    z_img, a_img, b_img, bad_img = got[0]
    assert z_img == _framed(x + (gamma if check == 0 else given) + [PAT])
    if check == 2:
        assert a_img == _framed([ref.row_eval(r, N_X, x, gamma) for r in A])
    else:
        assert a_img == _framed(a_want) and b_img == _framed(b_want)
    assert bad_img == _framed_word((spoiled[0] if spoiled else NONE) if check == 1 and m else WORD)


# ---- Protocol 8: the extension ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", P8_M)
def test_extend(ctx, m):
    M, T = m + 1, max(2 * m + 1, 1)
    fact, ifact = ctx.alloc(32 * (T + 1)), ctx.alloc(32 * (T + 1))
    ctx.cs_tables(T, fact.ptr, ifact.ptr)
    rng = np.random.default_rng(7000 + m)
    a, b = _residues(rng, M, ELL), _residues(rng, M, ELL)
    da, db = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
    single, batch = Guarded(ctx, 2 * m + 3), Guarded(ctx, 2 * m + 3)
    ctx.cs_extend(da.ptr, db.ptr, m, fact.ptr, ifact.ptr, single.ptr)
    ctx.cs_extend_batch(da.ptr, db.ptr, M, m, fact.ptr, ifact.ptr, batch.ptr, 2 * m + 3, 1)
    tail = ref.z_tail_bary(a[:m], b[:m], a[m], b[m])
    want = [PAT] * (2 * m + 3)               # the gammas' places z_tail[3 .. 2 + m] are left alone
    for p in [0, 1, 2] + ([2 + m + 1] if m else []) + [2 + x for x in range(m + 2, 2 * m + 1)]:
        want[p] = tail[p]
    assert single.image() == batch.image() == _framed(want)


# ---- h: moments, weights, check, combination ---------------------------------------------------------------------------
H_D = [1, 2, 255, 257]


def _reduced(arr):
    return [v % N for v in _to_ints(arr)]


@pytest.mark.parametrize("vectors", [1, 2])
@pytest.mark.parametrize("d", H_D + [1025])
def test_moments(ctx, d, vectors):
    n_out = d if d < 1025 else 65
    rng = np.random.default_rng(10 * d + vectors)
    u = [_rand(rng, d) for _ in range(vectors)]
    du = [ctx.upload(v) for v in u] + [None]
    ptr = lambda b: b.ptr if b is not None else None
    single = [Guarded(ctx, n_out) for _ in range(vectors)] + [None]
    batch = [Guarded(ctx, n_out) for _ in range(vectors)] + [None]
    ctx.bn256_qap_moments(du[0].ptr, ptr(du[1]), d, n_out, single[0].ptr, ptr(single[1]))
    ctx.bn256_qap_moments_batch(du[0].ptr, ptr(du[1]), d, d, n_out, batch[0].ptr, ptr(batch[1]), n_out, 1)
    for v in range(vectors):
        assert single[v].image() == batch[v].image() == _framed(_moments_ref(_reduced(u[v]), n_out)), v


@pytest.mark.parametrize("d", H_D)
def test_weights(ctx, d):
    rng = np.random.default_rng(d)
    a, b = _rand(rng, d), _rand(rng, d)
    da, db = ctx.upload(a), ctx.upload(b)
    s_a, s_b, b_a, b_b = (Guarded(ctx, d) for _ in range(4))
    ctx.bn256_qap_h_weights(da.ptr, db.ptr, d, s_a.ptr, s_b.ptr)
    ctx.bn256_qap_h_weights_batch(da.ptr, db.ptr, d, d, b_a.ptr, b_b.ptr, d, 1)
    inv_w = [pow(w, -1, N) for w in _weights(d)]
    assert s_a.image() == b_a.image() == _framed([x * f % N for x, f in zip(_reduced(a), inv_w)])
    assert s_b.image() == b_b.image() == _framed([x * f % N for x, f in zip(_reduced(b), inv_w)])


@pytest.mark.parametrize("spoil", [(), (-1,), (-1, 0)], ids=["clean", "last", "last_and_first"])
@pytest.mark.parametrize("d", H_D)
def test_check(ctx, d, spoil):
    rng = np.random.default_rng(d)
    a, b = _rand(rng, d), _rand(rng, d)
    y = [p * q % N for p, q in zip(_reduced(a), _reduced(b))]
    bad_rows = sorted({i % d for i in spoil})
    for i in bad_rows:
        y[i] = (y[i] + 1) % N
    da, db, dy = ctx.upload(a), ctx.upload(b), ctx.upload(_bytes(y))
    single, batch = GuardedWord(ctx), GuardedWord(ctx)
    ctx.bn256_qap_check(da.ptr, db.ptr, dy.ptr, d, single.ptr)
    ctx.bn256_qap_check_batch(da.ptr, db.ptr, dy.ptr, d, d, batch.ptr, 1)
    assert single.image() == batch.image() == _framed_word(bad_rows[0] if bad_rows else NONE)


def _combine_ref(A, B, t, deltas):
    """include/vmpc.h: C_k = sum_{i=1..k-1} A_i B_(k-i) + delta_v B_k + delta_w A_k, h_e = sum_{i=e+1..d} t_i C_(i-e)
    + delta_v delta_w t_e - [e = 0] delta_y, with A[i] = A_(i+1)"""
    d = len(A)
    dv, dw, dy = deltas if deltas is not None else (0, 0, 0)
    P = H.poly_mul(A, B)
    C = [0] + [((P[k - 2] if k >= 2 else 0) + dv * B[k - 1] + dw * A[k - 1]) % N for k in range(1, d + 1)]
    return [(sum(t[i] * C[i - e] for i in range(e + 1, d + 1)) + dv * dw * t[e] - (dy if e == 0 else 0)) % N
            for e in range(d + 1)]


@pytest.mark.parametrize("zk", [False, True], ids=["plain", "deltas"])
@pytest.mark.parametrize("d", H_D)
def test_combine(ctx, d, zk):
    rng = np.random.default_rng(2 * d + zk)
    A, B, deltas = _rand(rng, d), _rand(rng, d), _rand(rng, 3)
    t = H.t_coeffs(d)
    dA, dB, dd, dt = ctx.upload(A), ctx.upload(B), ctx.upload(deltas), ctx.upload(_bytes(t))
    # the scratch is nobody's output, but the single entry's 5 d and the batch's 3 d must not be overrun either
    s_scratch, b_scratch = Guarded(ctx, 5 * d), Guarded(ctx, 3 * d)
    single, batch = Guarded(ctx, d + 1), Guarded(ctx, d + 1)
    ctx.bn256_qap_h_combine(dA.ptr, dB.ptr, dt.ptr, d, dd.ptr if zk else None, s_scratch.ptr, single.ptr)
    ctx.bn256_qap_h_combine_batch(dA.ptr, dB.ptr, d, dt.ptr, d, dd.ptr if zk else None, b_scratch.ptr, batch.ptr, d + 1, 1)
    want = _combine_ref(_reduced(A), _reduced(B), t, _reduced(deltas) if zk else None)
    assert single.image() == batch.image() == _framed(want)
    for sc in (s_scratch, b_scratch):
        img = sc.image()
        assert img[:GUARD] == img[-GUARD:] == [PAT] * GUARD
    assert s_scratch.image()[GUARD + 3 * d:] == [PAT] * (2 * d + GUARD)      # 3 d of the documented 5 d are used


# ---- the polynomial product ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(1, 1), (256, 2), (257, 300)])
def test_poly_mul(ctx, na, nb):
    rng = np.random.default_rng(na + nb)
    a, b = _rand(rng, na), _rand(rng, nb)
    da, db = ctx.upload(a), ctx.upload(b)
    n = na + nb - 1
    single, batch = Guarded(ctx, n), Guarded(ctx, n)
    ctx.bn256_fr_poly_mul(da.ptr, na, db.ptr, nb, single.ptr)
    ctx.bn256_fr_poly_mul_batch(da.ptr, na, na, db.ptr, nb, nb, 0, n, batch.ptr, n, 1)
    ar, br = _reduced(a), _reduced(b)
    assert single.image() == batch.image() == _framed([coeff(ar, br, k) for k in range(n)])
