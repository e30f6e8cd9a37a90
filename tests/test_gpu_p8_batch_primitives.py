"""The batched Protocol 8 primitives (csrc/circuit_sat.hip: vmpc_fr_cs_triples_batch_dev, vmpc_fr_cs_extend_batch_dev)
through the C-ABI, against their single relatives row by row and against tests/p8_ref.py.  Every comparison is exact.

K witnesses are rows of ONE allocation with a stride that is larger than the row: z rows N + 5 scalars apart, the row
values m + 6 apart, everything filled with a sentinel that no kernel can write (a value above l) first - so a value in
the wrong row, a write into a gap or past the last row shows.

The shapes, from the kernels' constants (restated here): CS_WG = 256 gates per workgroup, FR_CONV_TILE = 256 outputs
per workgroup, FR_CONV_CHUNK = 64, CS_MIN_SEG = 256, CS_TARGET_WGS = 8192.
    triples    levels of 257, 256 and 87 gates (two workgroups with the second one lane wide, one full, a short one), K = 3
    extension  m = 0, 1 (no correlation launch), 2, 3, 63, 64, 65 (the staging chunk), 255, 256 (M = 256 / 257: one and two
               segments), 257, 258 (n_out = 256 / 257: one full tile, a tile and one output), 1000 (a ragged last tile),
               K = 3; and m = 1000 with K = 513, the first K at which tiles x segments x K = 4 x 4 x K exceeds
               CS_TARGET_WGS, so that the batch runs 2 segments of 512 where the single call runs 4 of 256
"""
import ctypes
import random

import numpy as np
import pytest

from tests import p8_ref as ref

pytestmark = pytest.mark.gpu

ELL = ref.ELL
MAX_M = 1 << 20                             # VMPC_FR_CS_MAX_M of include/vmpc.h
MAX_WIT = 65535                             # VMPC_FR_CS_MAX_WIT
PAT_BYTE = 0xA5
PAT = int.from_bytes(bytes([PAT_BYTE]) * 32, "little")      # above l: no kernel here can write it
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
    return ctx.upload(np.full((n, 32), PAT_BYTE, np.uint8))


def _get(ctx, buf, n):
    ctx.sync()
    return _ints(ctx.download(buf.ptr, 32 * n))


# ---- vmpc_fr_cs_triples_batch_dev ------------------------------------------------------------------------------------------
N_X, G_OFF, M_GATES, K = 7, 7 + 8, 600, 3
LEVELS = [(0, 257), (257, 513), (513, 600)]
N_Z = G_OFF + M_GATES + 3
ZS, ABS = N_Z + 5, M_GATES + 6              # the strides


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
    """A, B as [([(col, value)], constant)]: a level reads the inputs and the gates of earlier levels; K distinct
    inputs, the last one all l - 1"""
    rng = random.Random(2600)

    def row(limit):
        e = [(rng.randrange(limit), rng.choice([rng.randrange(1, ELL), ELL - 1, rng.randrange(1, 5)]))
             for _ in range(rng.randrange(1, 5))]
        return (e, rng.randrange(ELL) if rng.random() < 0.5 else 0)

    A, B = [None] * M_GATES, [None] * M_GATES
    gates = []
    for lo, hi in LEVELS:
        for i in range(lo, hi):
            A[i], B[i] = row(N_X + lo), row(N_X + lo)
        order = list(range(lo, hi))
        rng.shuffle(order)
        gates += order
    xs = [[rng.randrange(ELL) for _ in range(N_X)] for _ in range(K - 1)] + [[ELL - 1] * N_X]
    want = [ref.triples(N_X, A, B, x) for x in xs]
    assert len({tuple(w[2]) for w in want}) == K
    keep_a, csr_a = _csr(ctx, A)
    keep_b, csr_b = _csr(ctx, B)
    return {"A": A, "B": B, "csr_a": csr_a, "csr_b": csr_b, "keep": (keep_a, keep_b), "x": xs, "want": want,
            "gates": ctx.upload(np.array(gates, np.uint32))}


def _z_row(x, gamma):
    return x + [PAT] * (G_OFF - N_X) + gamma + [PAT] * (N_Z - G_OFF - M_GATES)


def _z_image(rows):
    """K rows of N_Z at stride ZS and one more scalar after the last gap"""
    return [v for r in rows for v in r + [PAT] * (ZS - N_Z)] + [PAT]


def _ab_image(rows):
    return [v for r in rows for v in r + [PAT] * (ABS - len(r))] + [PAT]


def test_triples_level_by_level_against_the_single_entry(ctx, circuit):
    xs, want = circuit["x"], circuit["want"]
    z = ctx.upload(_bytes(_z_image([_z_row(x, [PAT] * M_GATES) for x in xs])))
    a_out, b_out = _pattern(ctx, K * ABS + 1), _pattern(ctx, K * ABS + 1)
    # the single entry on each witness's own buffers
    singles = []
    for x in xs:
        sz = ctx.upload(_bytes(_z_row(x, [PAT] * M_GATES)))
        sa, sb = _pattern(ctx, M_GATES), _pattern(ctx, M_GATES)
        singles.append((sz, sa, sb))
    for i, (lo, hi) in enumerate(LEVELS):
        ctx.cs_triples_batch(circuit["csr_a"], circuit["csr_b"], circuit["gates"].ptr + 4 * lo, hi - lo, N_X, G_OFF, z.ptr,
                             ZS, a_out.ptr, b_out.ptr, ABS, K)
        for sz, sa, sb in singles:
            ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], circuit["gates"].ptr + 4 * lo, hi - lo, N_X, G_OFF, sz.ptr,
                           sa.ptr, sb.ptr)
        # what the level wrote and nothing else: inputs, gaps, later levels, the tails, the scalar past the end
        got_z = _get(ctx, z, K * ZS + 1)
        assert got_z == _z_image([_z_row(x, w[2][:hi] + [PAT] * (M_GATES - hi)) for x, w in zip(xs, want)]), i
        assert got_z == _z_image([_get(ctx, sz, N_Z) for sz, _, _ in singles]), i
        assert _get(ctx, a_out, K * ABS + 1) == _ab_image([w[0][:hi] + [PAT] * (M_GATES - hi) for w in want]), i
        assert _get(ctx, b_out, K * ABS + 1) == _ab_image([w[1][:hi] + [PAT] * (M_GATES - hi) for w in want]), i
    assert _get(ctx, a_out, K * ABS + 1) == _ab_image([_get(ctx, sa, M_GATES) for _, sa, _ in singles])
    assert _get(ctx, b_out, K * ABS + 1) == _ab_image([_get(ctx, sb, M_GATES) for _, _, sb in singles])


def test_triples_check_reports_each_witness_its_own_smallest_bad_gate(ctx, circuit):
    xs, want = circuit["x"], circuit["want"]
    spoiled = [(), (599, 300, 256, 255), (599,)]
    rows = []
    for x, w, sp in zip(xs, want, spoiled):
        gamma = list(w[2])
        for i in sp:
            gamma[i] = (gamma[i] + 1) % ELL
        rows.append(_z_row(x, gamma))
    image = _z_image(rows)
    z = ctx.upload(_bytes(image))
    a_out, b_out = _pattern(ctx, K * ABS + 1), _pattern(ctx, K * ABS + 1)
    bad = ctx.upload(np.array([7] * (K + 1), np.uint32))
    ctx.cs_triples_batch(circuit["csr_a"], circuit["csr_b"], None, M_GATES, N_X, G_OFF, z.ptr, ZS, a_out.ptr, b_out.ptr, ABS,
                         K, 1, bad.ptr)
    ctx.sync()
    assert ctx.download(bad.ptr, 4 * (K + 1)).view(np.uint32).tolist() == [NONE, 255, 599, 7]
    assert _get(ctx, z, K * ZS + 1) == image            # the gammas are the caller's: nothing is written to z
    # the wires of a clean witness are its own
    assert _get(ctx, a_out, K * ABS + 1)[:M_GATES] == want[0][0]
    assert _get(ctx, b_out, K * ABS + 1)[:M_GATES] == want[0][1]


def test_triples_values_only_over_the_output_rows(ctx, circuit):
    """check = 2: one matrix as A and as B, one buffer as both outputs, no first_bad"""
    xs, want = circuit["x"], circuit["want"]
    image = _z_image([_z_row(x, w[2]) for x, w in zip(xs, want)])
    z = ctx.upload(_bytes(image))
    out = _pattern(ctx, K * ABS + 1)
    ctx.cs_triples_batch(circuit["csr_a"], circuit["csr_a"], None, M_GATES, N_X, G_OFF, z.ptr, ZS, out.ptr, out.ptr, ABS, K,
                         2, None)
    assert _get(ctx, out, K * ABS + 1) == _ab_image([[ref.row_eval(r, N_X, x, w[2]) for r in circuit["A"]]
                                                     for x, w in zip(xs, want)])
    assert _get(ctx, z, K * ZS + 1) == image
    # a row stride equal to the row count: the rows are contiguous, as the prover's output buffer is
    tight = _pattern(ctx, K * M_GATES + 1)
    ctx.cs_triples_batch(circuit["csr_b"], circuit["csr_b"], None, M_GATES, N_X, G_OFF, z.ptr, ZS, tight.ptr, tight.ptr,
                         M_GATES, K, 2, None)
    assert _get(ctx, tight, K * M_GATES + 1) == [ref.row_eval(r, N_X, x, w[2]) for x, w in zip(xs, want)
                                                 for r in circuit["B"]] + [PAT]


# ---- vmpc_fr_cs_extend_batch_dev -------------------------------------------------------------------------------------------
N_IN = 2                                    # z_tail starts inside the row: the x part is not the entry's to touch
# (m, K, the witnesses compared with the single entry)
EXTEND_CASES = [(m, 3, (0, 1, 2)) for m in (1000, 0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 258)] + [(1000, 513, (0, 256, 512))]


@pytest.mark.parametrize("m,n_wit,compared", EXTEND_CASES, ids=[f"m{m}_K{k}" for m, k, _ in EXTEND_CASES])
def test_extension_against_the_single_entry(ctx, m, n_wit, compared):
    M, T = m + 1, max(2 * m + 1, 1)
    N = N_IN + 2 * m + 3
    zs, abs_ = N + 5, m + 6
    fact, ifact = ctx.alloc(32 * (T + 1)), ctx.alloc(32 * (T + 1))
    ctx.cs_tables(T, fact.ptr, ifact.ptr)
    rng = np.random.default_rng(9100 + m + n_wit)

    def rows(stride):
        """n_wit rows of M random canonical residues at `stride`, the gaps the sentinel"""
        img = np.full((n_wit, stride, 32), PAT_BYTE, np.uint8)
        img[:, :M] = rng.integers(0, 256, size=(n_wit, M, 32), dtype=np.uint8)
        img[:, :M, 31] &= 0x0f
        if n_wit == 3:
            img[2, :M] = _bytes([ELL - 1])[0]           # every value l - 1: the largest products and carries
        return img

    a_img, b_img = rows(abs_), rows(abs_)
    d_a, d_b = ctx.upload(a_img), ctx.upload(b_img)
    z = _pattern(ctx, n_wit * zs + 1)
    ctx.cs_extend_batch(d_a.ptr, d_b.ptr, abs_, m, fact.ptr, ifact.ptr, z.ptr + 32 * N_IN, zs, n_wit)
    ctx.sync()
    got = ctx.download(z.ptr, 32 * (n_wit * zs + 1)).reshape(-1, 32)
    written = [0, 1, 2] + ([2 + m + 1] if m else []) + [2 + x for x in range(m + 2, 2 * m + 1)]
    untouched = np.ones(n_wit * zs + 1, bool)
    for w in range(n_wit):
        untouched[[w * zs + N_IN + p for p in written]] = False
    # the x part, the gammas' places, the gaps and the scalar past the last row
    assert (got[untouched] == PAT_BYTE).all()
    assert (got[~untouched, 31] <= 0x10).all()          # and every place of the entry's was written
    # the row values are read only
    assert (ctx.download(d_a.ptr, a_img.nbytes).reshape(a_img.shape) == a_img).all()
    for w in compared:
        sa, sb = ctx.upload(a_img[w, :M]), ctx.upload(b_img[w, :M])
        sz = _pattern(ctx, 2 * m + 3)
        ctx.cs_extend(sa.ptr, sb.ptr, m, fact.ptr, ifact.ptr, sz.ptr)
        single = _get(ctx, sz, 2 * m + 3)
        mine = _ints(got[w * zs + N_IN:w * zs + N])
        assert [mine[p] for p in written] == [single[p] for p in written], w
    # and one witness without the single entry
    w = compared[-1]
    a, b = _ints(a_img[w, :M]), _ints(b_img[w, :M])
    want = ref.z_tail_bary(a[:m], b[:m], a[m], b[m])
    mine = _ints(got[w * zs + N_IN:w * zs + N])
    assert [mine[p] for p in written] == [want[p] for p in written]


def test_workspace_of_a_batch_does_not_grow_as_the_single_calls(ctx):
    """the segment length is chosen with the witnesses counted: the partial sums of 8 witnesses at m = 2^16 take less
    than twice one witness's, not eight times"""
    one, eight = ctx.cs_extend_batch_bytes(1 << 16, 1), ctx.cs_extend_batch_bytes(1 << 16, 8)
    assert 0 < one < eight < 2 * one
    # m = 1000: 4 segments up to K = 512, 2 from K = 513 on - one more witness, less workspace
    assert ctx.cs_extend_batch_bytes(1000, 513) < ctx.cs_extend_batch_bytes(1000, 512)
    assert ctx.cs_extend_batch_bytes(MAX_M + 1, 1) == 0 and ctx.cs_extend_batch_bytes(8, MAX_WIT + 1) == 0
    assert ctx.cs_extend_batch_bytes(8, 0) == 0


# ---- argument contracts (include/vmpc.h) ----------------------------------------------------------------------------------
def test_argument_contracts(ctx, circuit):
    from verifiable_mpc_amd import _native as nat
    lib, h, p = ctx.lib, ctx.handle, ctypes.c_void_p
    nul = [None] * 9
    # above a cap: VMPC_E_RANGE before any pointer is looked at - the context's included
    assert lib.vmpc_fr_cs_triples_batch_dev(None, *nul, MAX_M + 1, 0, 0, None, 0, None, None, 0, 1, 0, None) == nat.E_RANGE
    assert lib.vmpc_fr_cs_triples_batch_dev(None, *nul, 1, 0, 0, None, 1, None, None, 1, MAX_WIT + 1, 0, None) == nat.E_RANGE
    assert lib.vmpc_fr_cs_extend_batch_dev(None, None, None, MAX_M + 2, MAX_M + 1, None, None, None, 2 * MAX_M + 5, 1) == \
        nat.E_RANGE
    assert lib.vmpc_fr_cs_extend_batch_dev(None, None, None, 9, 8, None, None, None, 19, MAX_WIT + 1) == nat.E_RANGE
    # at the caps the null pointers are the complaint
    assert lib.vmpc_fr_cs_triples_batch_dev(h, *nul, MAX_M, 0, 0, None, MAX_M, None, None, MAX_M, MAX_WIT, 0, None) == \
        nat.E_INVAL
    assert lib.vmpc_fr_cs_extend_batch_dev(h, None, None, MAX_M + 1, MAX_M, None, None, None, 2 * MAX_M + 3, MAX_WIT) == \
        nat.E_INVAL
    xs, want = circuit["x"], circuit["want"]
    image = _z_image([_z_row(x, w[2]) for x, w in zip(xs, want)])
    z = ctx.upload(_bytes(image))
    out, bad = _pattern(ctx, K * ABS + 1), ctx.upload(np.array([7] * K, np.uint32))
    ca, cb = [p(v) for v in circuit["csr_a"]], [p(v) for v in circuit["csr_b"]]

    def triples(n_gates=M_GATES, z_stride=ZS, ab_stride=ABS, n_wit=K, check=1, first_bad=p(bad.ptr), z_ptr=p(z.ptr)):
        return lib.vmpc_fr_cs_triples_batch_dev(h, *ca, *cb, None, n_gates, N_X, G_OFF, z_ptr, z_stride, p(out.ptr),
                                                p(out.ptr), ab_stride, n_wit, check, first_bad)

    # a stride below the row length
    assert triples(z_stride=G_OFF + M_GATES - 1) == nat.E_RANGE
    assert triples(ab_stride=M_GATES - 1) == nat.E_RANGE
    assert triples(z_stride=(1 << 31) + 1) == nat.E_RANGE
    # check is 0, 1 or 2, and 1 needs a place for its answers; no z
    for kw in ({"check": 3}, {"check": -1}, {"first_bad": None}, {"z_ptr": None}):
        assert triples(**kw) == nat.E_INVAL, kw
    # nothing to do: VMPC_OK without a launch, and first_bad is not reset either
    assert triples(n_wit=0) == nat.OK and triples(n_gates=0) == nat.OK
    assert _get(ctx, out, K * ABS + 1) == [PAT] * (K * ABS + 1)
    assert _get(ctx, z, K * ZS + 1) == image
    assert ctx.download(bad.ptr, 4 * K).view(np.uint32).tolist() == [7] * K
    # the extension
    m = 5
    fact, ifact = ctx.alloc(32 * 12), ctx.alloc(32 * 12)
    ctx.cs_tables(11, fact.ptr, ifact.ptr)
    a = ctx.upload(_bytes([3] * (2 * (m + 1))))
    zt = _pattern(ctx, 2 * (2 * m + 3))

    def extend(ab_stride=m + 1, z_stride=2 * m + 3, n_wit=2, a_ptr=p(a.ptr), zt_ptr=p(zt.ptr), f_ptr=p(fact.ptr)):
        return lib.vmpc_fr_cs_extend_batch_dev(h, a_ptr, p(a.ptr), ab_stride, m, f_ptr, p(ifact.ptr), zt_ptr, z_stride, n_wit)

    assert extend(ab_stride=m) == nat.E_RANGE and extend(z_stride=2 * m + 2) == nat.E_RANGE
    assert extend(ab_stride=(1 << 31) + 1) == nat.E_RANGE
    for kw in ({"a_ptr": None}, {"zt_ptr": None}, {"f_ptr": None}):
        assert extend(**kw) == nat.E_INVAL, kw
    assert extend(n_wit=0) == nat.OK
    assert _get(ctx, zt, 2 * (2 * m + 3)) == [PAT] * (2 * (2 * m + 3))
    assert extend() == nat.OK
    got = _get(ctx, zt, 2 * (2 * m + 3))
    want_tail = ref.z_tail_bary([3] * m, [3] * m, 3, 3)
    assert got[:3] == want_tail[:3] and got[2 * m + 3:2 * m + 6] == want_tail[:3]
