"""Protocol 8's device primitives (csrc/circuit_sat.hip) one entry point at a time, against tests/p8_ref.py.  Every
comparison is exact (integer lists mod l); inputs are canonical residues, as the entries' contract asks.

The shapes stand for boundaries of the kernels' constants, restated here (nothing is imported from the code under
test): CS_RUN = 32 (sequence elements per scan lane), FR_SCAN_WG = 256 (threads of the one workgroup that scans the
lanes' run products), FR_CONV_TILE = 256 (outputs per workgroup of the correlation), FR_CONV_CHUNK = 64 (elements of u
staged per step), CS_MIN_SEG = 256 (shortest segment of j), CS_WG = 256 (every other kernel's workgroup).

vmpc_fr_cs_tables_dev, vmpc_fr_cs_lagrange_dev (csrc/fr_scan.h with RUN = 32; the sequences have K elements):
    lanes = ceil(K / CS_RUN) run products, thread t of the scanning workgroup owns per = ceil(lanes / FR_SCAN_WG) of them
    K = 0             no element at all (Lagrange only: the vector is [1])
    K = 1, 2          one short run
    K = 31, 32, 33    a run one short of full, full, and a second lane of one element
    K = 63, 64, 65    the same one lane further
    K = 8191, 8192    lanes = 256: per = 1, every thread owns one run (at 8191 the last run is short)
    K = 8193          lanes = 257: per = 2, threads 129..255 own nothing, the thread that hands on the total among them
    K = 16384         lanes = 512: per = 2, every block full
    K = 16385         lanes = 513: per = 3, 171 threads own something, 85 nothing
    c on a node: the prefix products turn to zero in the middle of a run and stay zero through the scan
vmpc_fr_cs_extend_dev (M = m + 1 elements of u, n_out = m - 1 outputs x = m + 2 .. 2m, tiles = ceil(n_out / FR_CONV_TILE),
segments = ceil(M / CS_MIN_SEG), chunks of FR_CONV_CHUNK inside a segment):
    m = 0, 1          n_out = 0: no correlation launch; m = 0 has no h(m + 1)
    m = 2, 3          n_out = 1, 2
    m = 63, 64, 65    M = 64, 65, 66: one full chunk, a second chunk of one and of two elements
    m = 255, 256, 257 M = 256 (one full segment; k_cs_dot0's lanes take one element each), 257 (a second segment of one
                      element), 258; n_out = 254, 255, 256 (a tile one short of full, full)
    m = 258           n_out = 257: a second tile of one output
    m = 511, 512, 513 M = 512 (two full segments), 513 (a third of one element), 514; n_out = 510, 511, 512 (two full tiles)
    m = 1025          n_out = 1024 (four full tiles), M = 1026 (a fifth segment of two elements)
    m = 4097          n_out = 4096 (16 tiles), M = 4098 (17 segments); it runs first, so the arena shrinks in use afterwards
    (the segment length leaves CS_MIN_SEG at m = 23042: the whole-proof case m = 32000 of tests/test_gpu_circuit_sat.py)
vmpc_fr_cs_triples_dev (CS_WG gates per workgroup, a lane per gate):
    levels of 257, 256 and 87 gates: two workgroups with the second one lane wide, one full, a short one
    a row of 300 entries at the largest residues: more than the 64 entries of a column-sum item in one accumulator
    bad gates 255 and 256: the last lane of workgroup 0 and the first of workgroup 1
vmpc_fr_cs_first_diff_dev (CS_WG elements per workgroup):
    n = 0 (no launch), 1, 255, 256, 257 (a workgroup one short of full, full, a second of one lane), 70001 (274 workgroups)
"""
import ctypes
import math
import random

import numpy as np
import pytest

from tests import p8_ref as ref

pytestmark = pytest.mark.gpu

ELL = ref.ELL
MAX_M = 1 << 20                             # VMPC_FR_CS_MAX_M of include/vmpc.h
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


# ---- vmpc_fr_cs_tables_dev ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 16384, 16385])
def test_factorial_tables(ctx, K):
    fact, ifact = _pattern(ctx, K + 2), _pattern(ctx, K + 2)
    ctx.cs_tables(K, fact.ptr, ifact.ptr)
    got_f, got_i = _get(ctx, fact, K + 2), _get(ctx, ifact, K + 2)
    assert got_f[K + 1] == PAT and got_i[K + 1] == PAT
    want_f, want_i = ref.tables(K)
    assert got_f[:K + 1] == want_f
    assert got_i[:K + 1] == want_i
    # and without the reference
    assert all(f * i % ELL == 1 for f, i in zip(got_f[:K + 1], got_i[:K + 1]))
    assert got_f[K] == math.factorial(K) % ELL


# ---- vmpc_fr_cs_lagrange_dev ----------------------------------------------------------------------------------------------
def _device_ifact(ctx, K):
    fact, ifact = ctx.alloc(32 * (K + 1)), ctx.alloc(32 * (K + 1))
    ctx.cs_tables(K, fact.ptr, ifact.ptr)
    return ifact


# (K, the K of the table that ifact comes from): the prover takes both of its vectors (K = m and K = 2m) from the
# table of 2m + 1
LAGRANGE_CASES = [(K, max(K, 1)) for K in (0, 1, 2, 31, 32, 33, 8192, 8193, 16385)] + [(8193, 2 * 8193 + 1)]


@pytest.mark.parametrize("K,table_K", LAGRANGE_CASES, ids=[f"K{k}_table{t}" for k, t in LAGRANGE_CASES])
def test_lagrange_vector(ctx, K, table_K):
    ifact = _device_ifact(ctx, table_K)
    rng = random.Random(7000 + K)
    nodes = sorted({j for j in (0, 1, 31, 32, 33, K // 2, K - 1, K) if 0 <= j <= K})
    for c in [rng.randrange(ELL), rng.randrange(ELL), ELL - 1, K + 1] + nodes:
        out = _pattern(ctx, K + 2)
        ctx.cs_lagrange(c, K, ifact.ptr, out.ptr)
        got = _get(ctx, out, K + 2)
        assert got[K + 1] == PAT, c
        lam = got[:K + 1]
        assert lam == ref.lagrange_bary(K, c), c
        if c <= K:
            assert lam == [int(j == c) for j in range(K + 1)], c
            continue
        # the constant polynomial and x^e, e <= K, are reproduced from their values on the nodes
        assert sum(lam) % ELL == 1, c
        for e in {min(1, K), K}:
            assert sum(v * pow(j, e, ELL) for j, v in enumerate(lam)) % ELL == pow(c, e, ELL), (c, e)
        if K <= 33:
            assert lam == ref.lagrange_naive(K, c), c


# ---- vmpc_fr_cs_extend_dev ------------------------------------------------------------------------------------------------
# m = 4097 first and m = 2 after it: the arena (a module-scoped context) is then larger than the call needs
EXTEND_M = [4097, 2, 0, 1, 3, 63, 64, 65, 255, 256, 257, 258, 511, 512, 513, 1025]
EXTEND_CASES = [(m, "random") for m in EXTEND_M[:1]] + [(4097, "top")] + [(m, "random") for m in EXTEND_M[1:]] + \
               [(m, "top") for m in (65, 258, 513)] + [(m, "zero_a") for m in (2, 258)]


@pytest.mark.parametrize("m,kind", EXTEND_CASES, ids=[f"m{m}_{k}" for m, k in EXTEND_CASES])
def test_extension(ctx, m, kind):
    M, K = m + 1, max(2 * m + 1, 1)
    rng = random.Random(9000 + m)
    if kind == "top":                   # every value l - 1: the largest products and carries
        a, b = [ELL - 1] * M, [ELL - 1] * M
    else:
        a, b = [rng.randrange(ELL) for _ in range(M)], [rng.randrange(ELL) for _ in range(M)]
        if kind == "zero_a":            # f is the zero polynomial: every h the entry writes is 0
            a = [0] * M
    # the tables from the host: a wrong element below is then the extension's own
    fact, ifact = (ctx.upload(_bytes(t)) for t in ref.tables(K))
    d_a, d_b = ctx.upload(_bytes(a)), ctx.upload(_bytes(b))
    n_z = 2 * m + 3
    written = [0, 1, 2] + ([2 + m + 1] if m else []) + [2 + x for x in range(m + 2, 2 * m + 1)]
    want = ref.z_tail_bary(a[:m], b[:m], a[m], b[m])
    assert len(want) == n_z
    runs = []
    for _ in range(2 if (m in (258, 1025) and kind == "random") else 1):
        z = _pattern(ctx, n_z + 1)
        ctx.cs_extend(d_a.ptr, d_b.ptr, m, fact.ptr, ifact.ptr, z.ptr)
        runs.append(_get(ctx, z, n_z + 1))
    got = runs[0]
    assert [got[p] for p in written] == [want[p] for p in written]
    # the gammas' places and the element past the end are not the entry's to write
    assert got[3:3 + m] == [PAT] * m and got[n_z] == PAT
    assert sorted(written + list(range(3, 3 + m))) == list(range(n_z))
    if kind == "zero_a":
        assert all(got[p] == 0 for p in written if p != 1) and got[1] != 0      # g(0) alone is not a value of f or h
    if m <= 12 and kind == "random":
        naive = ref.z_tail_naive(a[:m], b[:m], a[m], b[m])
        assert [got[p] for p in written] == [naive[p] for p in written]
    assert all(r == got for r in runs)          # integer sums in a fixed order: the same bytes every time


# ---- vmpc_fr_cs_triples_dev -----------------------------------------------------------------------------------------------
N_X, G_OFF, M_GATES = 7, 7 + 8, 600          # gamma_offset is not n_x: columns >= n_x are moved, not only shifted by 0
LEVELS = [(0, 257), (257, 513), (513, 600)]  # 257, 256 and 87 gates
N_Z = G_OFF + M_GATES + 3
EMPTY_ROW, ZERO_ROW, LONG_ROW = 3, 5, 550    # gates whose A row is the special one


def _circuit():
    """A, B as [([(col, value)], constant)]: level 0 reads inputs, level 1 inputs and level 0, level 2 all of them.
    TOP: 293 gates of the first two levels whose gamma is l - 1 when every input is l - 1."""
    rng = random.Random(600)
    top0 = list(range(10, 160))                  # level 0: x_i * (l - 1) x_j
    top1 = list(range(300, 443))                 # level 1: gamma of a top0 gate * (l - 1) x_j
    A, B = [None] * M_GATES, [None] * M_GATES

    def row(limit):
        e = [(rng.randrange(limit), rng.choice([rng.randrange(1, ELL), ELL - 1, rng.randrange(1, 5)]))
             for _ in range(rng.randrange(1, 5))]
        return (e, rng.randrange(ELL) if rng.random() < 0.5 else 0)

    for lo, hi in LEVELS:
        for i in range(lo, hi):
            limit = N_X + lo
            A[i], B[i] = row(limit), row(limit)
            if lo:      # a row that reads an input column and a gamma column: both sides of n_x in cs_z_map
                A[i] = (A[i][0] + [(rng.randrange(N_X), rng.randrange(1, ELL)), (N_X + rng.randrange(lo), rng.randrange(1, ELL))],
                        A[i][1])
    for k, i in enumerate(top0):
        A[i], B[i] = ([(k % N_X, 1)], 0), ([((k + 3) % N_X, ELL - 1)], 0)
    for k, i in enumerate(top1):
        A[i], B[i] = ([(N_X + top0[k], 1)], 0), ([(k % N_X, ELL - 1)], 0)
    A[EMPTY_ROW] = ([], rng.randrange(1, ELL))                      # a constant wire
    v = rng.randrange(1, ELL)
    A[ZERO_ROW] = ([(2, v), (4, 1), (2, ELL - v), (4, ELL - 1)], 0)   # v x_2 + x_4 - v x_2 - x_4: a multiple of l, not 0
    # 300 entries on 300 distinct positions, every value l - 1
    A[LONG_ROW] = ([(c, ELL - 1) for c in range(N_X)] + [(N_X + g, ELL - 1) for g in top0 + top1], ELL - 1)
    assert len(A[LONG_ROW][0]) == 300 == len({c for c, _ in A[LONG_ROW][0]})
    return A, B, top0 + top1


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
    A, B, top = _circuit()
    rng = random.Random(601)
    gates = []
    for lo, hi in LEVELS:
        order = list(range(lo, hi))
        rng.shuffle(order)
        assert order != sorted(order)
        gates += order
    xs = {"random": [rng.randrange(ELL) for _ in range(N_X)], "top": [ELL - 1] * N_X}
    want = {k: ref.triples(N_X, A, B, x) for k, x in xs.items()}
    assert all(want["top"][2][g] == ELL - 1 for g in top)       # every z the long row reads is l - 1
    assert want["random"][0][ZERO_ROW] == 0 and want["random"][0][EMPTY_ROW] == A[EMPTY_ROW][1]
    keep_a, csr_a = _csr(ctx, A)
    keep_b, csr_b = _csr(ctx, B)
    return {"A": A, "B": B, "csr_a": csr_a, "csr_b": csr_b, "keep": (keep_a, keep_b), "x": xs, "want": want,
            "gates": ctx.upload(np.array(gates, np.uint32))}


def _z_image(x, gamma):
    return x + [PAT] * (G_OFF - N_X) + gamma + [PAT] * (N_Z - G_OFF - M_GATES)


@pytest.mark.parametrize("kind", ["random", "top"])
def test_triples_level_by_level(ctx, circuit, kind):
    x, (a, b, gamma) = circuit["x"][kind], circuit["want"][kind]
    z = ctx.upload(_bytes(_z_image(x, [PAT] * M_GATES)))
    a_out, b_out = _pattern(ctx, M_GATES + 1), _pattern(ctx, M_GATES + 1)
    for i, (lo, hi) in enumerate(LEVELS):
        ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], circuit["gates"].ptr + 4 * lo, hi - lo, N_X, G_OFF, z.ptr,
                       a_out.ptr, b_out.ptr)
        # what the level wrote and nothing else: the inputs, the gap before the gammas, later levels, the tail
        done = gamma[:hi] + [PAT] * (M_GATES - hi)
        assert _get(ctx, z, N_Z) == _z_image(x, done), i
        assert _get(ctx, a_out, M_GATES + 1) == a[:hi] + [PAT] * (M_GATES + 1 - hi), i
        assert _get(ctx, b_out, M_GATES + 1) == b[:hi] + [PAT] * (M_GATES + 1 - hi), i


def _first_bad(ctx, circuit, z, a_out, b_out):
    bad = ctx.upload(np.array([7], np.uint32))
    ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], None, M_GATES, N_X, G_OFF, z.ptr, a_out.ptr, b_out.ptr, 1, bad.ptr)
    ctx.sync()
    return int(ctx.download(bad.ptr, 4).view(np.uint32)[0])


@pytest.mark.parametrize("spoiled,first", [((), NONE), ((599, 300, 256, 255), 255), ((599,), 599)],
                         ids=["none", "four", "last"])
def test_triples_check_names_the_smallest_bad_gate(ctx, circuit, spoiled, first):
    x, (a, b, gamma) = circuit["x"]["random"], circuit["want"]["random"]
    gamma = list(gamma)
    for i in spoiled:
        gamma[i] = (gamma[i] + 1) % ELL
    image = _z_image(x, gamma)
    z = ctx.upload(_bytes(image))
    a_out, b_out = _pattern(ctx, M_GATES), _pattern(ctx, M_GATES)
    assert _first_bad(ctx, circuit, z, a_out, b_out) == first
    assert _get(ctx, z, N_Z) == image           # the gammas are the caller's: nothing is written to z
    if not spoiled:
        assert _get(ctx, a_out, M_GATES) == a and _get(ctx, b_out, M_GATES) == b


def test_triples_values_only_and_no_gates(ctx, circuit):
    x, (a, b, gamma) = circuit["x"]["random"], circuit["want"]["random"]
    image = _z_image(x, gamma)
    z = ctx.upload(_bytes(image))
    out = _pattern(ctx, M_GATES + 1)
    # check = 2: one matrix as A and as B, one buffer as both outputs, no first_bad
    ctx.cs_triples(circuit["csr_a"], circuit["csr_a"], None, M_GATES, N_X, G_OFF, z.ptr, out.ptr, out.ptr, 2, None)
    assert _get(ctx, out, M_GATES + 1) == [ref.row_eval(r, N_X, x, gamma) for r in circuit["A"]] + [PAT]
    assert _get(ctx, z, N_Z) == image
    # no gates: nothing to do, with no gate list
    for check, bad in ((0, None), (2, None)):
        ctx.cs_triples(circuit["csr_a"], circuit["csr_b"], None, 0, N_X, G_OFF, z.ptr, out.ptr, out.ptr, check, bad)
    assert _get(ctx, z, N_Z) == image and _get(ctx, out, M_GATES + 1)[M_GATES] == PAT


# ---- vmpc_fr_cs_first_diff_dev --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_first_difference(ctx, n):
    rng = np.random.default_rng(n)
    host = rng.integers(0, 256, size=(n + 1, 32), dtype=np.uint8)
    host[:, 31] &= 0x03                          # below 2^250: a bit flipped below leaves a canonical residue
    a, b = ctx.upload(host), ctx.upload(host)

    def flipped(i, byte, bit):
        """first_diff with element i of b changed in one bit; b is restored afterwards"""
        e = host[i].copy()
        e[byte] ^= 1 << bit
        ctx.upload_into(b.ptr + 32 * i, e)
        got = ctx.cs_first_diff(a.ptr, b.ptr, n)
        ctx.upload_into(b.ptr + 32 * i, host[i])
        return got

    assert ctx.cs_first_diff(a.ptr, b.ptr, n) is None
    assert flipped(n, 0, 0) is None              # one past the compared range
    if n == 0:
        assert ctx.cs_first_diff(None, None, 0) is None
        return
    assert flipped(n - 1, 0, 0) == n - 1
    for i in sorted({0, n // 2, n - 1}):
        assert flipped(i, 31, 2) == i            # bit 250: the top limb only
        assert flipped(i, 0, 0) == i             # bit 0: the low limb only
        for limb in range(1, 7):
            assert flipped(i, 4 * limb + 1, 3) == i
    # several differences: the smallest, whatever order the workgroups finish in
    spots = sorted({n - 1, n // 2, n // 3, min(n - 1, 255), min(n - 1, 256)})
    for i in spots:
        e = host[i].copy()
        e[7] ^= 0x10
        ctx.upload_into(b.ptr + 32 * i, e)
    assert ctx.cs_first_diff(a.ptr, b.ptr, n) == spots[0]


# ---- argument contracts (include/vmpc.h) ----------------------------------------------------------------------------------
def test_argument_contracts(ctx, circuit):
    from verifiable_mpc_amd import _native as nat
    lib, h, p = ctx.lib, ctx.handle, ctypes.c_void_p
    # above the cap: VMPC_E_RANGE before any pointer is looked at - the context's included
    assert lib.vmpc_fr_cs_extend_dev(None, None, None, MAX_M + 1, None, None, None) == nat.E_RANGE
    assert lib.vmpc_fr_cs_triples_dev(None, None, None, None, None, None, None, None, None, None, MAX_M + 1, 0, 0, None,
                                      None, None, 0, None) == nat.E_RANGE
    assert lib.vmpc_fr_cs_tables_dev(None, 2 * MAX_M + 2, None, None) == nat.E_RANGE
    assert lib.vmpc_fr_cs_lagrange_dev(None, None, 2 * MAX_M + 2, None, None) == nat.E_RANGE
    assert lib.vmpc_fr_cs_first_diff_dev(None, None, None, (1 << 31) + 1, None) == nat.E_RANGE
    # at the cap itself the null pointers are the complaint
    assert lib.vmpc_fr_cs_extend_dev(h, None, None, MAX_M, None, None, None) == nat.E_INVAL
    assert lib.vmpc_fr_cs_triples_dev(h, None, None, None, None, None, None, None, None, None, MAX_M, 0, 0, None, None,
                                      None, 0, None) == nat.E_INVAL
    assert lib.vmpc_fr_cs_tables_dev(h, 2 * MAX_M + 1, None, None) == nat.E_INVAL
    assert lib.vmpc_fr_cs_lagrange_dev(h, None, 2 * MAX_M + 1, None, None) == nat.E_INVAL
    assert lib.vmpc_fr_cs_first_diff_dev(h, None, None, 1 << 31, None) == nat.E_INVAL
    # K = 0 has no table
    fact, ifact = _pattern(ctx, 2), _pattern(ctx, 2)
    assert lib.vmpc_fr_cs_tables_dev(h, 0, p(fact.ptr), p(ifact.ptr)) == nat.E_INVAL
    assert _get(ctx, fact, 2) == [PAT] * 2 and _get(ctx, ifact, 2) == [PAT] * 2
    # check is 0, 1 or 2, and 1 needs a place for its answer
    x, (_, _, gamma) = circuit["x"]["random"], circuit["want"]["random"]
    z = ctx.upload(_bytes(_z_image(x, gamma)))
    out, bad = _pattern(ctx, M_GATES), ctx.upload(np.array([7], np.uint32))
    ca, cb = [p(v) for v in circuit["csr_a"]], [p(v) for v in circuit["csr_b"]]
    for check, first_bad in ((3, p(bad.ptr)), (-1, p(bad.ptr)), (1, None)):
        assert lib.vmpc_fr_cs_triples_dev(h, *ca, *cb, None, M_GATES, N_X, G_OFF, p(z.ptr), p(out.ptr), p(out.ptr), check,
                                          first_bad) == nat.E_INVAL, check
    assert _get(ctx, out, M_GATES) == [PAT] * M_GATES
    assert int(ctx.download(bad.ptr, 4).view(np.uint32)[0]) == 7
    # c is a canonical residue
    K = 5
    table = _device_ifact(ctx, K)
    lam = _pattern(ctx, K + 1)
    for c in (ELL, 2**256 - 1):
        cb32 = ctypes.create_string_buffer(c.to_bytes(32, "little"), 32)
        assert lib.vmpc_fr_cs_lagrange_dev(h, cb32, K, p(table.ptr), p(lam.ptr)) == nat.E_NONCANON, hex(c)
        assert _get(ctx, lam, K + 1) == [PAT] * (K + 1)
    ctx.cs_lagrange(ELL - 1, K, table.ptr, lam.ptr)             # the largest c that is one
    assert _get(ctx, lam, K + 1) == ref.lagrange_bary(K, ELL - 1)
