"""Commitments over every form of generator vector that k_msm_bucket and its siblings read 128-byte table lines from
(csrc/ptio.h niels_ld_line / niels_st_line), bit-exact on the affine bytes against the C restatement of the reference
algorithm (oracle.c_oracle.vector_commitment: one ladder per term, product tree; pivot.py:139-145).

Forms: plain points (vmpc_msm_dev, k_msm_prep writes the lines), the one-row prepared form, 2- / 4- / 16-row tables
(the 16-row one through the fused short path and through the general pipeline) and the 13-row wide-window table,
forced at small n the way tests/test_gpu_wide_table.py forces it.  Sizes on both sides of the 8-entry burst and of the
32-entry staging window of the sorted indices; scalars uniform, all zero, all l - 1, one repeated digit.  The
generators begin with the points whose table entries are special: the neutral element (0, 1), (0, -1), the two points
of order 4, the base point and its negative, and another point with its negative.

Also: three scalar vectors in one pass (msm_table_batch), a Protocol-5 proof over a tabulated CRS at N = 64 (the fold
jump and the prover's round context read and write the same lines), and runs of more than 32 entries in ONE task under
64-entry segments (all scalars equal), which take the 32-entry burst of 16-byte index loads (msm_idx_fill16) and its
refill, at whatever alignment the run starts.

The wide-window table recodes s + k l instead of s for scalars from 2^240 up, k chosen by the column
(k_msm_recode_wide; tests/msm_sort_ref.py wide_k restates it).  That is the same exponent on a point of order l and a
different one on the three generators of order 2 and 4, so over the wide table the expected point is the oracle's plus
(k l mod 4) times each of those three: the same generators and scalars as in every other form."""
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import ed25519_ref as ed
from tests.msm_sort_ref import wide_k
from tests.test_gpu_bucket_runs import make_ctx
from tests.test_gpu_wide_table import stages

pytestmark = pytest.mark.gpu
ELL, P = ed.ELL, ed.P
WIDE = 13
N_MAX = 300
SIZES = [1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 300]
KINDS = ["uniform", "zero", "ell_minus_1", "repeated_digit"]
FORMS = ["msm", "rows1", "rows2", "rows4", "rows16_short", "rows16", "wide"]
ZERO32 = np.zeros(32, np.uint8)


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    n, info = _native.backend_info()
    assert n >= 1, info
    return _native


def special_points():
    sqrt_m1 = pow(2, (P - 1) // 4, P)
    assert sqrt_m1 * sqrt_m1 % P == P - 1
    q = ed.pt_affine(ed.pt_repeat(ed.BASE, 0x1234567))
    base = ed.pt_affine(ed.BASE)
    pts = [(0, 1), (0, P - 1), (sqrt_m1, 0), (P - sqrt_m1, 0), base, (P - base[0], base[1]), q, (P - q[0], q[1])]
    assert all(ed.on_curve((x, y, 1)) for x, y in pts)
    return pts


def scalar_bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)


@pytest.fixture(scope="module")
def case():
    """generators (host bytes), the scalar vectors of every kind and the oracle's commitment to every (kind, size)
    prefix: computed once, read by every form"""
    rng = random.Random(9696)
    special = special_points()
    sb = np.frombuffer(b"".join(ed.affine_to_bytes((x, y, 1)) for x, y in special), np.uint8).reshape(-1, 64)
    base_proj = np.frombuffer(ed.proj_to_bytes(ed.BASE), np.uint8)
    _, rest = c_oracle.fixed_base(base_proj, scalar_bytes([rng.randrange(1, ELL) for _ in range(N_MAX - len(special))]))
    pts = np.ascontiguousarray(np.concatenate([sb, rest]))
    digit = sum(0x1234 << (16 * i) for i in range(15)) + (0x0234 << 240)        # 0x1234 in every 16-bit window but the top
    assert digit < ELL
    scalars = {"uniform": scalar_bytes([rng.randrange(ELL) for _ in range(N_MAX)]),
               "zero": scalar_bytes([0] * N_MAX),
               "ell_minus_1": scalar_bytes([ELL - 1] * N_MAX),
               "repeated_digit": scalar_bytes([digit] * N_MAX)}
    want = {(kind, n): bytes(c_oracle.vector_commitment(scalars[kind][:n], ZERO32, pts[:n], pts[0])[1])
            for kind in KINDS for n in SIZES}
    assert want[("zero", 300)] == ed.affine_to_bytes((0, 1, 1))
    # over the wide table: columns 1 .. 3 hold the points of order 2 and 4
    want_wide = {}
    for (kind, n), raw in want.items():
        pt = ed.affine_from_bytes(raw)
        for i in range(1, min(n, 4)):
            s_i = int.from_bytes(scalars[kind][i].tobytes(), "little")
            pt = ed.pt_add(pt, ed.pt_repeat(special[i] + (1,), wide_k(s_i, i) * ELL % 4))
        want_wide[(kind, n)] = ed.affine_to_bytes(pt)
    assert any(want_wide[key] != want[key] for key in want) and want_wide[("zero", 300)] == want[("zero", 300)]
    return pts, scalars, want, want_wide


def commit(ctx, form, tables, dp, ds, n, n_table, out):
    if form == "msm":
        ctx.msm(ds.ptr, dp.ptr, n, None, None, 0, None, out.ptr)
        return
    rows = WIDE if form == "wide" else int(form[4:].split("_")[0])
    ctx.set_short_path(form == "rows16_short")
    ctx.msm_table(tables[rows].ptr, n_table, 0, ds.ptr, n, None, None, out.ptr, rows)


@pytest.mark.parametrize("form", FORMS)
def test_commitments_bit_exact(nat, case, form):
    pts, scalars, want, want_wide = case
    want = want_wide if form == "wide" else want
    ctx = nat.Context(0)
    try:
        dp = ctx.upload(pts)
        out = ctx.alloc(64)
        dss = {kind: ctx.upload(scalars[kind]) for kind in KINDS}
        for n in SIZES:
            # a table of exactly n columns (its padding columns and row stride change with n), and for the largest
            # size also prefixes of it
            rows = None if form == "msm" else (WIDE if form == "wide" else int(form[4:].split("_")[0]))
            tables = {rows: ctx.msm_table_build(dp.ptr, n, None, 0, rows)} if rows else {}
            for kind in KINDS:
                commit(ctx, form, tables, dp, dss[kind], n, n, out)
                ctx.sync()
                assert ctx.download(out.ptr, 64).tobytes() == want[(kind, n)], (form, kind, n)
            if n == N_MAX and rows:
                for m in (33, 65):
                    commit(ctx, form, tables, dp, dss["uniform"], m, n, out)
                    ctx.sync()
                    assert ctx.download(out.ptr, 64).tobytes() == want[("uniform", m)], (form, "prefix", m)
    finally:
        ctx.close()


@pytest.mark.parametrize("rows", [1, 16, WIDE])
def test_batch_of_three(nat, case, rows):
    pts, scalars, want, want_wide = case
    want = want_wide if rows == WIDE else want
    ctx = nat.Context(0)
    try:
        ctx.set_short_path(False)
        dp = ctx.upload(pts)
        out = ctx.alloc(64 * 3)
        kinds = ["uniform", "repeated_digit", "ell_minus_1"]
        dss = [ctx.upload(scalars[kind]) for kind in kinds]
        for n in (9, 65, 300):
            table = ctx.msm_table_build(dp.ptr, n, None, 0, rows)
            ctx.msm_table_batch(table.ptr, n, 0, [d.ptr for d in dss], n, None, None, out.ptr, rows)
            ctx.sync()
            raw = ctx.download(out.ptr, 64 * 3).tobytes()
            assert [raw[64 * k:64 * k + 64] for k in range(3)] == [want[(kind, n)] for kind in kinds], (rows, n)
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["msm", "rows1", "rows16", "wide"])
def test_one_bucket_beyond_the_staging_window(nat, monkeypatch, case, form):
    """64-entry segments and all scalars equal: every bucket that is hit holds all n entries (of one row, or of all
    rows), so a task is a run of 33 - 64 entries: one 32-entry burst and a refill.  n = 33, 64, 65, 300."""
    pts, scalars, want, want_wide = case
    want = want_wide if form == "wide" else want
    ctx = make_ctx(nat, monkeypatch, True)
    try:
        dp = ctx.upload(pts)
        out = ctx.alloc(64)
        for kind in ("repeated_digit", "ell_minus_1"):
            ds = ctx.upload(scalars[kind])
            for n in (33, 64, 65, 300):
                rows = None if form == "msm" else (WIDE if form == "wide" else int(form[4:]))
                tables = {rows: ctx.msm_table_build(dp.ptr, n, None, 0, rows)} if rows else {}
                st = stages(ctx, lambda: commit(ctx, form, tables, dp, ds, n, n, out))
                assert "msm_bucket" in st and "short_bins" not in st, (form, st)
                assert ctx.download(out.ptr, 64).tobytes() == want[(kind, n)], (form, kind, n)
    finally:
        ctx.close()


def test_protocol_5_over_a_tabulated_crs(nat, monkeypatch):
    """N = 64 (63 generators and the appended element) over a 16-row table of g with h and k as extras: the
    commitment, the fold jump (reads the table, writes the folded vector's table; brought down to this size by its two
    knobs) and the rounds; the proof is the proof of the table-free CRS and verifies"""
    import verifiable_mpc_amd as vm
    monkeypatch.setenv("VMPC_P4_JUMP", "3")
    monkeypatch.setenv("VMPC_P4_JUMP_MIN_LOG2", "3")
    rng = random.Random(6464)
    n = 63                      # the prover appends one element: N = 64
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    h, k = group.generator, vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ELL))
    exps = [rng.randrange(1, ELL) for _ in range(n)]
    x = [rng.randrange(ELL) for _ in range(n)]
    coeffs = [rng.randrange(ELL) for _ in range(n)]
    r = [rng.randrange(ELL) for _ in range(n)]
    proofs = []
    for rows in (None, 16):
        g = vm.PointVector.fixed_base(h, exps, keep_proj=False)
        if rows:
            g.precompute([h, k], rows=rows)
            assert g._table.rows == rows
        gens = {"g": g, "h": h, "k": k}
        xs, L = vm.ScalarVector.from_ints(x), vm.pivot.LinearForm(vm.ScalarVector.from_ints(coeffs))
        Pc = vm.pivot.vector_commitment(xs, 99, g, h)
        y = gf(L(xs))
        g.ctx.profile(True)
        g.ctx.profile_read(reset=True)
        proof = vm.compressed_pivot.protocol_5_prover(gens, Pc, L, y, xs, 99, gf, transcript="compact", r=list(r), rho=7)
        st = {name for name, (_, cnt) in g.ctx.profile_read(reset=True).items() if cnt}
        g.ctx.profile(False)
        assert ("table_fold" in st) == bool(rows), st
        assert vm.compressed_pivot.protocol_5_verifier(gens, Pc, L, y, proof, gf, transcript="compact") is True
        proofs.append({key: (v.to_affine_bytes() if hasattr(v, "to_affine_bytes") else [int(e) for e in v]
                             if isinstance(v, list) else int(v)) for key, v in proof.items()})
        proofs[-1]["P"] = Pc.to_affine_bytes()
    assert proofs[0] == proofs[1]
    # the commitment itself against the oracle
    _, garr = c_oracle.fixed_base(np.frombuffer(ed.proj_to_bytes(ed.BASE), np.uint8), scalar_bytes(exps))
    _, want = c_oracle.vector_commitment(scalar_bytes(x), scalar_bytes([99])[0], garr,
                                         np.frombuffer(ed.affine_to_bytes(ed.BASE), np.uint8))
    assert proofs[1]["P"] == bytes(want)
