"""GPU: Pi_Nullity (verifiable_mpc_amd.nullity, csrc/nullity.hip) against the big-int restatement tests/nullity_ref.py
and the fixture the reference's own nullity.py produced (tests/golden/nullity_ed25519.json).  Everything is integer
arithmetic mod l: bit-exact, no tolerances."""
import ctypes
import random

import numpy as np
import pytest

from tests import nullity_ref as nr
from tests.test_nullity_ref import CASES, IDS, check_nullity_fixture, foreign_inputs
from tests.test_refshape_harness import proj_hex

pytestmark = pytest.mark.gpu

ELL = nr.ELL
hx = lambda v: format(int(v), "x")
SPECIAL = [0, 1, ELL - 1, ELL, 2**256 - 1, 2**255, ELL + 5]       # values a uint8 element may hold, l and above included
S_VALUES = (0, 1, 2, 3, 17)
SHAPES = [(1, 1), (63, 63), (64, 64), (65, 70), (1023, 1023), (4097, 4097)]      # (n, row_stride)


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


def raw_matrix(rng, s, n, stride=None):
    """s rows of `stride` 256-bit values as Python ints: random, with the special values strewn in (always among the
    first columns and the last); returns (ints[s][stride], (s, stride, 32) uint8)"""
    stride = stride or n
    rows = [[rng.randrange(2**256) if rng.random() < 0.5 else rng.randrange(ELL) for _ in range(stride)] for _ in range(s)]
    for i, row in enumerate(rows):
        for k, v in enumerate(SPECIAL):
            row[(i + k) % n] = v
        row[n - 1] = SPECIAL[(i + 4) % len(SPECIAL)]
    raw = b"".join(v.to_bytes(32, "little") for row in rows for v in row)
    return rows, np.frombuffer(raw, np.uint8).reshape(s, stride, 32).copy()


@pytest.fixture(scope="module")
def matrices():
    """one 17-row matrix per shape, made once; the tests read prefixes of it"""
    rng = random.Random(1718)
    return {shape: raw_matrix(rng, 17, *shape) for shape in SHAPES}


def rhos(rng):
    return [0, 1, ELL - 1, rng.randrange(2, ELL - 1)]


def stages(ctx, fn):
    """(fn(), the names of the profile stages that ran inside it)"""
    ctx.profile(True)
    try:
        ctx.profile_read()
        out = fn()
        ctx.sync()
        return out, {name for name, (_, launches) in ctx.profile_read().items() if launches}
    finally:
        ctx.profile(False)


# ---- vmpc_fr_rows_combine_dev -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}_stride{s[1]}")
def test_combine_matches_the_restatement(vm, matrices, shape):
    n, stride = shape
    ctx = vm.get_context()
    rows, arr = matrices[shape]
    buf = ctx.upload(arr)
    rng = random.Random(n)
    for s in S_VALUES:
        forms = [row[:n] for row in rows[:s]]
        for rho in rhos(rng):
            out = vm.ScalarVector.empty(n, ctx)
            ctx.upload_into(out.ptr, np.full((n, 32), 0xAB, np.uint8))
            _, seen = stages(ctx, lambda: ctx.fr_rows_combine(buf.ptr, s, n, stride, rho, out.ptr))
            assert out.to_ints() == nr.combine(forms, rho, n), (s, hx(rho))
            assert "nl_combine_seg" not in seen and (s == 0 or "nl_combine" in seen)


@pytest.mark.parametrize("s", [31, 32, 33, 100, 1000])
def test_combine_tall_shapes_take_the_segmented_path(vm, s):
    """n = 5 columns cannot fill the chip: from s = 32 rows on (two segments of NL_MIN_SEG = 16, csrc/nullity.hip) the
    rows are cut into segments - 33 rows: segments of 17 and 16; 1000 rows: 59 segments, the last one short"""
    n = 5
    ctx = vm.get_context()
    rng = random.Random(s)
    rows, arr = raw_matrix(rng, s, n)
    buf = ctx.upload(arr)
    for rho in rhos(rng):
        out = vm.ScalarVector.empty(n, ctx)
        _, seen = stages(ctx, lambda: ctx.fr_rows_combine(buf.ptr, s, n, n, rho, out.ptr))
        assert ("nl_combine_seg" in seen) == (s >= 32) and ("nl_combine" in seen) == (s < 32)
        assert out.to_ints() == nr.combine(rows, rho), hx(rho)


def test_combine_is_deterministic_and_refuses_what_it_cannot_take(vm):
    ctx = vm.get_context()
    rng = random.Random(5)
    rows, arr = raw_matrix(rng, 200, 7)
    buf = ctx.upload(arr)
    rho = rng.randrange(ELL)
    outs = []
    for _ in range(3):
        out = vm.ScalarVector.empty(7, ctx)
        ctx.fr_rows_combine(buf.ptr, 200, 7, 7, rho, out.ptr)
        outs.append(out.to_ints())
    assert outs[0] == outs[1] == outs[2] == nr.combine(rows, rho)
    native = vm._native
    out = vm.ScalarVector.empty(7, ctx)
    for args in ((buf.ptr, (1 << 16) + 1, 7, 7), (buf.ptr, 2, (1 << 30) + 1, (1 << 30) + 1), (None, 1 << 17, 7, 7)):
        with pytest.raises(native.VmpcError) as ei:
            ctx.fr_rows_combine(args[0], args[1], args[2], args[3], rho, out.ptr)
        assert ei.value.code == native.E_RANGE
    for args, dst in (((None, 2, 7, 7), out.ptr), ((buf.ptr, 2, 7, 7), None), ((buf.ptr, 2, 7, 6), out.ptr)):
        with pytest.raises(native.VmpcError) as ei:
            ctx.fr_rows_combine(args[0], args[1], args[2], args[3], rho, dst)
        assert ei.value.code == native.E_INVAL
    rb = ctypes.create_string_buffer(ELL.to_bytes(32, "little"), 32)
    assert ctx.lib.vmpc_fr_rows_combine_dev(ctx.handle, ctypes.c_void_p(buf.ptr), 2, 7, 7, rb,
                                            ctypes.c_void_p(out.ptr)) == native.E_NONCANON
    assert ctx.lib.vmpc_fr_rows_combine_dev(ctx.handle, ctypes.c_void_p(buf.ptr), 2, 7, 7, None,
                                            ctypes.c_void_p(out.ptr)) == native.E_INVAL
    assert ctx.lib.vmpc_fr_rows_dot_dev(ctx.handle, ctypes.c_void_p(buf.ptr), 2, 7, 7, None, ctypes.c_void_p(out.ptr),
                                        None) == native.E_INVAL
    assert ctx.lib.vmpc_fr_rows_dot_dev(ctx.handle, ctypes.c_void_p(buf.ptr), (1 << 16) + 1, 7, 7, None, None,
                                        None) == native.E_RANGE


# ---- vmpc_fr_rows_dot_dev ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}_stride{s[1]}")
def test_rows_dot_matches_the_restatement(vm, matrices, shape):
    n, stride = shape
    ctx = vm.get_context()
    rows, arr = matrices[shape]
    buf = ctx.upload(arr)
    rng = random.Random(n + 1)
    x = [rng.randrange(ELL) for _ in range(n)]
    x[0], x[n - 1] = ELL - 1, ELL - 1
    xs = vm.ScalarVector.from_ints(x)
    for s in S_VALUES:
        forms = [row[:n] for row in rows[:s]]
        want = nr.values(forms, x)
        out = vm.ScalarVector.empty(s, ctx)
        first = ctx.fr_rows_dot(buf.ptr, s, n, stride, xs.ptr, out.ptr)
        assert out.to_ints() == want, s
        assert first == next((i for i, v in enumerate(want) if v), None)
        assert ctx.fr_rows_dot(buf.ptr, s, n, stride, xs.ptr, out.ptr, want_first=False) is None
        assert out.to_ints() == want


@pytest.mark.parametrize("entry", [ELL - 1, 2**256 - 1], ids=["l_minus_1", "all_ones"])
def test_rows_dot_accumulator_worst_case(vm, entry):
    """every entry and every x_j at l - 1, n = 4097: the largest canonical products; 512 rows, so that the plan
    (csrc/nullity.hip: about 2048 workgroups) cuts the columns into 4 segments of 1280 and a lane adds up to 5
    products with nothing reduced in between.  And the same with every entry 2^256 - 1, the largest a 32-byte element
    can be."""
    n, s = 4097, 512
    ctx = vm.get_context()
    arr = np.tile(np.frombuffer(entry.to_bytes(32, "little"), np.uint8), (s, n, 1))
    buf = ctx.upload(arr)
    xs = vm.ScalarVector.from_ints([ELL - 1] * n)
    out = vm.ScalarVector.empty(s, ctx)
    first = ctx.fr_rows_dot(buf.ptr, s, n, n, xs.ptr, out.ptr)
    assert out.to_ints() == [n * entry * (ELL - 1) % ELL] * s and first == 0
    got = vm.ScalarVector.empty(n, ctx)
    ctx.fr_rows_combine(buf.ptr, 3, n, n, ELL - 1, got.ptr)
    assert got.to_ints() == [entry % ELL] * n          # rho = -1 over three equal rows: entry (1 - 1 + 1)


def vanishing_rows(rng, s, n, x):
    rows = []
    for _ in range(s):
        row = [rng.randrange(ELL) for _ in range(n - 1)]
        acc = sum(c * v for c, v in zip(row, x)) % ELL
        rows.append(row + [-acc * pow(x[-1], ELL - 2, ELL) % ELL])
    return rows


def as_array(rows):
    return np.frombuffer(b"".join((v % ELL).to_bytes(32, "little") for row in rows for v in row),
                         np.uint8).reshape(len(rows), len(rows[0]), 32).copy()


@pytest.mark.parametrize("violator", [0, 5, None], ids=["first", "last", "absent"])
def test_first_nonzero_names_the_form_that_does_not_vanish(vm, violator):
    s, n = 6, 300
    rng = random.Random(66)
    x = [rng.randrange(1, ELL) for _ in range(n)]
    rows = vanishing_rows(rng, s, n, x)
    if violator is not None:
        rows[violator][17] = (rows[violator][17] + 1) % ELL
    fm = vm.FormMatrix(as_array(rows))
    assert fm.first_nonzero(x) == violator == nr.first_nonzero(rows, x)
    assert fm.values(vm.ScalarVector.from_ints(x)) == nr.values(rows, x)
    if violator is not None:        # two violators: the smaller index, whatever order the workgroups finish in
        rows[3][2] = (rows[3][2] + 1) % ELL
        assert vm.FormMatrix(as_array(rows)).first_nonzero(x) == min(violator, 3)


# ---- FormMatrix ---------------------------------------------------------------------------------------------------------------
def test_sparse_and_dense_forms_agree(vm):
    s, n = 9, 40
    rng = random.Random(940)
    row_ptr, col, vals, dense = [0], [], [], [[0] * n for _ in range(s)]
    for i in range(s):
        for _ in range(0 if i == 4 else rng.randrange(1, 12)):          # row 4 is the zero form
            c, v = rng.randrange(n), rng.choice([rng.randrange(-9, 9), rng.randrange(ELL), 2**300 + 7])
            col.append(c)
            vals.append(v)
            dense[i][c] += v                                            # duplicates add
        row_ptr.append(len(col))
    sparse = vm.FormMatrix.from_csr(row_ptr, col, vals, n)
    full = vm.FormMatrix([vm.pivot.LinearForm(list(row)) for row in dense])
    x = [rng.randrange(ELL) for _ in range(n)]
    rho = rng.randrange(ELL)
    assert sparse.combine(rho).to_ints() == full.combine(rho).to_ints() == nr.combine(dense, rho)
    assert sparse.values(x) == full.values(x) == nr.values(dense, x)
    assert sparse.first_nonzero(x) == full.first_nonzero(x) == nr.first_nonzero(dense, x)
    zero_on = [0] * n
    assert sparse.first_nonzero(zero_on) is None and full.first_nonzero(zero_on) is None
    assert full.digest == nr.dense_digest(dense)
    assert sparse.digest == nr.sparse_digest([{j: v for j, v in enumerate(row)} for row in dense], n)
    assert (len(sparse), sparse.n, len(full), full.n) == (s, n, s, n)


def test_form_matrix_constructors_hold_the_same_forms(vm, matrices):
    n, stride = 65, 70
    ctx = vm.get_context()
    rows, arr = matrices[(n, stride)]
    forms = [[v % ELL for v in row[:n]] for row in rows[:5]]
    rng = random.Random(3)
    rho, x = rng.randrange(ELL), [rng.randrange(ELL) for _ in range(n)]
    want = (nr.combine(forms, rho), nr.values(forms, x), nr.dense_digest(forms))
    gf = vm.GF(ELL)
    made = [
        vm.FormMatrix(np.ascontiguousarray(arr[:5, :n])),                                 # values >= l among them
        vm.FormMatrix([vm.pivot.LinearForm(vm.ScalarVector.from_ints(f)) if i % 2 else
                       vm.pivot.AffineForm([gf(c) if j % 2 else c - ELL for j, c in enumerate(f)], 7)
                       for i, f in enumerate(forms)]),
        vm.FormMatrix.from_device(vm.ScalarVector.from_ints([v for row in rows[:5] for v in row]), 5, n, stride),
    ]
    for fm in made:
        assert (fm.combine(rho).to_ints(), fm.values(x), fm.digest) == want
        assert [f.coeffs.to_ints() for f in fm.forms()] == forms
    empty = vm.FormMatrix([], n=4)
    assert empty.combine(rho).to_ints() == [0] * 4 and empty.values([1, 2, 3, 4]) == []
    assert empty.first_nonzero([1, 2, 3, 4]) is None and empty.digest == nr.dense_digest([], 4)
    with pytest.raises(ValueError):
        vm.FormMatrix([vm.pivot.LinearForm([1, 2]), vm.pivot.LinearForm([1])])
    with pytest.raises(ValueError):
        made[0].values([1, 2])


# ---- the protocol ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def record_hashes(vm, monkeypatch):
    calls = []
    one, many = vm.pivot.fiat_shamir_hash, vm.pivot.fiat_shamir_hash_variants
    monkeypatch.setattr(vm.pivot, "fiat_shamir_hash", lambda lst, order: (calls.append(one(lst, order)), calls[-1])[1])
    monkeypatch.setattr(vm.pivot, "fiat_shamir_hash_variants",
                        lambda common, tails, order: (calls.extend(many(common, tails, order)), calls[-len(tails):])[1])
    return calls


def our_inputs(vm, case, monkeypatch):
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    monkeypatch.setattr(vm.circuit_sat, "prng", random.Random(case["seed"] + 1))
    generators = vm.create_generators(case["n"], vm.PivotChoice.compressed, group)
    monkeypatch.setattr(vm.compressed_pivot, "prng", random.Random(case["seed"] + 2))

    def value(t):
        return int(t[2:]) if t[0] == "i" else gf(int(t[2:], 16))
    x = [value(t) for t in case["x_typed"]]
    lin_forms = [vm.pivot.LinearForm([value(t) for t in form]) for form in case["forms_typed"]]
    gamma = int(case["gamma"], 16)
    P = vm.pivot.vector_commitment(x, gamma, generators["g"], generators["h"])
    return generators, P, lin_forms, x, gamma, gf


def coords_hex(pt):
    return [hx(c) for c in pt.coords]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_transcript_list_mode_reproduces_the_fixture(vm, monkeypatch, record_hashes, capsys, case):
    """rho, L (Python ints unreduced where the reference's are), y, every proof element with its representative, every
    hash of prover and verifier, and the verifier's answer"""
    nullity = vm.nullity
    generators, P, lin_forms, x, gamma, gf = our_inputs(vm, case, monkeypatch)
    proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf, transcript="reference")
    ok = nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf, transcript="reference")
    assert ok is case["verified"]
    check_nullity_fixture(case, P, proof, L, y, rho, record_hashes, gf.order, coords=coords_hex)
    assert isinstance(L, vm.pivot.LinearForm) is case["L_is_linear_form"]
    # the masks handed in instead of drawn: the same proof
    again = nullity.prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf, transcript="reference",
                                             r=[int(v, 16) for v in case["r"]], mask=int(case["mask"], 16))
    assert coords_hex(again[0]["A"]) == case["proof"]["A_proj"] and again[3] == rho
    capsys.readouterr()
    if case["s"] > 1:
        assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho + 1, y, proof, gf,
                                                 transcript="reference") is False
        assert capsys.readouterr().out == nullity.MISMATCH + "\n"
    assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho, y + 1, proof, gf,
                                             transcript="reference") is False


@pytest.mark.parametrize("case", [c for c in CASES if c["name"].endswith(("field", "nonzero"))],
                         ids=[i for i in IDS if i.endswith(("field", "nonzero"))])
def test_reference_transcript_device_forms(vm, monkeypatch, case):
    """device coefficients print as the field elements the fixture's forms hold: the same rho, L from the kernel"""
    nullity = vm.nullity
    generators, P, lin_forms, x, gamma, gf = our_inputs(vm, case, monkeypatch)
    fm = vm.FormMatrix(lin_forms)
    for forms in (fm, fm.forms()):
        proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, forms, x, gamma, gf, transcript="reference")
        assert hx(rho) == case["rho"] and isinstance(L.coeffs, vm.ScalarVector)
        assert [hx(v) for v in L.coeffs.to_ints()] == [t[2:] for t in case["L_typed"]]
        assert "f:" + hx(int(y) % ELL) == case["y_typed"]
        assert nullity.verify_nullity_compressed(generators, P, L, forms, rho, y, proof, gf, transcript="reference") is True
    assert fm.first_nonzero(x) == (1 if case["name"] == "3x7_field_nonzero" else None)


def test_compact_transcript_prove_verify_and_tampering(vm, capsys):
    s, n = 5, 1023
    nullity = vm.nullity
    rng = random.Random(51023)
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    exps = [rng.randrange(1, ELL) for _ in range(n)]
    generators = {"g": vm.PointVector.fixed_base(group.generator, exps, keep_proj=False), "h": group.generator,
                  "k": vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ELL))}
    x = [rng.randrange(1, ELL) for _ in range(n)]
    rows = vanishing_rows(rng, s, n, x)
    xs = vm.ScalarVector.from_ints(x)
    gamma = rng.randrange(1, ELL)
    P = vm.pivot.vector_commitment(xs, gamma, generators["g"], generators["h"])
    fm = vm.FormMatrix(as_array(rows))
    assert fm.first_nonzero(xs) is None
    proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, fm, xs, gamma, gf)        # compact by default
    assert rho == nr.compact_rho(P.coords, nr.dense_digest(rows)) and int(y) == 0
    assert isinstance(L.coeffs, vm.ScalarVector) and L.coeffs.to_ints() == nr.combine(rows, rho)
    assert nullity.verify_nullity_compressed(generators, P, L, fm, rho, y, proof, gf) is True
    assert nullity.verify_nullity_compressed(generators, P, L, as_array(rows), rho, y, proof, gf, transcript="compact") is True
    capsys.readouterr()
    # one coefficient of one form changed: another digest, so another rho
    other = [list(r) for r in rows]
    other[3][511] = (other[3][511] + 1) % ELL
    assert nullity.verify_nullity_compressed(generators, P, L, vm.FormMatrix(as_array(other)), rho, y, proof, gf) is False
    # rho changed
    assert nullity.verify_nullity_compressed(generators, P, L, fm, (rho + 1) % ELL, y, proof, gf) is False
    # L replaced: by another form's combination, and by one that differs in its last coefficient only
    capsys.readouterr()
    for bad in (fm.combine(rho + 1), vm.ScalarVector.from_ints(L.coeffs.to_ints()[:-1] + [5])):
        assert nullity.verify_nullity_compressed(generators, P, vm.pivot.LinearForm(bad), fm, rho, y, proof, gf) is False
        assert capsys.readouterr().out == nullity.MISMATCH + "\n"
    # y changed
    assert nullity.verify_nullity_compressed(generators, P, L, fm, rho, y + 1, proof, gf) is False
    # and a form that does not vanish is proved as it is (y != 0), like the reference does
    other_fm = vm.FormMatrix(as_array(other))
    assert other_fm.first_nonzero(xs) == 3
    proof2, L2, y2, rho2 = nullity.prove_nullity_compressed(generators, P, other_fm, xs, gamma, gf)
    assert int(y2) % ELL == pow(rho2, 3, ELL) * x[511] % ELL != 0       # (int() of a field element is signed)
    assert nullity.verify_nullity_compressed(generators, P, L2, other_fm, rho2, y2, proof2, gf) is True
    assert nullity.verify_nullity_compressed(generators, P, L2, other_fm, rho2, gf(0), proof2, gf) is False


# ---- the drop-in ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_installed_nullity_reproduces_the_fixture_from_foreign_types(vm, refshape, monkeypatch, record_hashes, case):
    """install() rebinds the two names of the (stand-in) reference's nullity module; called the reference's way, with
    the stand-in's forms, the shim's field elements and points, they give what the reference's own module gave"""
    from tests.refshape.ac20 import nullity
    rs = refshape
    patched = vm.install(rs.package)
    assert f"{rs.package}.nullity.prove_nullity_compressed" in patched
    assert f"{rs.package}.nullity.verify_nullity_compressed" in patched
    generators, P, lin_forms, x, gamma, gf = foreign_inputs(rs, nullity, case)
    assert isinstance(generators["g"], vm.PointVector)          # the installed create_generators ran
    assert not isinstance(lin_forms[0], vm.pivot.AffineForm) and not isinstance(x[-1], (int, vm.fields.FiniteFieldElement))
    proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf)
    assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf) is case["verified"]
    assert isinstance(proof["A"], vm.Ed25519Point) and isinstance(L, rs.pivot.AffineForm)
    check_nullity_fixture(case, P, proof, L, y, rho, record_hashes, gf.order,
                          coords=lambda pt: coords_hex(pt) if isinstance(pt, vm.Ed25519Point) else proj_hex(pt))
    vm.uninstall(rs.package)
    assert not hasattr(nullity.prove_nullity_compressed, "__vmpc_accelerated__")


def test_installed_nullity_leaves_other_groups_to_the_original(vm, refshape):
    """QuadraticResidues after install(): the stand-in's own functions run, plain lists and QR elements throughout"""
    from tests.refshape.ac20 import nullity
    rs = refshape
    vm.install(rs.package)
    assert nullity.verify_nullity_compressed.__vmpc_original__ is not None
    group, gf = rs.demo.group_and_field("QR")
    rng = random.Random(12)
    for i, mod in enumerate((rs.r1cs, rs.compressed_pivot)):
        mod.prng = random.Random(40 + i)
    generators = rs.r1cs.create_generators(3, rs.cs.PivotChoice.compressed, group)
    x = [gf(rng.randrange(1, gf.order)) for _ in range(3)]
    lin_forms = []
    for _ in range(2):
        a, b = gf(rng.randrange(gf.order)), gf(rng.randrange(gf.order))
        lin_forms.append(rs.pivot.LinearForm([a, b, -(a * x[0] + b * x[1]) / x[2]]))
    gamma = rng.randrange(1, gf.order)
    P = rs.pivot.vector_commitment(x, gamma, generators["g"], generators["h"])
    proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf)
    assert isinstance(generators["g"], list) and not isinstance(proof["A"], vm.Ed25519Point) and int(y) == 0
    assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf) is True
    assert nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho + 1, y, proof, gf) is False
