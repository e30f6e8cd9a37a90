"""The moment transform by the subproduct tree (csrc/bn256_qap_mtree.hip, device.moment_transform) against the direct
kernel's bytes: the primitive through the C ABI at every geometry edge (against the big-integer definition of
tests/moments_tree_ref.py where d n_out is small, against bn256_qap_moments on the device otherwise), the batch with
strides, an arena group boundary, the errors, every caller of _h_rows under "tree" against the default, launch counts
and the mode's plumbing.  Every comparison is exact."""
import random
import types

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import h_ref as H
from tests import keygen_ref as K
from tests import moments_tree_ref as R
from tests.conftest import load_golden
from tests.test_gpu_pinocchio_h import ALL_TRUE, _case_inputs, _gen, _qaps, _scale_circuit, to_ints

pytestmark = pytest.mark.gpu
N = bn.N
S = R.S_MAX
CPU_LIMIT = 1 << 21          # d n_out up to which the definition on Python ints is the reference
TREE_STAGES = ("bn_qap_mtree_nleaf", "bn_qap_mtree_level", "bn_qap_mtree_reverse")
BUILD_STAGES = ("bn_qap_mtree_tleaf", "bn_qap_mtree_dseries", "bn_qap_mtree_newton")


@pytest.fixture(scope="module")
def vm():
    import verifiable_mpc_amd as v
    v.get_context()
    return v


@pytest.fixture(scope="module")
def ctx(vm):
    return vm.get_context()


@pytest.fixture(scope="module")
def pn(vm):
    return vm.pynocchio


@pytest.fixture(scope="module")
def nat(vm):
    return vm._native


@pytest.fixture(scope="module")
def fx():
    return load_golden("pinocchio_keygen.json")["cases"]


def launches(ctx, fn):
    """stage name -> launches recorded while fn() ran"""
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        fn()
        ctx.sync()
        return {k: v[1] for k, v in ctx.profile_read(reset=True).items() if v[1]}
    finally:
        ctx.profile(False)


_PLANS = {}


def plan_of(ctx, nat, d, n_max):
    if (d, n_max) not in _PLANS:
        buf = ctx.alloc(nat.bn256_qap_mtree_bytes(d, n_max))
        ctx.bn256_qap_mtree_build(d, n_max, buf.ptr)
        _PLANS[d, n_max] = buf
    return _PLANS[d, n_max]


def tree(ctx, nat, d, n_out, u0, u1=None, n_max=None):
    """the tree entry on one witness -> the bytes of out0 (and out1)"""
    n_max = n_out if n_max is None else n_max
    plan = plan_of(ctx, nat, d, n_max)
    d0, d1 = ctx.upload(u0), (None if u1 is None else ctx.upload(u1))
    o0, o1 = ctx.alloc(32 * n_out), (None if u1 is None else ctx.alloc(32 * n_out))
    scratch = ctx.alloc(nat.bn256_qap_moments_tree_scratch_bytes(d, 1))
    ctx.bn256_qap_moments_tree_batch(plan.ptr, d, n_max, d0.ptr, None if u1 is None else d1.ptr, d, n_out, o0.ptr,
                                     None if u1 is None else o1.ptr, n_out, scratch.ptr, 1)
    ctx.sync()
    got = [ctx.download(o0.ptr, 32 * n_out).tobytes()]
    if u1 is not None:
        got.append(ctx.download(o1.ptr, 32 * n_out).tobytes())
    return got


def direct(ctx, d, n_out, u0, u1=None):
    d0, d1 = ctx.upload(u0), (None if u1 is None else ctx.upload(u1))
    o0, o1 = ctx.alloc(32 * n_out), (None if u1 is None else ctx.alloc(32 * n_out))
    ctx.bn256_qap_moments(d0.ptr, None if u1 is None else d1.ptr, d, n_out, o0.ptr, None if u1 is None else o1.ptr)
    ctx.sync()
    got = [ctx.download(o0.ptr, 32 * n_out).tobytes()]
    if u1 is not None:
        got.append(ctx.download(o1.ptr, 32 * n_out).tobytes())
    return got


def reference(ctx, d, n_out, u0, u1=None):
    """the definition on Python ints where that is quick, the direct kernel otherwise"""
    if d * n_out <= CPU_LIMIT:
        return [K.to_array(R.moments(to_ints(u), n_out)).tobytes() for u in (u0, u1) if u is not None]
    return direct(ctx, d, n_out, u0, u1)


SHAPES = [(d, d) for d in (1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 4 * S + 1, 1000, 4097)] + \
    [(300, 300), (700, 1400), (4097, 8)]


# ---- the primitive ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,n_out", SHAPES)
def test_primitive_random_unreduced_and_all_n_minus_1(ctx, nat, d, n_out):
    rnd = np.random.default_rng(d + n_out).integers(0, 256, size=(d, 32), dtype=np.uint8)   # any 32-byte values
    top = K.to_array([N - 1] * d)
    want = reference(ctx, d, n_out, rnd, top)
    assert tree(ctx, nat, d, n_out, rnd, top) == want
    assert tree(ctx, nat, d, n_out, rnd) == want[:1]                 # u1 NULL: one vector


@pytest.mark.parametrize("d,n_out", SHAPES)
def test_primitive_zero_and_single_entries(ctx, nat, d, n_out):
    zero = np.zeros((d, 32), np.uint8)
    first, last = zero.copy(), zero.copy()
    first[0] = K.to_array([N - 2])[0]                                # the one nonzero entry at j = 1
    last[d - 1] = K.to_array([0x1234567 << 200])[0]                  # at j = d, the last point of a padded leaf
    assert tree(ctx, nat, d, n_out, zero) == [bytes(32 * n_out)]
    got = tree(ctx, nat, d, n_out, first, last)
    assert got[0] == K.to_array([N - 2] * n_out).tobytes()           # 1^k
    want_last = [(0x1234567 << 200) * pow(d, k, N) % N for k in range(n_out)]
    assert got[1] == K.to_array(want_last).tobytes()


def test_primitive_at_2_16_against_the_direct_kernel(ctx, nat):
    d = 1 << 16
    rng = np.random.default_rng(16)
    u0, u1 = (rng.integers(0, 256, size=(d, 32), dtype=np.uint8) for _ in range(2))
    assert tree(ctx, nat, d, d, u0, u1) == direct(ctx, d, d, u0, u1)


def test_n_out_below_the_plans_n_max(ctx, nat):
    d, n_max = 300, 300
    u = np.random.default_rng(5).integers(0, 256, size=(d, 32), dtype=np.uint8)
    full = tree(ctx, nat, d, n_max, u)[0]
    for n_out in (1, 7, 299):
        assert tree(ctx, nat, d, n_out, u, n_max=n_max)[0] == full[:32 * n_out]


# ---- the batch ------------------------------------------------------------------------------------------------------------

def _batch(ctx, nat, d, n_out, k, us, u_stride, out_stride, two=True):
    """k rows `stride` scalars apart in sentinel-filled buffers -> the two output buffers as uint8 (k, out_stride, 32)"""
    plan = plan_of(ctx, nat, d, n_out)
    hu = [np.full((k, u_stride, 32), 0xA5, np.uint8) for _ in range(2)]
    for v in range(2):
        for w in range(k):
            hu[v][w, :d] = us[v][w]
    du = [ctx.upload(h) for h in hu]
    outs = [ctx.upload(np.full((k, out_stride, 32), 0x5A, np.uint8)) for _ in range(2)]
    scratch = ctx.alloc(nat.bn256_qap_moments_tree_scratch_bytes(d, k))
    ctx.bn256_qap_moments_tree_batch(plan.ptr, d, n_out, du[0].ptr, du[1].ptr if two else None, u_stride, n_out,
                                     outs[0].ptr, outs[1].ptr if two else None, out_stride, scratch.ptr, k)
    ctx.sync()
    return [ctx.download(o.ptr, 32 * k * out_stride).reshape(k, out_stride, 32) for o in outs]


def _rows(d, k, seed):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 256, size=(d, 32), dtype=np.uint8) for _ in range(k)] for _ in range(2)]


def test_batch_with_strides_and_sentinels(ctx, nat):
    d, n_out, k = 2 * S + 1, 2 * S + 1, 3
    us = _rows(d, k, 21)
    got = _batch(ctx, nat, d, n_out, k, us, d + 5, n_out + 3)
    for v in range(2):
        for w in range(k):
            assert got[v][w, :n_out].tobytes() == tree(ctx, nat, d, n_out, us[v][w])[0], (v, w)
        assert (got[v][:, n_out:] == 0x5A).all()                     # beyond a row's length: never written


def test_arena_group_boundary_changes_no_byte(ctx, nat):
    d, k = 4 * S + 1, 3
    us = _rows(d, k, 22)
    whole = _batch(ctx, nat, d, d, k, us, d, d)
    one = launches(ctx, lambda: _batch(ctx, nat, d, d, k, us, d, d))
    # a level's residues of ONE witness and a little: every witness its own group
    cap = nat.bn256_qap_moments_tree_batch_bytes(d, d, 1) + 4096
    assert cap < nat.bn256_qap_moments_tree_batch_bytes(d, d, k)
    ctx.set_ntt_arena_cap(cap)
    try:
        cut = _batch(ctx, nat, d, d, k, us, d, d)
        seen = launches(ctx, lambda: _batch(ctx, nat, d, d, k, us, d, d))
    finally:
        ctx.set_ntt_arena_cap(0)
    assert all((a == b).all() for a, b in zip(whole, cut))
    assert seen["bn_qap_mtree_nleaf"] > one["bn_qap_mtree_nleaf"] == 1, (one, seen)
    assert whole[0][0].tobytes() == reference(ctx, d, d, us[0][0])[0]


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_errors(ctx, nat):
    cap = nat.BN256_FR_POLY_MAX
    calls = [lambda: ctx.bn256_qap_moments_tree_batch(0, 8, 8, 0, 0, 8, 9, 0, 0, 9, 0, 1),          # n_out > n_max
             lambda: ctx.bn256_qap_moments_tree_batch(0, cap, 8, 0, 0, cap, 8, 0, 0, 8, 0, 1),      # d above the cap
             lambda: ctx.bn256_qap_moments_tree_batch(0, 8, cap + 1, 0, 0, 8, 8, 0, 0, 8, 0, 1),    # n_max above it
             lambda: ctx.bn256_qap_mtree_build(cap, 8, 0), lambda: ctx.bn256_qap_mtree_build(8, cap + 1, 0)]
    for call in calls:
        with pytest.raises(nat.VmpcError) as ei:
            call()
        assert ei.value.code == nat.E_RANGE
    with pytest.raises(nat.VmpcError) as ei:
        ctx.bn256_qap_moments_tree_batch(0, cap - 1, 8, 0, 0, cap - 1, 8, 0, 0, 8, 0, 1)            # at the cap: NULL
    assert ei.value.code == nat.E_INVAL
    assert nat.bn256_qap_mtree_bytes(cap, 8) == 0 and nat.bn256_qap_moments_tree_scratch_bytes(cap, 1) == 0
    for d, n_max in ((1, 1), (129, 129), (1000, 2000)):
        assert nat.bn256_qap_mtree_bytes(d, n_max) == 32 * R.plan_scalars(d, n_max)[3]
        assert nat.bn256_qap_moments_tree_scratch_bytes(d, 3) == 32 * R.scratch_scalars(d, 3)


# ---- through the public interface ---------------------------------------------------------------------------------------

def fresh_qap(pn, built):
    V, W, Y, out_ix, m, _ = built
    return pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), out_ix, m=m)


def deltas_of(seed):
    rng = random.Random(seed)
    return types.SimpleNamespace(v=rng.randrange(N), w=rng.randrange(N), y=rng.randrange(N))


def both(vm, fn):
    """fn() under the default and under "tree" """
    want = fn()
    with vm.device.moment_transform("tree"):
        got = fn()
    return want, got


@pytest.mark.parametrize("form", ["dense", "r1cs"])
def test_compute_h_on_the_fixture(vm, pn, fx, form):
    for case in fx:
        c, deltas = _case_inputs(case)
        qap = _qaps(pn, case)[form]
        want, got = both(vm, lambda: (pn.compute_h(qap, c, deltas).coeffs, pn.compute_h(qap, c).coeffs))
        assert got == want and len(got[0]) == case["d"] + 1 and len(got[1]) == case["d"] - 1, (case["name"], form)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 127, 128, 129, 257, 1000])
def test_compute_h_on_random_r1cs(vm, ctx, pn, d):
    built = H.satisfiable_r1cs(d, seed=600 + d)
    c, dl = built[5], deltas_of(d)
    qap = fresh_qap(pn, built)
    want = (pn.compute_h(qap, c).coeffs, pn.compute_h(qap, c, dl).coeffs)
    got = []
    with vm.device.moment_transform("tree"):
        seen = launches(ctx, lambda: got.append((pn.compute_h(qap, c).coeffs, pn.compute_h(qap, c, dl).coeffs)))
    assert got == [want] and len(want[0]) == max(d - 1, 0) and len(want[1]) == d + 1
    assert "bn_qap_moments" not in seen and seen.get("bn_qap_mtree_nleaf") == 2, seen


def test_compute_h_batch_and_shares(vm, pn):
    d, k = 257, 3
    built = H.satisfiable_r1cs(d, seed=99)
    qap = fresh_qap(pn, built)
    cs, dl = [built[5]] * k, [deltas_of(40 + w) for w in range(k)]
    rng = random.Random(98)
    shares = [[rng.randrange(N) for _ in range(len(built[5]))] for _ in range(k)]   # no satisfying witness: no check
    want, got = both(vm, lambda: (
        [h.coeffs for h in pn.compute_h_batch(qap, cs)], [h.coeffs for h in pn.compute_h_batch(qap, cs, dl)],
        pn.compute_h_share(qap, shares[0]).coeffs, pn.compute_h_share(qap, shares[1], dl[1]).coeffs,
        [h.coeffs for h in pn.compute_h_share_batch(qap, shares, dl)]))
    assert got == want
    assert len(got[1]) == k and len(got[1][0]) == d + 1 and len(got[2]) == d - 1 and len(got[4][2]) == d + 1
    assert got[4][0] != got[4][1]


def test_verified_proof_from_a_tree_made_h_at_2_14(vm, pn):
    d = 1 << 14
    V, W, Y, out_ix, m, c, a, b, y = _scale_circuit(d, seed=79)
    qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
    r = random.Random(15)
    td = K.TD(*(r.randrange(N) for _ in range(8)))
    gen = _gen(pn, td)
    key = pn.PreparedKey.generate(td, qap, gen)
    dl = types.SimpleNamespace(v=r.randrange(N), w=r.randrange(N), y=r.randrange(N))
    with vm.device.moment_transform("tree"):
        h = pn.compute_h(qap, c, dl)
    assert any(h.coeffs)
    proof = pn.compute_proof(qap, c, h, key, dl)
    assert pn.verify(qap, pn.generate_verikey(td, qap, gen), proof, to_ints(c[:out_ix + 1])) == ALL_TRUE


def test_violated_witness_still_raises(vm, pn, fx):
    case = fx[1]
    qap = _qaps(pn, case)["r1cs"]
    c, deltas = _case_inputs(case)
    wire = list(qap.indices_mid)[len(qap.indices_mid) // 2]
    c[wire] = (c[wire] + 1) % N
    a, b, y = (H.row_values(case["r1cs"][k], c) for k in "VWY")
    first = min(j for j in range(case["d"]) if (a[j] * b[j] - y[j]) % N) + 1
    for mode in ("direct", "tree"):
        with vm.device.moment_transform(mode):
            with pytest.raises(ValueError, match=rf"constraint {first} "):
                pn.compute_h(qap, c, deltas)


# ---- launch counts ------------------------------------------------------------------------------------------------------

def _tree_counts(seen):
    return {k: v for k, v in seen.items() if k.startswith("bn_qap_mtree_")}


def test_launch_counts_depend_on_levels_only(vm, ctx, pn):
    seen = {}
    with vm.device.moment_transform("tree"):
        for d in (4 * S + 1, 6 * S):                     # both L = 3
            assert R.geometry(d)[1] == 3
            built = H.satisfiable_r1cs(d, seed=700 + d)
            qap, c = fresh_qap(pn, built), built[5]
            first = launches(ctx, lambda: pn.compute_h(qap, c))
            assert all(first.get(s) == 1 for s in BUILD_STAGES[:2]) and first.get(BUILD_STAGES[2], 0) >= 1, first
            seen[d, 1] = launches(ctx, lambda: pn.compute_h(qap, c))
            seen[d, 3] = launches(ctx, lambda: pn.compute_h_batch(qap, [c] * 3))
            for got in (seen[d, 1], seen[d, 3]):
                assert "bn_qap_moments" not in got and "bn_qap_moments_sum" not in got, got
                assert not any(s in got for s in BUILD_STAGES), got       # the plan is the QAP's: built once
                assert _tree_counts(got) == {"bn_qap_mtree_nleaf": 1, "bn_qap_mtree_level": 3, "bn_qap_mtree_reverse": 1}
    assert _tree_counts(seen[4 * S + 1, 1]) == _tree_counts(seen[4 * S + 1, 3]) == _tree_counts(seen[6 * S, 1])


# ---- the mode ---------------------------------------------------------------------------------------------------------------

def test_mode_plumbing(vm, ctx, pn, nat):
    dev = vm.device
    assert ctx.moment_transform == "direct"
    with pytest.raises(ValueError):
        with dev.moment_transform("fast"):
            pass
    with pytest.raises(RuntimeError, match="left by an exception"):
        with dev.moment_transform("tree"):
            assert ctx.moment_transform == "tree"
            raise RuntimeError("left by an exception")
    assert ctx.moment_transform == "direct"
    with dev.moment_transform("tree"):
        with dev.moment_transform("auto"):
            assert ctx.moment_transform == "auto"
        assert ctx.moment_transform == "tree"
    assert ctx.moment_transform == "direct"
    d = 200
    built = H.satisfiable_r1cs(d, seed=801)
    qap, c = fresh_qap(pn, built), built[5]
    seen = launches(ctx, lambda: pn.compute_h(qap, c))
    assert seen.get("bn_qap_moments") == 1 and not _tree_counts(seen), seen
    assert pn.h_batch_bytes(d, 10, 0, 2, tree=True) > pn.h_batch_bytes(d, 10, 0, 2) == pn.h_batch_bytes(d, 10, 0, 2, False)


def test_auto_chooses_by_the_threshold(vm, ctx, pn, nat):
    t = nat.BN256_QAP_MTREE_MIN
    got = {}
    with vm.device.moment_transform("auto"):
        for d in (t - 1, t):
            V, W, Y, out_ix, m, c, a, b, y = _scale_circuit(d, seed=d)
            qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
            got[d] = launches(ctx, lambda: pn.compute_h(qap, c))
    assert got[t - 1].get("bn_qap_moments") == 1 and not _tree_counts(got[t - 1]), got[t - 1]
    assert "bn_qap_moments" not in got[t] and got[t].get("bn_qap_mtree_nleaf") == 1, got[t]
