"""GPU tests of the context's polynomial-product mode (vmpc_ctx_set_poly_product, device.poly_product): off by default,
and under mode 2 every caller of the product inside the library - h and its batch and share forms, t's coefficients, the
knowledge-of-exponent prover - returns the bytes it returns under mode 0, through the NTT's four stages instead of the
schoolbook kernel's."""
import random
import types

import numpy as np
import pytest

from oracle import bn256_ref as bn
from tests import h_ref as H

pytestmark = pytest.mark.gpu
N = bn.N
NTT_STAGES = ("bn_fr_ntt_split", "bn_fr_ntt_fwd", "bn_fr_ntt_inv", "bn_fr_ntt_crt")


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
def koe(vm):
    return vm.knowledge_of_exponent


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


def fresh_qap(pn, built):
    """a new R1CSQAP object: t's coefficients are cached per (context, QAP)"""
    V, W, Y, out_ix, m, _ = built
    return pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), out_ix, m=m)


def deltas_of(seed):
    rng = random.Random(seed)
    return types.SimpleNamespace(v=rng.randrange(N), w=rng.randrange(N), y=rng.randrange(N))


def opening(vm, koe, n, seed):
    rng = random.Random(seed)
    P = vm.pynocchio
    prev, koe.prng = koe.prng, rng           # the setup draws its trapdoor from the module's generator
    try:
        pp = koe.trusted_setup(P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2), n, N)
    finally:
        koe.prng = prev
    x = [rng.randrange(N) for _ in range(n)]
    coeffs = [rng.randrange(N) for _ in range(n)]
    gamma = rng.randrange(N)
    return lambda: koe.opening_linear_form_prover(vm.pivot.LinearForm(coeffs), x, gamma, pp)


def proof_bytes(res):
    proof, u = res
    return {k: proof[k].coords for k in ("P", "pi", "Q")}, int(u)


# ---- the mode itself --------------------------------------------------------------------------------------------------

def test_default_is_schoolbook_and_the_block_restores_it(vm, ctx, koe):
    assert ctx.get_poly_product() == 0
    prove = opening(vm, koe, 64, 1)
    seen = launches(ctx, prove)
    assert seen.get("bn_fr_poly_mul") == 1 and not any(s in seen for s in NTT_STAGES), seen
    with vm.device.poly_product("ntt"):
        assert ctx.get_poly_product() == 2
        seen = launches(ctx, prove)
    assert all(seen.get(s, 0) >= 1 for s in NTT_STAGES) and "bn_fr_poly_mul" not in seen, seen
    assert ctx.get_poly_product() == 0
    with pytest.raises(RuntimeError, match="left by an exception"):
        with vm.device.poly_product("auto"):
            assert ctx.get_poly_product() == 1
            raise RuntimeError("left by an exception")
    assert ctx.get_poly_product() == 0
    # a block inside a block restores the outer block's mode, not the default
    with vm.device.poly_product("ntt"):
        with vm.device.poly_product("schoolbook"):
            assert ctx.get_poly_product() == 0
        assert ctx.get_poly_product() == 2
    assert ctx.get_poly_product() == 0
    with pytest.raises(ValueError):
        with vm.device.poly_product("fft"):
            pass
    assert ctx.get_poly_product() == 0


def test_invalid_mode_is_refused_and_changes_nothing(vm, ctx):
    nat = vm._native
    for start in (0, 1):
        ctx.set_poly_product(start)
        try:
            for bad in (-1, 3, 100):
                with pytest.raises(nat.VmpcError) as ei:
                    ctx.set_poly_product(bad)
                assert ei.value.code == nat.E_INVAL
                assert ctx.get_poly_product() == start
        finally:
            ctx.set_poly_product(0)


def test_auto_chooses_by_the_threshold(vm, ctx):
    nat = vm._native
    t = nat.BN256_FR_NTT_MIN
    buf = ctx.upload(np.random.default_rng(3).integers(0, 256, size=(t, 32), dtype=np.uint8))
    out = ctx.alloc(32 * 2 * t)
    with vm.device.poly_product("auto"):
        below = launches(ctx, lambda: ctx.bn256_fr_poly_mul(buf.ptr, t, buf.ptr, t - 1, out.ptr))
        at = launches(ctx, lambda: ctx.bn256_fr_poly_mul(buf.ptr, t, buf.ptr, t, out.ptr))
    assert below.get("bn_fr_poly_mul") == 1 and not any(s in below for s in NTT_STAGES), below
    assert "bn_fr_poly_mul" not in at and at.get("bn_fr_ntt_crt") == 1 and at.get("bn_fr_ntt_split") == 2, at


def test_fr_poly_mul_method(vm, ctx, koe):
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 256, size=(300, 32), dtype=np.uint8), rng.integers(0, 256, size=(129, 32), dtype=np.uint8)
    want = koe.fr_poly_mul(a, b)
    seen = launches(ctx, lambda: np.array_equal(koe.fr_poly_mul(a, b, method="ntt"), want) or pytest.fail("bits differ"))
    assert seen.get("bn_fr_ntt_crt") == 1 and "bn_fr_poly_mul" not in seen
    with vm.device.poly_product("ntt"):
        seen = launches(ctx, lambda: np.array_equal(koe.fr_poly_mul(a, b), want) or pytest.fail("bits differ"))
        assert seen.get("bn_fr_ntt_crt") == 1 and "bn_fr_poly_mul" not in seen
        seen = launches(ctx, lambda: np.array_equal(koe.fr_poly_mul(a, b, method="schoolbook"), want) or pytest.fail("bits"))
        assert seen.get("bn_fr_poly_mul") == 1 and not any(s in seen for s in NTT_STAGES)
        assert ctx.get_poly_product() == 2
    with pytest.raises(ValueError):
        koe.fr_poly_mul(a, b, method="karatsuba")


# ---- every caller, mode 2 against mode 0 ------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [2, 3, 129, 300])
def test_h_and_its_batch_under_the_ntt(vm, ctx, pn, d):
    k = 3
    built = [H.satisfiable_r1cs(d, seed=50 + d)]
    V, W, Y, out_ix, m, c = built[0]
    cs = [c] * k          # (a random R1CS has the one witness it was built with; the deltas differ per row)
    dl = [deltas_of(10 * d + w) for w in range(k)]
    got = {}
    for mode in ("schoolbook", "ntt"):
        with vm.device.poly_product(mode):
            qap = fresh_qap(pn, built[0])
            seen = launches(ctx, lambda: got.__setitem__(mode, (
                pn.compute_h(qap, c).coeffs, pn.compute_h(qap, c, dl[0]).coeffs,
                [h.coeffs for h in pn.compute_h_batch(qap, cs)], [h.coeffs for h in pn.compute_h_batch(qap, cs, dl)])))
        if mode == "ntt":
            assert "bn_fr_poly_mul" not in seen and seen.get("bn_fr_ntt_crt", 0) >= 8, seen
        else:
            assert not any(s in seen for s in NTT_STAGES), seen
    assert got["ntt"] == got["schoolbook"]
    assert len(got["ntt"][1]) == d + 1 and len(got["ntt"][3]) == k


def test_h_share_under_the_ntt(vm, ctx, pn):
    d = 129
    built = H.satisfiable_r1cs(d, seed=77)
    rng = random.Random(77)
    share = [rng.randrange(N) for _ in range(len(built[5]))]      # a share vector satisfies nothing: no check is made
    got = {}
    for mode in ("schoolbook", "ntt"):
        with vm.device.poly_product(mode):
            qap = fresh_qap(pn, built)
            got[mode] = (pn.compute_h_share(qap, share).coeffs, pn.compute_h_share(qap, share, deltas_of(5)).coeffs)
    assert got["ntt"] == got["schoolbook"] and len(got["ntt"][1]) == d + 1


@pytest.mark.parametrize("n", [1, 2, 33])
def test_opening_prover_under_the_ntt(vm, ctx, koe, n):
    prove = opening(vm, koe, n, 200 + n)
    want = proof_bytes(prove())
    with vm.device.poly_product("ntt"):
        seen = launches(ctx, lambda: proof_bytes(prove()) == want or pytest.fail("the proofs differ"))
    assert seen.get("bn_fr_ntt_crt") == 1 and "bn_fr_poly_mul" not in seen, seen


@pytest.mark.parametrize("d", [128, 129, 1000])
def test_t_coeffs_under_the_ntt(vm, ctx, pn, d):
    built = H.satisfiable_r1cs(d, seed=300 + d)
    got = {}
    for mode in ("schoolbook", "ntt"):
        with vm.device.poly_product(mode):
            seen = launches(ctx, lambda: got.__setitem__(
                mode, ctx.download(pn._t_coeffs(ctx, fresh_qap(pn, built)).ptr, 32 * (d + 1)).tobytes()))
        if d > 128:
            assert ("bn_fr_ntt_crt" in seen) == (mode == "ntt") and ("bn_fr_poly_mul" in seen) == (mode != "ntt"), seen
    assert got["ntt"] == got["schoolbook"]
    if d <= 129:
        want = H.t_coeffs(d)
        assert [int.from_bytes(got["ntt"][32 * i:32 * i + 32], "little") for i in range(d + 1)] == want
