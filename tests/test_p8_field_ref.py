"""tests/p8_field_ref.py held against tests/p8_ref.py at p = l, its two routes against each other at p = n, and the
knowledge-of-exponent algebra against its own verifier equations (no GPU)."""
import random

import pytest

from tests import p8_field_ref as fref
from tests import p8_ref as ref

ELL, BN_N = fref.ELL, fref.BN_N
CASES = [(101, 5, 1, 2), (103, 5, 3, 2), (7, 4, 0, 1), (8, 6, 9, 0), (21, 3, 5, 1)]      # (seed, n_x, m, n_out)


def test_the_two_moduli_are_the_groups_orders():
    assert ELL == ref.ELL
    from verifiable_mpc_amd import device, pynocchio
    assert BN_N == pynocchio.ORDER == device.BN256_ORDER and BN_N.bit_length() == 256


@pytest.mark.parametrize("seed,n_x,m,n_out", CASES)
def test_at_l_the_restatement_is_p8_ref(seed, n_x, m, n_out):
    rng = random.Random(seed)
    A, B, O = ref.random_circuit(rng, n_x, m, n_out)
    x = [rng.randrange(ELL) for _ in range(n_x + 1)]          # one trailing input no form reads
    r_a, r_b, c, rho = (rng.randrange(2 * m + 1, ELL) for _ in range(4))
    F = fref.P8(ELL)
    assert F.circuit_digest(n_x, A, B, O) == ref.circuit_digest(n_x, A, B, O)
    assert F.triples(n_x, A, B, x) == ref.triples(n_x, A, B, x)
    a, b, gamma = ref.triples(n_x, A, B, x)
    tail = ref.z_tail_bary(a, b, r_a, r_b)
    assert F.z_tail_bary(a, b, r_a, r_b) == tail == F.z_tail_naive(a, b, r_a, r_b)
    assert F.lagrange_bary(2 * m, c) == ref.lagrange_bary(2 * m, c) == F.lagrange_naive(2 * m, c)
    assert F.forms_bary(n_x, len(x), A, B, c) == ref.forms_bary(n_x, len(x), A, B, c)
    z = [v % ELL for v in x] + tail
    y = [(ref.dot(co, z) + k) % ELL for co, k in ref.forms_bary(n_x, len(x), A, B, c)]
    outputs = [ref.row_eval(r, n_x, x, gamma) for r in O]
    for route in ("bary", "naive"):
        assert F.combine(n_x, len(x), A, B, O, c, rho, y, outputs, route) == \
            ref.combine(n_x, len(x), A, B, O, c, rho, y, outputs, route)


@pytest.mark.parametrize("m", [0, 1, 2, 3, 5, 8])
def test_at_n_the_two_routes_agree(m):
    rng = random.Random(900 + m)
    F = fref.P8(BN_N)
    n_x, n_out = 4, 2
    A, B, O = F.random_circuit(rng, n_x, m, n_out)
    x = [rng.randrange(BN_N) for _ in range(n_x)]
    r_a, r_b = rng.randrange(1, BN_N), rng.randrange(1, BN_N)
    a, b, gamma = F.triples(n_x, A, B, x)
    tail = F.z_tail_bary(a, b, r_a, r_b)
    assert tail == F.z_tail_naive(a, b, r_a, r_b) and len(tail) == 3 + 2 * m
    assert tail[3:3 + m] == gamma
    c, rho = rng.randrange(2 * m + 1, BN_N), rng.randrange(BN_N)
    assert F.lagrange_bary(m, c) == F.lagrange_naive(m, c)
    assert F.lagrange_bary(2 * m, c) == F.lagrange_naive(2 * m, c)
    assert F.lagrange_bary(2 * m, m) == [int(j == m) for j in range(2 * m + 1)]          # a node: the unit vector
    z = [v % BN_N for v in x] + tail
    Fb, Gb, Hb = F.forms_bary(n_x, n_x, A, B, c)
    assert (Fb, Gb, Hb) == F.forms_naive(n_x, n_x, A, B, O, c)[:3]
    y = [(F.dot(co, z) + k) % BN_N for co, k in (Fb, Gb, Hb)]
    assert y[0] * y[1] % BN_N == y[2]                          # h = f g at the challenge
    outputs = [F.row_eval(r, n_x, x, gamma) for r in O]
    bary = F.combine(n_x, n_x, A, B, O, c, rho, y, outputs, "bary")
    assert bary == F.combine(n_x, n_x, A, B, O, c, rho, y, outputs, "naive")
    assert (F.dot(bary[0], z) + bary[1]) % BN_N == 0
    assert F.circuit_digest(n_x, A, B, O) != fref.P8(ELL).circuit_digest(n_x, A, B, O)   # the tag names the field


def test_koe_transcript_is_its_stated_bytes():
    import hashlib
    F = fref.P8(BN_N)
    P, pi, dg = bytes(range(64)), bytes(range(128)), bytes(32)
    c, d1 = F.koe_first_challenge(P, pi, dg, 7)
    assert d1 == hashlib.sha256(b"vmpc-ac20/p8-koe/first/v1" + P + pi + dg + (7).to_bytes(8, "little")).digest()
    assert c == int.from_bytes(d1, "little") % BN_N
    rho = F.koe_second_challenge(d1, [1, 2, 3], [5])
    want = hashlib.sha256(b"vmpc-ac20/p8-koe/second/v1" + d1 + b"".join(v.to_bytes(32, "little") for v in (1, 2, 3)) +
                          (1).to_bytes(4, "little") + (5).to_bytes(32, "little")).digest()
    assert rho == int.from_bytes(want, "little") % BN_N


@pytest.mark.parametrize("N", [1, 2, 5, 14])
def test_trapdoor_identities_hold_for_random_z_and_L(N):
    rng = random.Random(40 + N)
    t = fref.KoeTrapdoor(rng.randrange(1, BN_N), rng.randrange(1, BN_N), rng.randrange(1, BN_N))
    z = [rng.randrange(BN_N) for _ in range(N)]
    L = [rng.randrange(BN_N) for _ in range(N)]
    gamma = rng.randrange(1, BN_N)
    P_exp, pi_exp = t.commitment(z, gamma)
    Q_exp, u = t.opening(L, z, gamma)
    assert len(t.product(L, z, gamma)) == 2 * N
    assert t.opening_by_evaluation(L, z, gamma) == (Q_exp, u)
    assert u == sum(a * b for a, b in zip(L, z)) % BN_N
    assert t.restriction_check(P_exp, pi_exp)
    assert t.prq_check(L, P_exp, Q_exp, u)
    # each element is needed: a wrong one breaks its equation
    assert not t.restriction_check(P_exp, (pi_exp + 1) % BN_N)
    assert not t.prq_check(L, P_exp, (Q_exp + 1) % BN_N, u)
    assert not t.prq_check(L, P_exp, Q_exp, (u + 1) % BN_N)
    assert not t.prq_check(L, (P_exp + 1) % BN_N, Q_exp, u)


def test_prove_koe_closes_on_a_small_circuit():
    rng = random.Random(5)
    F = fref.P8(BN_N)
    A, B, O = F.random_circuit(rng, 5, 3, 2)
    x = [rng.randrange(BN_N) for _ in range(5)]
    out = F.prove_koe(5, A, B, O, x, 11, 13, lambda z: (bytes(64), bytes(128)))
    assert len(out["z"]) == 14 and len(out["L"]) == 14           # N = n_in + 3 + 2m, no padding
