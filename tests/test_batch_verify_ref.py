"""tests/batch_verify_ref.py against tests/frvec_ref.py, and the pure term assembly of the batched verifier
(compressed_pivot.batch_unfold_terms) against oracle/ed25519_ref.py: sum_p w_p unfold(Q_p) is the MSM of the terms."""
import random

import pytest

from oracle import ed25519_ref as ed
from tests import batch_verify_ref as ref
from tests import frvec_ref

ELL = ref.ELL


def _rand(rng, n):
    return [rng.randrange(ELL) for _ in range(n)]


@pytest.mark.parametrize("R,lb", [(0, 0), (0, 3), (1, 0), (3, 1), (2, 2)])
def test_one_proof_with_weight_one_is_challenge_products(R, lb):
    rng = random.Random(1000 + 10 * R + lb)
    cs, z = _rand(rng, R), _rand(rng, 1 << lb)
    n = 1 << (R + lb)
    form = _rand(rng, n)
    v = frvec_ref.challenge_products(cs, lb, z)
    u, dots = ref.batch_products([cs], lb, [z], [1], [form], n)
    assert u == v
    assert dots == [frvec_ref.dot(v, form)]
    _, short = ref.batch_products([cs], lb, [z], [1], [form], n - 1)
    assert short == [frvec_ref.dot(v[:-1], form[:-1])]
    assert ref.batch_products([cs], lb, [z], [1], [None], 0)[1] == [0]


def test_linear_in_the_weights():
    rng = random.Random(7)
    K, R, lb = 3, 3, 1
    n = 1 << (R + lb)
    cs, zs, forms = [_rand(rng, R) for _ in range(K)], [_rand(rng, 2) for _ in range(K)], [_rand(rng, n) for _ in range(K)]
    w1, w2 = _rand(rng, K), [ELL - 1, 1 << 128, 1]
    u1, d1 = ref.batch_products(cs, lb, zs, w1, forms, n)
    u2, d2 = ref.batch_products(cs, lb, zs, w2, forms, n)
    u3, d3 = ref.batch_products(cs, lb, zs, [(5 * a + b) % ELL for a, b in zip(w1, w2)], forms, n)
    assert u3 == [(5 * a + b) % ELL for a, b in zip(u1, u2)]
    assert d3 == [(5 * a + b) % ELL for a, b in zip(d1, d2)]
    # ... and a proof's column of u is its own weight times its own products
    singles = [ref.batch_products([cs[p]], lb, [zs[p]], [1], [forms[p]], n) for p in range(K)]
    assert u1 == [sum(w1[p] * singles[p][0][j] for p in range(K)) % ELL for j in range(n)]
    assert d1 == [w1[p] * singles[p][1][0] % ELL for p in range(K)]


def _pt(rng):
    return ed.pt_repeat(ed.BASE, rng.randrange(1, ELL))


def _unfold(q0, rounds):
    """Q' = A * Q**c * B**(c**2) (compressed_pivot.py:66), round by round"""
    q = q0
    for A, B, c in rounds:
        q = ed.pt_add(ed.pt_add(A, ed.pt_repeat(q, c)), ed.pt_repeat(B, c * c % ELL))
    return q


@pytest.mark.parametrize("R", [1, 3])
def test_assembled_terms_are_the_weighted_sum_of_the_unfolded_commitments(R):
    from verifiable_mpc_amd.compressed_pivot import batch_unfold_terms
    rng = random.Random(40 + R)
    K = 2
    weights = [ELL - 1, 1 << 128]
    proofs, want = [], ed.IDENTITY
    for p in range(K):
        q_terms = [(1, _pt(rng)), (rng.randrange(ELL), _pt(rng)), (rng.randrange(ELL), _pt(rng))]
        rounds = [(_pt(rng), _pt(rng), rng.randrange(ELL)) for _ in range(R)]
        proofs.append((q_terms, rounds))
        q0 = ed.IDENTITY
        for sc, pt in q_terms:
            q0 = ed.pt_add(q0, ed.pt_repeat(pt, sc))
        want = ed.pt_add(want, ed.pt_repeat(_unfold(q0, rounds), weights[p]))
    scalars, points = batch_unfold_terms(proofs, weights, ELL)
    assert len(scalars) == len(points) == K * (2 * R + 3)
    assert all(isinstance(s, int) and 0 <= s < ELL for s in scalars)
    got = ed.IDENTITY
    for sc, pt in zip(scalars, points):
        got = ed.pt_add(got, ed.pt_repeat(pt, sc))
    assert ed.pt_eq(got, want)
    # a weight that misses one proof's terms changes the sum
    other, _ = batch_unfold_terms(proofs, [weights[0], weights[1] + 1], ELL)
    assert other[:2 * R + 3] == scalars[:2 * R + 3] and other[2 * R + 3:] != scalars[2 * R + 3:]
