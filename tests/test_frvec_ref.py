"""CPU: tests/frvec_ref.py against an independent definition, in exponent space.

A generator g_j is its exponent e_j, and one round of the fold of compressed_pivot.py:64, g' = g_l^c * g_r, is
e'_i = c e_l[i] + e_r[i] mod l.  The challenge products and the tail scalars are the coefficients that let an MSM over
the unfolded generators stand for a commitment over the folded ones; folding the exponents round by round and pairing
with z says the same without a bit of an index being looked at.
"""
import random

import pytest

from tests import frvec_ref as ref

ELL = ref.ELL


def fold(e, c):
    h = len(e) // 2
    assert len(e) == 2 * h
    return [(c * l + r) % ELL for l, r in zip(e[:h], e[h:])]


def fold_all(e, cs):
    for c in cs:
        e = fold(e, c)
    return e


def inner(a, b):
    assert len(a) == len(b)
    return sum(u * v for u, v in zip(a, b)) % ELL


def residues(rng, n):
    v = [rng.randrange(ELL) for _ in range(n)]
    if n:
        v[0] = v[-1] = ELL - 1
    return v


def test_axpy_and_dot_on_small_numbers():
    assert ref.axpy(3, [1, 2, ELL - 1], [5, 0, 3]) == [8, 6, 0]
    assert ref.axpy(ELL - 1, [1, 2, 0]) == [ELL - 1, ELL - 2, 0]
    assert ref.axpy(2, [4], None, tail=ELL + 7) == [8, 7]
    assert ref.axpy(2, [], None, tail=5) == [5] and ref.axpy(2, [], []) == []
    assert ref.dot([], []) == 0
    assert ref.dot([ELL - 1, 2], [ELL - 1, 3]) == 7
    with pytest.raises(ValueError):
        ref.dot([1, 2], [1])


@pytest.mark.parametrize("R", [0, 1, 2, 5, 9])
def test_bit_products_two_constructions(R):
    rng = random.Random(300 + R)
    cs = residues(rng, R)
    assert ref.bit_products_by_halves(cs) == ref.bit_products(cs)
    # the all-ones index takes no challenge, index 0 takes them all
    prod = 1
    for c in cs:
        prod = prod * c % ELL
    assert ref.bit_products(cs)[-1] == 1 and ref.bit_products(cs)[0] == prod


@pytest.mark.parametrize("R,low_bits", [(0, 0), (0, 3), (1, 0), (3, 1), (5, 2)])
def test_challenge_products_are_the_folds_as_one_linear_map(R, low_bits):
    rng = random.Random(1000 + 10 * R + low_bits)
    cs, z = residues(rng, R), residues(rng, 1 << low_bits)
    s = ref.challenge_products(cs, low_bits, z)
    assert len(s) == 1 << (R + low_bits)
    assert s == ref.challenge_products(cs, low_bits, z, ref.bit_products_by_halves(cs))
    for _ in range(3):
        e = residues(rng, 1 << (R + low_bits))
        assert inner(s, e) == inner(z, fold_all(e, cs))
    # a challenge 0 drops the left half of its round, challenges 1 leave z repeated
    if R:
        assert ref.challenge_products([1] * R, low_bits, z) == z * (1 << R)
        s0 = ref.challenge_products([0] + cs[1:], low_bits, z)
        assert not any(s0[:len(s0) // 2]) and s0[len(s0) // 2:] == s[len(s) // 2:]


TAIL_CASES = [(log2_m0, t) for log2_m0 in (1, 2, 6) for t in range(log2_m0)]


@pytest.mark.parametrize("log2_m0,t", TAIL_CASES)
def test_tail_scalars_are_the_cross_terms_over_the_unfolded_generators(log2_m0, t):
    rng = random.Random(2000 + 10 * log2_m0 + t)
    m0 = 1 << log2_m0
    m = m0 >> t
    h = m // 2
    cs, z = residues(rng, t), residues(rng, m)
    A, B = ref.tail_scalars(cs, log2_m0, z)
    assert len(A) == len(B) == m0
    for _ in range(3):
        e = residues(rng, m0)
        f = fold_all(e, cs)
        assert len(f) == m
        assert inner(A, e) == inner(z[:h], f[h:])
        assert inner(B, e) == inner(z[h:], f[:h])
    assert not any(a and b for a, b in zip(A, B))
    # with non-zero z and challenges exactly one of the two is non-zero at every index
    cs1, z1 = [c or 1 for c in cs], [v or 1 for v in z]
    A1, B1 = ref.tail_scalars(cs1, log2_m0, z1)
    assert all(bool(a) != bool(b) for a, b in zip(A1, B1))


@pytest.mark.parametrize("log2_m0,t", TAIL_CASES)
def test_tail_scalar_blocks_concatenate_to_the_whole(log2_m0, t):
    rng = random.Random(3000 + 10 * log2_m0 + t)
    m0 = 1 << log2_m0
    cs, z = residues(rng, t), residues(rng, m0 >> t)
    A, B = ref.tail_scalars(cs, log2_m0, z)
    partitions = [[0, m0], list(range(m0 + 1)), [0, 0, 1, m0, m0]]
    for _ in range(3):
        partitions.append([0] + sorted(rng.randrange(m0 + 1) for _ in range(rng.randrange(1, 5))) + [m0])
    for cuts in partitions:
        gotA, gotB = [], []
        for j0, j1 in zip(cuts, cuts[1:]):
            a, b = ref.tail_scalars_block(cs, log2_m0, z, j0, j1 - j0)
            assert len(a) == len(b) == j1 - j0
            gotA += a
            gotB += b
        assert (gotA, gotB) == (A, B), cuts
