"""CPU check of tests/bn256_encodings.py: the predicate agrees with the oracle's curves on valid multiples and on
arbitrary canonical pairs, and every row of the validation table lands in the class it is listed under - by a
classification written out here (canonical? congruent to Q? congruent to infinity? on the curve, by the oracle's own
Curve.on_curve), not by the helper's predicate."""
import random

import pytest

from oracle import bn256_ref as bn
from tests import bn256_encodings as enc

P, TOP = enc.P, enc.TOP


def oracle_point(group, vals):
    return tuple(vals) if group == 1 else ((vals[0], vals[1]), (vals[2], vals[3]))


@pytest.mark.parametrize("group", [1, 2])
def test_predicate_agrees_with_the_oracle(group):
    E, G = enc.CURVES[group]
    rng = random.Random(group)
    pt = None
    for k in range(1, 24):
        pt = E.add(pt, G)
        assert E.on_curve(pt)
        for q in (pt, E.neg(pt), E.mul(rng.randrange(1, bn.N), G)):
            vals = enc.flat(group, q)
            assert enc.is_good(group, vals) and enc.decode(enc.encode(vals)) == vals
    assert enc.is_good(group, enc.flat(group, None)) and enc.encode(enc.flat(group, None)) == bytes(enc.WIDTH[group])
    for _ in range(200):
        vals = tuple(rng.randrange(P) for _ in range(enc.RESIDUES[group]))
        assert enc.is_good(group, vals) == E.on_curve(oracle_point(group, vals)) == enc.on_curve(group, vals)
    # a residue of P or more is refused whatever it is congruent to
    good = enc.flat(group, E.mul(5, G))
    for j in range(enc.RESIDUES[group]):
        for v in (P, TOP - 1, good[j] + P):
            if v < TOP:
                assert not enc.is_good(group, good[:j] + (v,) + good[j + 1:])


@pytest.mark.parametrize("group", [1, 2])
def test_the_valid_point(group):
    E, G = enc.CURVES[group]
    k, pt = enc.valid_point(group)
    assert k >= 2 and pt == E.mul(k, G) and E.on_curve(pt)
    q = enc.q_residues(group)
    assert all(r < TOP - P for r in q) and all(r + P < TOP for r in q)
    assert len(enc.q_bytes(group)) == enc.WIDTH[group]
    assert not all(r < TOP - P for r in enc.flat(1, bn.G1))          # why the table is not built on G1's generator


@pytest.mark.parametrize("group", [1, 2])
def test_every_row_is_in_its_class(group):
    E, _ = enc.CURVES[group]
    q = enc.q_residues(group)
    nres = enc.RESIDUES[group]
    seen = {c: 0 for c in enc.CLASSES}
    valid = {r.vals for r in enc.table(group) if r.cls == "good" and any(r.vals)}
    assert q in valid
    for row in enc.table(group):
        vals = row.vals
        assert len(vals) == nres and all(0 <= v < TOP for v in vals), row.name
        assert len(enc.encode(vals)) == enc.WIDTH[group]
        canonical = all(v < P for v in vals)
        reduced = tuple(v % P for v in vals)
        curve = not any(reduced) or E.on_curve(oracle_point(group, reduced))
        if row.cls == "good":
            assert canonical and curve, row.name
        elif row.cls == "off":
            assert canonical and not curve and any(vals), row.name
        elif row.cls == "alias":
            assert not canonical and reduced in valid and curve, row.name
        elif row.cls == "inf-alias":
            assert not canonical and not any(reduced) and any(vals), row.name
        else:
            assert row.cls == "other" and not canonical and reduced not in valid and any(reduced), row.name
        assert enc.is_good(group, vals) == (row.cls == "good"), row.name
        seen[row.cls] += 1
    n_low = sum(v < P for _, v in enc.word_boundary_values())
    n_high = len(enc.word_boundary_values()) - n_low
    extra = 1 if group == 2 else 0                    # the twist point with a zero residue, and its alias
    assert seen["good"] == 4 + extra
    assert seen["off"] == nres + 5 + (2 if group == 2 else 0) + n_low * nres
    assert seen["alias"] == nres + 1 + extra and seen["inf-alias"] == nres + 2
    assert seen["other"] == 2 * nres + n_high * nres
    assert enc.count_bad(group, enc.table(group)) == len(enc.table(group)) - 4 - extra == len(enc.bad_rows(group))


def test_word_boundary_values():
    vals = enc.word_boundary_values()
    assert len(vals) >= 14 and all(v != P for _, v in vals)
    for name, v in vals:
        i = int(name.split()[1])
        # the value equals P in every word above i and differs in word i: there the comparison is decided
        assert v >> (32 * (i + 1)) == P >> (32 * (i + 1))
        assert ((v >> (32 * i)) & 0xFFFFFFFF) - enc.P_WORDS[i] == (1 if "raised" in name else -1)
        assert (v > P) == ("raised" in name)
        assert v & ((1 << (32 * i)) - 1) == (0 if "raised" in name else (1 << (32 * i)) - 1)
    probes = enc.probe_values()
    assert probes[:8] == [0, 1, P - 1, P, P + 1, TOP - 1, 1 << 255, (1 << 255) - 1] and len(probes) == 8 + len(vals) + 1000


@pytest.mark.parametrize("group", [1, 2])
def test_the_gate_kinds(group):
    q = enc.q_residues(group)
    off, alias, inf = (enc.malformed(group, k) for k in enc.KINDS)
    assert off[:-1] == q[:-1] and off[-1] == q[-1] ^ 1 and off[-1] < P
    assert alias[:-1] == q[:-1] and alias[-1] == q[-1] + P
    assert inf == (P,) * enc.RESIDUES[group] and any(enc.encode(inf))          # not the all-zero bytes
    assert not any(enc.is_good(group, v) for v in (off, alias, inf))
    assert enc.decode(enc.malformed_bytes(group, "alias")) == alias


def test_the_twist_point_with_a_zero_residue():
    t = enc.twist_point_with_zero()
    assert t[1] == 0 and all(t[j] for j in (0, 2, 3)) and bn.E2.on_curve(oracle_point(2, t))
    alias, = [r.vals for r in enc.table(2) if r.name == "that point with P for its zero x.im"]
    assert alias == (t[0], P, t[2], t[3]) and not enc.is_good(2, alias)
    for a in ((5, 0), (0, 7), (3, 4), (P - 1, 2), bn.B_TWIST):
        sq = bn.Fp2.mul(a, a)
        r = enc._sqrt_fp2(sq)
        assert r in (a, bn.Fp2.neg(a)), a
