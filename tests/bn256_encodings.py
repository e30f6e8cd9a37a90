"""Encodings of BN-256 points, well formed and malformed, and the predicate that tells them apart: the CPU side of
tests/test_gpu_bn256_validate.py (gk_validate against the predicate) and tests/test_gpu_bn256_gates.py (every entry
point that takes points from outside).  Plain Python over oracle/bn256_ref.py; nothing here touches the library.

An encoding is the tuple of a point's 256-bit residues as they lie in memory, 32 bytes little-endian each: (x, y) in
G1, (x.re, x.im, y.re, y.im) on the twist (include/vmpc.h).  It is GOOD iff every residue is below P and either all
residues are zero (the point at infinity) or y^2 = x^3 + b holds in F_p / F_p2.  Everything else a gate must refuse:
a residue r + P is another byte string for the same point (malleability), and P, which is 0 mod P, in the place of a
zero is another byte string for infinity that a search for all-zero bytes does not see.

The valid point Q of a group is the first k G, k = 2, 3, .., whose every residue is below 2^256 - P - so that r + P
still fits in 32 bytes - and for which every row listed as "off the curve" is indeed off it.  Checked on the CPU by
tests/test_bn256_encodings.py."""
import functools
import random
from collections import namedtuple

from oracle import bn256_ref as bn

P = bn.P
TOP = 1 << 256
RESIDUES = {1: 2, 2: 4}
WIDTH = {1: 64, 2: 128}
CURVES = {1: (bn.E1, bn.G1), 2: (bn.E2, bn.G2)}
RESIDUE_NAMES = {1: ("x", "y"), 2: ("x.re", "x.im", "y.re", "y.im")}
CLASSES = ("good", "off", "alias", "inf-alias", "other")
KINDS = ("off", "alias", "inf-alias")              # the three malformed kinds of the gate tests

Row = namedtuple("Row", "cls name vals")


# ---- residues <-> bytes ------------------------------------------------------------------------------------------------
def flat(group, pt):
    """an oracle point ((x, y), ((x.re, x.im), (y.re, y.im)) or None) as its tuple of residues"""
    if pt is None:
        return (0,) * RESIDUES[group]
    return tuple(pt) if group == 1 else (*pt[0], *pt[1])


def encode(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def decode(raw):
    return tuple(int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32))


# ---- the predicate -----------------------------------------------------------------------------------------------------
def is_canonical(vals):
    return all(0 <= v < P for v in vals)


def on_curve(group, vals):
    """y^2 == x^3 + b for canonical residues (written out here, not taken from the oracle's Curve)"""
    if group == 1:
        x, y = vals
        return (y * y - (x * x * x + bn.B)) % P == 0
    x, y = (vals[0], vals[1]), (vals[2], vals[3])
    lhs = bn.Fp2.mul(y, y)
    rhs = bn.Fp2.add(bn.Fp2.mul(bn.Fp2.mul(x, x), x), bn.B_TWIST)
    return lhs == rhs


def is_good(group, vals):
    assert len(vals) == RESIDUES[group]
    if not is_canonical(vals):
        return False
    return not any(vals) or on_curve(group, vals)


def count_bad(group, rows):
    """what vmpc_bn256_validate_dev must count over these encodings (tuples of residues, or Rows)"""
    return sum(not is_good(group, r.vals if isinstance(r, Row) else r) for r in rows)


# ---- values around P ---------------------------------------------------------------------------------------------------
P_WORDS = [(P >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _join(words):
    return sum(w << (32 * i) for i, w in enumerate(words))


def word_boundary_values():
    """[(name, value)]: for each 32-bit word i of P, P with word i lowered by one and every lower word 0xffffffff
    (below P; the comparison is decided in word i after equal words above), and P with word i raised by one and every
    lower word zero (above P) - wherever that value exists and is not P itself"""
    out = []
    for i in range(8):
        if P_WORDS[i] > 0:
            v = _join([0xFFFFFFFF] * i + [P_WORDS[i] - 1] + P_WORDS[i + 1:])
            out.append((f"word {i} lowered", v))
        if P_WORDS[i] < 0xFFFFFFFF:
            v = _join([0] * i + [P_WORDS[i] + 1] + P_WORDS[i + 1:])
            out.append((f"word {i} raised", v))
    assert all(v != P and 0 <= v < TOP for _, v in out)
    return out


def probe_values(n_random=1000, seed=256):
    """the 256-bit values the comparison with P is tried on: the fixed edges, the word boundaries, uniform values"""
    rng = random.Random(seed)
    return [0, 1, P - 1, P, P + 1, TOP - 1, 1 << 255, (1 << 255) - 1] + [v for _, v in word_boundary_values()] + \
        [rng.randrange(TOP) for _ in range(n_random)]


# ---- the rows ----------------------------------------------------------------------------------------------------------
def _put(vals, j, v):
    return vals[:j] + (v,) + vals[j + 1:]


def _off_rows(group, q):
    """canonical encodings meant to be off the curve, made from the valid point q (residues)"""
    nres, names = RESIDUES[group], RESIDUE_NAMES[group]
    half = nres // 2
    x, y = q[:half], q[half:]
    rows = [(f"low bit of {names[j]} flipped", _put(q, j, q[j] ^ 1)) for j in range(nres)]
    rows += [("y + 1", _put(q, half, (q[half] + 1) % P)),
             ("(x, 0)", x + (0,) * half),
             ("(0, y)", (0,) * half + y),
             ("x and y swapped", y + x),
             ("P - 1 in every residue", (P - 1,) * nres)]
    if group == 2:
        g1 = bn.E1.mul(7, bn.G1)
        rows += [("re and im of x swapped", (q[1], q[0], q[2], q[3])),
                 ("a G1 point in the real parts", (g1[0], 0, g1[1], 0))]
    for wname, v in word_boundary_values():
        if v < P:
            rows += [(f"{wname} in {names[j]}", _put(q, j, v)) for j in range(nres)]
    return rows


@functools.lru_cache(maxsize=None)
def valid_point(group):
    """(k, Q as the oracle's point): see the module's text"""
    E, G = CURVES[group]
    pt = G
    for k in range(2, 64):
        pt = E.add(pt, G)
        q = flat(group, pt)
        if all(r < TOP - P for r in q) and all(is_canonical(v) and not is_good(group, v) for _, v in _off_rows(group, q)):
            return k, pt
    raise AssertionError("no multiple of the generator below 64 G qualifies")


def _sqrt_fp(a):
    r = pow(a, (P + 1) // 4, P)                     # P = 3 mod 4
    return r if r * r % P == a % P else None


def _sqrt_fp2(a):
    """a square root in F_p[i]/(i^2 + 1), or None: (c + d i)^2 = a with c^2 = (a.re +- |a|) / 2, d = a.im / (2 c)"""
    a0, a1 = a
    if a1 == 0:
        r = _sqrt_fp(a0)
        if r is not None:
            return (r, 0)
        r = _sqrt_fp(-a0 % P)
        return None if r is None else (0, r)
    s = _sqrt_fp((a0 * a0 + a1 * a1) % P)
    if s is None:
        return None
    half = pow(2, P - 2, P)
    for t in (s, -s % P):
        c = _sqrt_fp((a0 + t) * half % P)
        if c:
            r = (c, a1 * pow(2 * c, P - 2, P) % P)
            if bn.Fp2.mul(r, r) == (a0 % P, a1 % P):
                return r
    return None


@functools.lru_cache(maxsize=None)
def twist_point_with_zero():
    """residues (a, 0, y.re, y.im) of the first point of the twist with a real x = a = 1, 2, .. and no other zero
    residue.  A valid encoding with a ZERO residue: writing P there gives other bytes for the same point, which only
    the comparison's answer AT P refuses - the curve equation holds.  (It need not lie in G2; the gate does not ask.
    G1 has no such point: its order is prime, and x = 0 or y = 0 would be a point of order 3 or 2.)"""
    for a in range(1, 64):
        y = _sqrt_fp2(bn.Fp2.add(bn.Fp2.mul(bn.Fp2.mul((a, 0), (a, 0)), (a, 0)), bn.B_TWIST))
        if y is not None and y[0] and y[1]:
            vals = (a, 0, y[0], y[1])
            assert is_good(2, vals)
            return vals
    raise AssertionError("no twist point with a small real x")


def q_residues(group):
    return flat(group, valid_point(group)[1])


@functools.lru_cache(maxsize=None)
def table(group):
    """every row of the validation table, as a tuple of Row(cls, name, vals); cls is one of CLASSES"""
    E, G = CURVES[group]
    nres, names = RESIDUES[group], RESIDUE_NAMES[group]
    half = nres // 2
    _, pt = valid_point(group)
    q = flat(group, pt)
    rows = [Row("good", "Q", q), Row("good", "-Q", flat(group, E.neg(pt))), Row("good", "the generator", flat(group, G)),
            Row("good", "all-zero bytes", (0,) * nres)]
    rows += [Row("off", name, v) for name, v in _off_rows(group, q)]
    rows += [Row("alias", f"{names[j]} + P", _put(q, j, q[j] + P)) for j in range(nres)]
    rows.append(Row("alias", "every residue + P", tuple(r + P for r in q)))
    if group == 2:
        t = twist_point_with_zero()
        rows.append(Row("good", "a twist point with x.im = 0", t))
        rows.append(Row("alias", "that point with P for its zero x.im", _put(t, 1, P)))
    rows.append(Row("inf-alias", "P in every residue", (P,) * nres))
    rows += [Row("inf-alias", f"P in {names[j]}, 0 elsewhere", _put((0,) * nres, j, P)) for j in range(nres)]
    rows.append(Row("inf-alias", "P in the x residues only", (P,) * half + (0,) * half))
    rows += [Row("other", f"2^256 - 1 in {names[j]}", _put(q, j, TOP - 1)) for j in range(nres)]
    rows += [Row("other", f"P in {names[j]} of Q", _put(q, j, P)) for j in range(nres)]
    for wname, v in word_boundary_values():
        if v > P:
            rows += [Row("other", f"{wname} in {names[j]}", _put(q, j, v)) for j in range(nres)]
    assert len({r.name for r in rows}) == len(rows)
    return tuple(rows)


def rows_of(group, *classes):
    return [r for r in table(group) if r.cls in classes]


def bad_rows(group):
    return [r for r in table(group) if r.cls != "good"]


def malformed(group, kind):
    """the gate tests' malformed point, as residues: "off" - Q with the low bit of its LAST residue flipped (y.im on the
    twist); "alias" - Q with r + P in its last residue; "inf-alias" - P in every residue"""
    nres, names = RESIDUES[group], RESIDUE_NAMES[group]
    name = {"off": f"low bit of {names[-1]} flipped", "alias": f"{names[-1]} + P", "inf-alias": "P in every residue"}[kind]
    row, = [r for r in table(group) if r.cls == kind and r.name == name]
    return row.vals


def malformed_bytes(group, kind):
    return encode(malformed(group, kind))


def q_bytes(group):
    return encode(q_residues(group))
