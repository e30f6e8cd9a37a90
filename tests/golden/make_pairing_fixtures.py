#!/usr/bin/env python3
"""Generate tests/golden/bn256_pairing.json by running the REFERENCE's own modules.

Needs a checkout of the reference (read-only), named by VMPC_REFERENCE:
    VMPC_REFERENCE=<reference checkout> python3 -B tests/golden/make_pairing_fixtures.py
Two parts:
  (a) `pairing`: values of the reference's verifiable_mpc/ac20/pairing.py optimal_ate for a few point pairs
      (generators, random multiples, infinity on either side).  pairing.py needs MPyC's extension field for the
      twist (BN256_TWIST.field); the mpyc shim has none (make_fixtures.py stubs pairing.py out), so this script
      supplies a small stand-in for exactly the API pairing.py uses - GFp_2([a, b, 0]), .value.value[k], int(),
      arithmetic with ints, ** and reciprocal() - and point objects with .x/.y/.z, ~, normalize() and identity.
  (b) `pinocchio`: one Pinocchio instance made by the reference (Trapdoor, generate_evalkey, generate_verikey,
      compute_proof on the demo program, seeded) over the shim's BN-256 groups, and the result of the
      reference's own `verify` on it, run with the real pairing.py of (a).
The fixture is DATA (points, scalars, pairing values); no reference source text is stored.
GT values are 12 hex residues in the order of include/vmpc.h: [x.x, x.y, x.z, y.x, y.y, y.z], each (re, im).
"""
import importlib.util
import json
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REFERENCE = os.environ.get("VMPC_REFERENCE")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "verifiable_mpc")):
    sys.exit("set VMPC_REFERENCE to a checkout of the reference (the directory that holds verifiable_mpc/)")
sys.path.insert(0, os.path.join(HERE, "mpyc_shim"))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, REPO)

from oracle import bn256_ref as bn                                  # noqa: E402

SEED = 20201152
P = bn.P


def hx(v):
    return format(int(v) % P, "x")


# ---- (a) the stand-in field and curve API that pairing.py reads -------------------------------------------------

class _Coeffs:
    __slots__ = ("value",)

    def __init__(self, value):
        self.value = value


class GFp1:
    """F_p element: int(), arithmetic with ints and other elements"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = int(v) % P

    def __int__(self): return self.v
    def __add__(self, o): return GFp1(self.v + int(o))
    __radd__ = __add__
    def __sub__(self, o): return GFp1(self.v - int(o))
    def __rsub__(self, o): return GFp1(int(o) - self.v)
    def __mul__(self, o): return GFp1(self.v * int(o))
    __rmul__ = __mul__
    def __neg__(self): return GFp1(-self.v)
    def __pow__(self, e): return GFp1(pow(self.v, e, P))
    def __eq__(self, o): return self.v == int(o)


class GFp2:
    """F_p[i]/(i^2 + 1) with the MPyC extension-field surface pairing.py uses: GFp2([a, b, 0]), GFp2(k),
    .value.value[k], int() (zero iff the element is zero), reciprocal(), **"""
    __slots__ = ("a", "b")

    def __init__(self, v=0):
        if isinstance(v, (list, tuple)):
            a, b = int(v[0]), int(v[1]) if len(v) > 1 else 0
        else:
            a, b = int(v), 0
        self.a, self.b = a % P, b % P

    @property
    def value(self):
        return _Coeffs([self.a, self.b])

    def __int__(self): return self.a + P * self.b

    @staticmethod
    def _lift(o):
        return o if isinstance(o, GFp2) else GFp2(int(o))

    def __add__(self, o):
        o = self._lift(o)
        return GFp2([self.a + o.a, self.b + o.b])
    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        return GFp2([self.a - o.a, self.b - o.b])

    def __rsub__(self, o): return self._lift(o) - self

    def __neg__(self): return GFp2([-self.a, -self.b])

    def __mul__(self, o):
        o = self._lift(o)
        return GFp2([self.a * o.a - self.b * o.b, self.a * o.b + self.b * o.a])
    __rmul__ = __mul__

    def __pow__(self, e):
        r, x = GFp2(1), self
        while e:
            if e & 1:
                r = r * x
            x = x * x
            e >>= 1
        return r

    def reciprocal(self):
        d = pow(self.a * self.a + self.b * self.b, P - 2, P)
        return GFp2([self.a * d, -self.b * d])

    def __eq__(self, o):
        o = self._lift(o)
        return self.a == o.a and self.b == o.b

    def __repr__(self):
        return f"({self.a},{self.b})"


def _curve(field):
    class Point:
        """Jacobian (x, y, z) over `field`; infinity is the class's `identity` object"""
        def __init__(self, xyz, check=True):
            self.x, self.y, self.z = (c if isinstance(c, field) else field(c) for c in xyz)

        def __invert__(self):
            return type(self)((self.x, -self.y, self.z))

        def normalize(self):
            if self is self.identity:
                return self
            zi = self.z.reciprocal() if field is GFp2 else GFp1(pow(int(self.z), P - 2, P))
            zi2 = zi * zi
            return type(self)((self.x * zi2, self.y * zi2 * zi, field(1)))

    Point.field = field
    Point.identity = Point.__new__(Point)
    return Point


Twist, G1pt = _curve(GFp2), _curve(GFp1)


def load_reference_pairing():
    """pairing.py imported unmodified over a mpyc.fingroups whose EllipticCurve hands out the stand-ins above"""
    fake = types.ModuleType("mpyc.fingroups")
    fake.EllipticCurve = lambda name, *a: Twist if name == "BN256_twist" else G1pt
    saved = sys.modules.get("mpyc.fingroups")
    import mpyc                                                  # noqa: F401 (the shim's package)
    sys.modules["mpyc.fingroups"] = fake
    try:
        spec = importlib.util.spec_from_file_location(
            "verifiable_mpc.ac20.pairing", os.path.join(REFERENCE, "verifiable_mpc", "ac20", "pairing.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is not None:
            sys.modules["mpyc.fingroups"] = saved
        else:
            del sys.modules["mpyc.fingroups"]
    return mod


def g1_point(pt):
    return G1pt.identity if pt is None else G1pt((pt[0], pt[1], 1))


def twist_point(pt):
    return Twist.identity if pt is None else Twist((GFp2(list(pt[0])), GFp2(list(pt[1])), GFp2(1)))


def gt_hex(f):
    out = []
    for half in (f.x, f.y):
        for c in (half.x, half.y, half.z):
            out += [hx(c.value.value[0]), hx(c.value.value[1])]
    return out


def pairing_cases(pairing_mod, rng):
    """reference pynocchio.pairing(a, b) = optimal_ate(b, a) on G1 x twist point pairs"""
    a, b, c = (rng.randrange(1, bn.N) for _ in range(3))
    pairs = [
        ("generators", bn.G1, bn.G2),
        ("a*G1, G2", bn.E1.mul(a, bn.G1), bn.G2),
        ("G1, b*G2", bn.G1, bn.E2.mul(b, bn.G2)),
        ("a*G1, b*G2", bn.E1.mul(a, bn.G1), bn.E2.mul(b, bn.G2)),
        ("-G1, c*G2", bn.E1.neg(bn.G1), bn.E2.mul(c, bn.G2)),
        ("c*G1, -G2", bn.E1.mul(c, bn.G1), bn.E2.neg(bn.G2)),
        ("O, G2", None, bn.G2),
        ("G1, O", bn.G1, None),
    ]
    out = []
    for name, p1, p2 in pairs:
        e = pairing_mod.optimal_ate(twist_point(p2), g1_point(p1))
        out.append({"name": name, "g1": None if p1 is None else [hx(v) for v in p1],
                    "g2": None if p2 is None else [hx(v) for v in (*p2[0], *p2[1])],
                    "gt": gt_hex(e)})
        print("pairing:", name, "->", out[-1]["gt"][:2], flush=True)
    return out


# ---- (b) one Pinocchio instance and the reference's verify ------------------------------------------------------

def pinocchio_case(pairing_mod, seed):
    sys.modules["verifiable_mpc.ac20.pairing"] = pairing_mod
    from mpyc.finfields import GF                                    # (shim)
    from mpyc.fingroups import EllipticCurve                         # (shim)
    import verifiable_mpc.trinocchio.pynocchio as pynocchio          # (reference)
    import verifiable_mpc.tools.code_to_qap as c2q
    import verifiable_mpc.tools.qap_creator as qc

    def as_pairing_point(pt):
        v = pt.value
        if isinstance(v[0], tuple):
            return twist_point(v)
        return g1_point(v)

    # the reference's pairing on the shim's points (optimal_ate reads .x/.y/.z, which the shim does not have)
    pynocchio.optimal_ate = lambda q, p: pairing_mod.optimal_ate(
        Twist.identity if q.value is None else as_pairing_point(q),
        G1pt.identity if p.value is None else as_pairing_point(p))

    bn_curve = EllipticCurve("BN256", "jacobian")
    bn_twist = EllipticCurve("BN256_twist", "jacobian")
    g1, g2 = bn_curve.generator, bn_twist.generator
    modulus = bn_curve.order
    gf = GF(modulus=modulus)
    gf.is_signed = False
    pynocchio.prng = random.Random(seed)
    code = """
def qeval(x):
    y = x**3 + x**2 + x
    return y + x + 5
"""
    qap = c2q.QAP(code, gf)
    td = pynocchio.Trapdoor(modulus)
    gen = pynocchio.Generators(td, g1, g2)
    evalkey = pynocchio.generate_evalkey(td, qap, gen)
    verikey = pynocchio.generate_verikey(td, qap, gen)
    c = qap.calculate_witness([gf(3)])
    p_poly = pynocchio.compute_p_poly(qap, c)
    h, r = p_poly / qap.t
    assert r == qc.Poly([0] * qap.d)
    deltas = pynocchio.SampleDeltas(modulus)
    h = h + pynocchio.compute_h_zk_terms(qap, c, deltas)
    proof = pynocchio.compute_proof(qap, c, h, evalkey, deltas)
    verification = pynocchio.verify(qap, verikey, proof, c)
    print("pinocchio verify:", verification, flush=True)
    assert all(verification.values())

    def enc(pt):
        v = pt.value
        if v is None:
            return None
        flat = []
        for cpt in v:
            flat += list(cpt) if isinstance(cpt, tuple) else [cpt]
        return [hx(x) for x in flat]
    return {"seed": seed, "indices_io": list(qap.indices_io), "indices_mid": list(qap.indices_mid),
            "c": [format(int(v) % modulus, "x") for v in c],
            "h": [format(int(v) % modulus, "x") for v in h.coeffs],
            "deltas": [format(int(d) % modulus, "x") for d in (deltas.v, deltas.w, deltas.y)],
            "verikey": {k: enc(v) for k, v in verikey.items()},
            "evalkey": {k: enc(v) for k, v in evalkey.items()},
            "proof": {k: enc(v) for k, v in proof.items()},
            "verification": verification}


def main():
    pairing_mod = load_reference_pairing()
    out = {"pairing": pairing_cases(pairing_mod, random.Random(SEED)),
           "pinocchio": pinocchio_case(pairing_mod, SEED + 1)}
    with open(os.path.join(HERE, "bn256_pairing.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("bn256_pairing.json written")


if __name__ == "__main__":
    main()
