#!/usr/bin/env python3
"""Generate tests/golden/pinocchio_keygen.json by running the REFERENCE's own key generation.

Needs a checkout of the reference (read-only), named by VMPC_REFERENCE:
    VMPC_REFERENCE=<reference checkout> python3 -B tests/golden/make_keygen_fixtures.py
For each program below, with pynocchio.prng = random.Random(seed), over the mpyc shim's BN-256 groups: the reference's
code_to_qap.QAP, Trapdoor, Generators, generate_evalkey and generate_verikey, then the witness, SampleDeltas, the
zero-knowledge h, compute_proof and verify (with the reference's pairing.py, loaded as make_pairing_fixtures.py does).
Recorded: the program text and seed, the R1CS rows (code_to_r1cs.flatcode_to_r1cs), the dense QAP coefficients v, w,
y and t, the eight trapdoor values, both keys as ordered [name, point] lists, c, the deltas, h, the proof and the
verify result, plus the wall time of the reference's QAP construction and key generation on the generating host.
The fixture is DATA; no reference source text is stored.
"""
import json
import os
import random
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_pairing_fixtures as mpf                                 # noqa: E402  (checks VMPC_REFERENCE)

PROGRAMS = [
    # demos/demo_zkp_pynocchio.py:46-50
    ("demo", 20261016, """
def qeval(x):
    y = x**3 + x**2 + x
    return y + x + 5
""", [3]),
    ("larger", 20261017, """
def qeval(x, z):
    a = x**4 + 2*x**3*z + z**3
    b = a*a + x*z + 7
    c = b*x - a*z + z**2
    e = c*c - b + 3*a*z
    return e*a + c*b + 3*x + 11
""", [5, 7]),
]


def hx(v, mod):
    return format(int(v) % mod, "x")


def run_case(pairing_mod, name, seed, code, inputs):
    sys.modules["verifiable_mpc.ac20.pairing"] = pairing_mod
    from mpyc.finfields import GF                                    # (shim)
    from mpyc.fingroups import EllipticCurve                         # (shim)
    import verifiable_mpc.trinocchio.pynocchio as pynocchio          # (reference)
    import verifiable_mpc.tools.code_to_qap as c2q
    import verifiable_mpc.tools.code_to_r1cs as c2r
    import verifiable_mpc.tools.qap_creator as qc

    def as_pairing_point(pt):
        v = pt.value
        return mpf.twist_point(v) if isinstance(v[0], tuple) else mpf.g1_point(v)

    pynocchio.optimal_ate = lambda q, p: pairing_mod.optimal_ate(
        mpf.Twist.identity if q.value is None else as_pairing_point(q),
        mpf.G1pt.identity if p.value is None else as_pairing_point(p))
    bn_curve = EllipticCurve("BN256", "jacobian")
    bn_twist = EllipticCurve("BN256_twist", "jacobian")
    g1, g2 = bn_curve.generator, bn_twist.generator
    n = bn_curve.order
    gf = GF(modulus=n)
    gf.is_signed = False
    P = mpf.P

    t0 = time.perf_counter()
    qap = c2q.QAP(code, gf)
    t_qap = time.perf_counter() - t0
    inp, body = c2r.extract_inputs_and_body(c2r.parse(code))
    V, W, Y = c2r.flatcode_to_r1cs(inp, c2r.flatten_body(body))

    pynocchio.prng = random.Random(seed)
    td = pynocchio.Trapdoor(n)
    t0 = time.perf_counter()
    gen = pynocchio.Generators(td, g1, g2)
    evalkey = pynocchio.generate_evalkey(td, qap, gen)
    verikey = pynocchio.generate_verikey(td, qap, gen)
    t_keygen = time.perf_counter() - t0

    c = qap.calculate_witness([gf(v) for v in inputs])
    p_poly = pynocchio.compute_p_poly(qap, c)
    h, r = p_poly / qap.t
    assert r == qc.Poly([0] * qap.d)
    deltas = pynocchio.SampleDeltas(n)
    h = h + pynocchio.compute_h_zk_terms(qap, c, deltas)
    proof = pynocchio.compute_proof(qap, c, h, evalkey, deltas)
    verification = pynocchio.verify(qap, verikey, proof, c)
    print(f"{name}: d={qap.d} m={qap.m} qap {t_qap:.2f} s keygen {t_keygen:.2f} s verify {verification}", flush=True)
    assert all(verification.values())

    def enc(pt):
        v = pt.value
        if v is None:
            return None
        flat = []
        for cpt in v:
            flat += list(cpt) if isinstance(cpt, tuple) else [cpt]
        return [hx(x, P) for x in flat]

    def coeffs(poly):
        return [hx(x, n) for x in poly.coeffs]

    return {"name": name, "seed": seed, "code": code, "inputs": inputs,
            "d": qap.d, "m": qap.m, "out_ix": qap.out_ix,
            "r1cs": {"V": V, "W": W, "Y": Y},
            "qap": {"v": [coeffs(p) for p in qap.v], "w": [coeffs(p) for p in qap.w],
                    "y": [coeffs(p) for p in qap.y], "t": coeffs(qap.t)},
            "trapdoor": {k: hx(getattr(td, k), n) for k in
                         ("r_v", "r_w", "s", "alpha_v", "alpha_w", "alpha_y", "beta", "gamma", "r_y")},
            "evalkey": [[k, enc(v)] for k, v in evalkey.items()],
            "verikey": [[k, enc(v)] for k, v in verikey.items()],
            "c": [hx(v, n) for v in c],
            "deltas": [hx(x, n) for x in (deltas.v, deltas.w, deltas.y)],
            "h": [hx(v, n) for v in h.coeffs],
            "proof": {k: enc(v) for k, v in proof.items()},
            "verification": verification,
            "reference_seconds": {"qap": round(t_qap, 3), "keygen": round(t_keygen, 3)}}


def main():
    pairing_mod = mpf.load_reference_pairing()
    out = {"cases": [run_case(pairing_mod, *prog) for prog in PROGRAMS]}
    with open(os.path.join(HERE, "pinocchio_keygen.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("pinocchio_keygen.json written", os.path.getsize(os.path.join(HERE, "pinocchio_keygen.json")), "bytes")


if __name__ == "__main__":
    main()
