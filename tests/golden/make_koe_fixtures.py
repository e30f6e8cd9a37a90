#!/usr/bin/env python3
"""Generate tests/golden/koe_bn256.json by running the REFERENCE's own knowledge-of-exponent pivot.

Needs a checkout of the reference (read-only), named by VMPC_REFERENCE:
    VMPC_REFERENCE=<reference checkout> python3 -B tests/golden/make_koe_fixtures.py
The reference's verifiable_mpc/ac20/knowledge_of_exponent.py runs unmodified over the mpyc shim's BN-256 groups,
switched to multiplicative notation as the reference's demo does, and over its own pairing.py through the stand-ins of
make_pairing_fixtures.py (the shim has no extension field).  Its `prng` is a seeded generator that records what
trusted_setup draws (g_exp, alpha, z, in that order).
Cases: n = 1, 5 and 32, each with a linear form and an affine form with a non-zero constant; at n = 5 also a
restriction argument over a proper subset S; and n = 4 with x = 0 and gamma = 0 (P, pi and Q are the point at infinity).
The fixture is DATA (points, scalars, the verifier's answers); no reference source text is stored.
Points are hex affine coordinates (G1: x, y; twist: x.re, x.im, y.re, y.im), null = the point at infinity.
Last, the reference's prover is timed at n = 2^8 on this host (printed only; DESIGN.md section 12 quotes it).
"""
import json
import os
import random
import sys
import time
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_pairing_fixtures as mp                                   # noqa: E402 (paths, stand-ins, reference pairing)

SEED = 20201529


class RecordingRandom(random.Random):
    def seed(self, *a, **k):
        super().seed(*a, **k)
        self.draws = []

    def randrange(self, *a, **k):
        v = super().randrange(*a, **k)
        self.draws.append(v)
        return v


def load_reference():
    pairing_mod = mp.load_reference_pairing()
    sys.modules["verifiable_mpc.ac20.pairing"] = pairing_mod
    import verifiable_mpc.ac20.knowledge_of_exponent as koe          # (reference)

    def as_pairing_point(pt):
        v = pt.value
        if v is None:
            return mp.Twist.identity if pt.is_twist else mp.G1pt.identity
        return mp.twist_point(v) if isinstance(v[0], tuple) else mp.g1_point(v)

    # the reference's pairing on the shim's points (optimal_ate reads .x/.y/.z, which the shim does not have)
    koe.pairing = types.SimpleNamespace(
        optimal_ate=lambda q, p: pairing_mod.optimal_ate(as_pairing_point(q), as_pairing_point(p)))
    return koe


def enc(pt):
    v = pt.normalize().value
    if v is None:
        return None
    flat = []
    for c in v:
        flat += list(c) if isinstance(c, tuple) else [c]
    return [mp.hx(x) for x in flat]


def main():
    koe = load_reference()
    from mpyc.finfields import GF                                    # (shim)
    from mpyc.fingroups import EllipticCurve                         # (shim)
    import verifiable_mpc.ac20.pivot as pivot                        # (reference)

    group1, group2 = EllipticCurve("BN256", "jacobian"), EllipticCurve("BN256_twist", "jacobian")
    for g, twist in ((group1, False), (group2, True)):
        g.is_additive, g.is_multiplicative, g.is_twist = False, True, twist
    order = group1.order
    gf = GF(modulus=order)
    g1, g2 = group1.generator, group2.generator
    rng = random.Random(SEED)
    hexs = lambda vals: [format(int(v) % order, "x") for v in vals]

    def setup(n, seed):
        koe.prng = RecordingRandom(seed)
        pp = koe.trusted_setup(g1, g2, n, order)
        g_exp, alpha, z = koe.prng.draws
        return pp, {"n": n, "g_exp": format(g_exp, "x"), "alpha": format(alpha, "x"), "z": format(z, "x"),
                    "pp_lhs": [enc(p) for p in pp["pp_lhs"]], "pp_rhs": [enc(p) for p in pp["pp_rhs"]]}

    def opening(pp, L, x, gamma, name):
        proof, u = koe.opening_linear_form_prover(L, x, gamma, pp)
        verification = koe.opening_linear_form_verifier(L, pp, proof, u)
        print(name, verification, flush=True)
        assert all(verification.values())
        return {"name": name, "x": hexs(x), "gamma": format(int(gamma) % order, "x"), "L": hexs(L.coeffs),
                "constant": format(int(L.constant) % order, "x"), "P": enc(proof["P"]), "pi": enc(proof["pi"]),
                "Q": enc(proof["Q"]), "u": format(int(u) % order, "x"), "verification": verification}

    out = {"seed": SEED, "setups": []}
    for k, n in enumerate((1, 5, 32)):
        pp, rec = setup(n, SEED + k)
        rec["openings"], rec["restrictions"] = [], []
        x = [gf(rng.randrange(order)) for _ in range(n)]
        gamma = gf(rng.randrange(order))
        coeffs = [gf(rng.randrange(order)) for _ in range(n)]
        rec["openings"].append(opening(pp, pivot.LinearForm(coeffs), x, gamma, f"linear n={n}"))
        coeffs = [gf(rng.randrange(order)) for _ in range(n)]
        rec["openings"].append(opening(pp, pivot.AffineForm(coeffs, gf(rng.randrange(1, order))), x, gamma,
                                       f"affine n={n}"))
        if n == 5:
            S = [0, 2, 3]
            P, pi = koe.restriction_argument_prover(S, x, gamma, pp)
            ok = koe.restriction_argument_verifier(P, pi, pp)
            print("restriction", S, ok, flush=True)
            rec["restrictions"].append({"S": S, "x": hexs(x), "gamma": format(int(gamma) % order, "x"),
                                        "P": enc(P), "pi": enc(pi), "verification": ok})
        out["setups"].append(rec)
    # x = 0 and gamma = 0: P, pi, Q are the point at infinity, u = 0, and the reference's verifier accepts
    n = 4
    pp, rec = setup(n, SEED + 9)
    rec["restrictions"] = []
    coeffs = [gf(rng.randrange(order)) for _ in range(n)]
    rec["openings"] = [opening(pp, pivot.LinearForm(coeffs), [gf(0)] * n, gf(0), "zero witness n=4")]
    assert rec["openings"][0]["P"] is None and rec["openings"][0]["Q"] is None and rec["openings"][0]["u"] == "0"
    out["setups"].append(rec)
    with open(os.path.join(HERE, "koe_bn256.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("koe_bn256.json written", flush=True)

    # the reference's own prover on this host (pure Python over the shim), for DESIGN.md section 12
    n = 1 << 8
    t0 = time.perf_counter()
    pp, _ = setup(n, SEED + 20)
    t1 = time.perf_counter()
    x = [gf(rng.randrange(order)) for _ in range(n)]
    L = pivot.LinearForm([gf(rng.randrange(order)) for _ in range(n)])
    koe.opening_linear_form_prover(L, x, gf(rng.randrange(order)), pp)
    t2 = time.perf_counter()
    print(f"reference on this host, n = 2^8: trusted_setup {t1 - t0:.2f} s, opening_linear_form_prover {t2 - t1:.2f} s",
          flush=True)


if __name__ == "__main__":
    main()
