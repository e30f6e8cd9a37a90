#!/usr/bin/env python3
"""Generate tests/golden/nullity_ed25519.json by running the REFERENCE's own verifiable_mpc/ac20/nullity.py (over its
pivot.py and compressed_pivot.py) on tests/golden/mpyc_shim, with seeded prngs (the way make_fixtures.py imports them;
needs the reference checkout, read-only):
    python3 -B tests/golden/make_nullity_fixtures.py
Cases (s forms, n = len(x), n + 1 a power of two as Protocol 5 requires): (1, 3), (3, 7), (5, 15), each once with
Python-int coefficients (negative ones included; rho^i then grows them unreduced) and once with field elements.  Every
form vanishes on x except in the case "3x7_field_nonzero", where form 1 does not and y != 0: the reference proves
whatever y is.  Recorded per case: the generators' exponents (create_generators' draw order), x, gamma, the forms,
un-normalised [P], Protocol 5's masks, rho, L, y, the whole proof with its representatives, every Fiat-Shamir hash and
the verifier's answer ("i:<decimal>" = Python int, "f:<hex>" = field element).  DATA only."""
import json
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import Recorder, compressed_pivot, cs_r1cs, group_and_field, hx, pivot, pt_proj_hex, typed   # noqa: E402

import verifiable_mpc.ac20.nullity as nullity          # noqa: E402 (reference)

SEED = 20200317


def vanishing_forms(rng, s, n, x, gf, ints):
    """s forms with L_i(x) = 0: n - 1 free coefficients, the last one solved for.  ints: small Python ints of both
    signs (the solved one is a residue held as an int); else field elements."""
    order = gf.order
    forms = []
    for _ in range(s):
        free = [rng.randrange(-50, 50) for _ in range(n - 1)] if ints else \
            [gf(rng.randrange(order)) for _ in range(n - 1)]
        acc = sum(c * v for c, v in zip(free, x[:-1]))
        last = -acc / x[-1]
        forms.append(pivot.LinearForm(free + [int(last) if ints else last]))
    return forms


def case(name, s, n, seed, ints, nonzero_form=None):
    group, gf = group_and_field()
    order = gf.order
    rng = random.Random(seed)
    cs_r1cs.prng = random.Random(seed + 1)
    st = cs_r1cs.prng.getstate()
    generators = cs_r1cs.create_generators(n, cs_r1cs.PivotChoice.compressed, group)
    replay = random.Random()
    replay.setstate(st)
    exps = [replay.randrange(1, order) for _ in range(n)]
    exp_k = replay.randrange(1, order)
    x = [gf(rng.randrange(1, order)) for _ in range(n)]
    gamma = rng.randrange(1, order)
    lin_forms = vanishing_forms(rng, s, n, x, gf, ints)
    if nonzero_form is not None:
        lin_forms[nonzero_form].coeffs[0] = lin_forms[nonzero_form].coeffs[0] + 1
    values = [f(x) for f in lin_forms]
    assert all((int(v) % order == 0) == (i != nonzero_form) for i, v in enumerate(values))
    P = pivot.vector_commitment(x, gamma, generators["g"], generators["h"])
    compressed_pivot.prng = random.Random(seed + 2)
    st = compressed_pivot.prng.getstate()
    with Recorder() as rec:
        proof, L, y, rho = nullity.prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf)
        n_prover = len(rec.calls)
        ok = nullity.verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf)
    replay.setstate(st)
    r = [replay.randrange(order) for _ in range(n)]
    mask = replay.randrange(order)
    assert ok is True and (int(y) % order != 0) == (nonzero_form is not None)
    rounds = (n + 1).bit_length() - 2
    return {
        "name": name, "s": s, "n": n, "seed": seed, "rounds": rounds,
        "gen_exponents": [hx(e) for e in exps], "gen_exponent_k": hx(exp_k),
        "x_typed": [typed(v, order) for v in x], "gamma": hx(gamma),
        "forms_typed": [[typed(c, order) for c in f.coeffs] for f in lin_forms],
        "values": [hx(int(v) % order) for v in values],
        "P_proj": pt_proj_hex(P),
        "r": [hx(v) for v in r], "mask": hx(mask),
        "rho": hx(rho),
        "L_typed": [typed(c, order) for c in L.coeffs], "L_constant_typed": typed(L.constant, order),
        "L_is_linear_form": isinstance(L, pivot.LinearForm),
        "y_typed": typed(y, order),
        "proof_keys": list(proof.keys()),
        "proof": {"t_typed": typed(proof["t"], order), "A_proj": pt_proj_hex(proof["A"]),
                  "A_i_proj": [pt_proj_hex(proof[f"A{i}"]) for i in range(rounds)],
                  "B_i_proj": [pt_proj_hex(proof[f"B{i}"]) for i in range(rounds)],
                  "z_prime_typed": [typed(v, order) for v in proof["z_prime"]]},
        "hashes": rec.calls[:n_prover],          # rho, c0, c1, then one per round
        "verifier_hashes": rec.calls[n_prover:],
        "verified": ok,
    }


if __name__ == "__main__":
    cases = [case("1x3_int", 1, 3, SEED, True), case("3x7_int", 3, 7, SEED + 10, True),
             case("5x15_int", 5, 15, SEED + 20, True), case("1x3_field", 1, 3, SEED + 30, False),
             case("3x7_field_nonzero", 3, 7, SEED + 40, False, nonzero_form=1),
             case("5x15_field", 5, 15, SEED + 50, False)]
    out = os.path.join(HERE, "nullity_ed25519.json")
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/make_nullity_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print(out, os.path.getsize(out), [(c["name"], c["verified"]) for c in cases])
