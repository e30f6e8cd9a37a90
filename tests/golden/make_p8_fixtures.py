#!/usr/bin/env python3
"""Generate tests/golden/p8_circuits.json by running the REFERENCE's own circuit_builder and
circuit_sat_cb.protocol_8_excl_pivot_prover over tests/golden/mpyc_shim, with seeded prngs (the way make_fixtures.py
imports them; needs the reference checkout, read-only):
    python3 -B tests/golden/make_p8_fixtures.py
Four circuits: a product chain x**6 (depth = m), an inner product (depth 1), one with scalar-mul and constant wires
and two outputs, and one with int inputs that needs padding (padded the way demos/demo_zkp_ac20.py pads).  Recorded per
circuit: the gates as data, x, r_a, r_b, gamma, the reference's affine forms A, B, O, its a, b, c, z (typed), both
hashes, y1..y3, outputs, circuit_forms, lin_forms and L (typed: "i:<decimal>" = Python int, "f:<hex>" = field element),
and the un-normalised [z].  DATA only."""
import json
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import Recorder, cs_r1cs, group_and_field, hx, pivot, pt_proj_hex, typed   # noqa: E402

import verifiable_mpc.ac20.circuit_builder as cb          # noqa: E402 (reference)
import verifiable_mpc.ac20.circuit_sat_cb as cs_cb        # noqa: E402 (reference)


def chain(circuit, gf):
    x = cb.CircuitVar(gf(3), circuit, "x")
    (x ** 6).label_output("y")


def inner(circuit, gf):
    xs = [cb.CircuitVar(gf(v), circuit, "a") for v in (2, 3, 5, 7)]
    ys = [cb.CircuitVar(gf(v), circuit, "b") for v in (11, 13, 17, 19)]
    acc = xs[0] * ys[0]
    for u, v in zip(xs[1:], ys[1:]):
        acc = acc + u * v
    acc.label_output("ip")


def mixed(circuit, gf):
    a, b, c = (cb.CircuitVar(gf(v), circuit, n) for v, n in ((4, "a"), (9, "b"), (25, "c")))
    t = 3 * (a * b) + c + 7
    u = (t - a) * (b + 2)
    (u * u).label_output("u2")
    (5 * t - 1).label_output("t5")


def padded(circuit, gf):
    a, b, c = (cb.CircuitVar(v, circuit, n) for v, n in ((1, "a"), (2, "b"), (3, "c")))
    d = a * b + c
    e = d * (a - 2 * b)
    (e * d + 1).label_output("e")
    x = circuit.initial_inputs()
    _, padding, _ = cs_cb.check_input_length_power_of_2(x, circuit)
    for i in range(padding):
        cb.CircuitVar(0, circuit, "unused_" + str(i))


def form_rec(f, order):
    return {"coeffs": [typed(v, order) for v in f.coeffs], "constant": typed(f.constant, order)}


def operand(v, order):
    if isinstance(v, cb.CircuitVar):
        return {"var": v.name, "input_index": v.input_index}
    return {"const": typed(v, order)}


def case(name, build, seed):
    group, gf = group_and_field()
    order = gf.order
    circuit = cb.Circuit()
    build(circuit, gf)
    x = circuit.initial_inputs()
    n = len(x)
    N = n + 3 + 2 * circuit.mul_ct
    rng = random.Random(seed)
    exps = [rng.randrange(1, order) for _ in range(N)]
    gens = {"g": [group.generator ** e for e in exps], "h": group.generator}
    for i, mod in enumerate((cs_r1cs, cs_cb, cb)):
        mod.prng = random.Random(seed + 10 + i)
    st_fgh, st_gamma = cs_r1cs.prng.getstate(), cs_cb.prng.getstate()
    with Recorder() as rec:
        proof, z_commitment, L, z, gamma = cs_cb.protocol_8_excl_pivot_prover(gens, circuit, x, gf)
    replay = random.Random()
    replay.setstate(st_fgh)
    r_a, r_b = replay.randrange(1, order), replay.randrange(1, order)
    replay.setstate(st_gamma)
    assert replay.randrange(1, order) == gamma
    c1 = int(rec.calls[0]["c"], 16)
    lf = cb.calculate_fg_form(circuit, wire=0, challenge=c1, gf=gf)
    lg = cb.calculate_fg_form(circuit, wire=1, challenge=c1, gf=gf)
    lh = cb.calculate_h_form(circuit, c1, gf)
    circuit_forms = [cb.convert_to_ac20(f, circuit) for f in cb.calculate_circuit_forms(circuit)]
    lin_forms = [f - y for f, y in zip(circuit_forms, proof["outputs"])] + [lf - proof["y1"], lg - proof["y2"], lh - proof["y3"]]
    a, b, c = circuit.multiplication_triples(x)
    muls = circuit.mul_gates()
    verification, L_v = cs_cb.protocol_8_excl_pivot_verifier(proof, circuit, gf)
    assert verification == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True}
    return {
        "name": name, "seed": seed, "input_ct": circuit.input_ct, "mul_ct": circuit.mul_ct,
        "output_gates": list(circuit.output_gates), "circuit_str": str(circuit),
        "gates": [{"op": g.op.name, "inputs": [operand(v, order) for v in g.inputs], "output": g.output.name,
                   "output_index": g.output.output_index, "mul_index": g.mul_index} for g in circuit.gates],
        "gen_exponents": [hx(e) for e in exps],
        "x_typed": [typed(v, order) for v in x], "r_a": hx(r_a), "r_b": hx(r_b), "gamma": hx(gamma),
        "A": [form_rec(cb.construct_affine_form(g, circuit, 0), order) for g in muls],
        "B": [form_rec(cb.construct_affine_form(g, circuit, 1), order) for g in muls],
        "O": [form_rec(f, order) for f in cb.calculate_circuit_forms(circuit)],
        "a_typed": [typed(v, order) for v in a], "b_typed": [typed(v, order) for v in b],
        "c_typed": [typed(v, order) for v in c],
        "z_typed": [typed(v, order) for v in z], "z_commitment_proj": pt_proj_hex(z_commitment),
        "hashes": rec.calls,
        "y_typed": [typed(proof[k], order) for k in ("y1", "y2", "y3")],
        "outputs_typed": [typed(v, order) for v in proof["outputs"]],
        "linform_f": form_rec(lf, order), "linform_g": form_rec(lg, order), "linform_h": form_rec(lh, order),
        "circuit_forms": [form_rec(f, order) for f in circuit_forms],
        "lin_forms": [form_rec(f, order) for f in lin_forms],
        "L": form_rec(L, order),
    }


if __name__ == "__main__":
    cases = [case("chain", chain, 81), case("inner", inner, 82), case("mixed", mixed, 83), case("padded", padded, 84)]
    out = os.path.join(HERE, "p8_circuits.json")
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/make_p8_fixtures.py", "cases": cases}, f, indent=0)
    print(out, os.path.getsize(out), [(c["name"], c["mul_ct"], c["input_ct"]) for c in cases])
