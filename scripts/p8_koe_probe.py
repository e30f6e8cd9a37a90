"""Protocol 8 over BN-256 with the knowledge-of-exponent pivot, stage by stage (verifiable_mpc_amd/circuit_sat_gpu.py,
knowledge_of_exponent.py) -> profiles/p8_koe_probe.jsonl.

    python scripts/p8_koe_probe.py [--sizes 10,14,16] [--reps 7] [--warmup 2] [--out profiles/p8_koe_probe.jsonl]

Per m = 2^k on the product chain x^(m+1) (gate i = gate (i-1) * x: depth m, the triples are m launches): medians of
`reps` runs after `warmup` runs, each bracketed by a stream synchronisation, of
    setup        trusted_setup for N = 4 + 2m scalars (2N points a side), and the circuit's device tables
    triples, extension, P / pi MSMs (restriction_argument_prover over the device z), forms (Lagrange vectors + column
    sums), product (stage + polynomial product + split), Q MSM
    prove, verify  circuit_sat_prover / circuit_sat_verifier whole
under the default modes ("default": direct extension, schoolbook product) and under cs_extension("auto") +
poly_product("auto") ("auto").  Beside them, from the same run: the Ed25519 compressed-pivot prove and verify of the
same circuit shape (x padded so that N + 1 is a power of two), and both proofs' sizes in bytes on the wire (points
compressed where the format has it: 32 bytes an Ed25519 point; BN-256 points as the affine 64 / 128 bytes this package
sends)."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def chain(m):
    return 1, (list(range(m + 1)), [0] + list(range(1, m)), np.ones(m, np.int64)), \
        (list(range(m + 1)), [0] * m, np.ones(m, np.int64)), ([0, 1], [m], np.ones(1, np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/p8_koe_probe.jsonl")
    args = ap.parse_args()
    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    from verifiable_mpc_amd import knowledge_of_exponent as koe
    from verifiable_mpc_amd.device import BnScalarVector
    ctx = vm.get_context()
    P = vm.pynocchio
    order = P.ORDER
    gf_n = vm.GF(order)
    # the generators: (1, -2) and the twist generator of the reference's pairing.py
    from oracle import bn256_ref as bn
    g1, g2 = P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2)
    group = vm.EllipticCurve("Ed25519", "projective")
    gf_l = vm.GF(group.order)
    rng = np.random.default_rng(29)

    def timed(fn):
        out, r = [], None
        for i in range(args.warmup + args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            if i >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), max(out) - min(out), r

    with open(args.out, "w") as f:        # a run replaces the file
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for k in [int(s) for s in args.sizes.split(",")]:
            m = 1 << k
            n_x, A, B, O = chain(m)
            x = [3]
            N = 1 + 3 + 2 * m
            t0 = time.perf_counter()
            pp = koe.trusted_setup(g1, g2, N, order)
            ctx.sync()
            setup_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            sc = cs.SparseCircuit(n_x, A, B, O, order=order)
            d = sc.device()
            ctx.sync()
            circuit_ms = (time.perf_counter() - t0) * 1e3
            levels = len(sc.level_ptr) - 1
            for mode, ext, prod in (("default", "direct", "schoolbook"), ("auto", "auto", "auto")):
                with contextlib.ExitStack() as stack:
                    stack.enter_context(vm.device.cs_extension(ext))
                    stack.enter_context(vm.device.poly_product(prod))
                    row = {"pivot": "koe", "modes": mode, "m": m, "N": N, "levels": levels, "reps": args.reps,
                           "warmup": args.warmup, "trusted_setup_ms": setup_ms, "circuit_setup_ms": circuit_ms}
                    z = BnScalarVector.from_ints(x + [0] * (N - 1), ctx)
                    a, b = BnScalarVector.from_ints([0] * m + [5], ctx), BnScalarVector.from_ints([0] * m + [7], ctx)

                    def triples():
                        for lv in range(levels):
                            lo, hi = int(sc.level_ptr[lv]), int(sc.level_ptr[lv + 1])
                            ctx.cs_triples(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, n_x, 4, z.ptr,
                                           a.ptr, b.ptr, bn=True)
                    row["triples_ms"], row["triples_spread_ms"], _ = timed(triples)
                    row["extension_ms"], row["extension_spread_ms"], _ = timed(
                        lambda: ctx.cs_extend(a.ptr, b.ptr, m, d["fact"].ptr, d["ifact"].ptr, z.ptr + 32, bn=True))
                    row["commit_msms_ms"], row["commit_msms_spread_ms"], _ = timed(
                        lambda: koe.restriction_argument_prover(range(N), z, 99, pp))
                    c = 2 * m + 12345
                    row["forms_ms"], row["forms_spread_ms"], forms = timed(lambda: cs._Forms(sc, 1, c, order))
                    L = forms.combine(7, forms.values(z), [0], gf_n)
                    c_bar, d_u = ctx.alloc(32 * 2 * N), ctx.alloc(32)

                    def product():
                        lhs, rhs = koe._staged(ctx, z, 99, L.coeffs)
                        ctx.bn256_fr_poly_mul(lhs.ptr, N + 1, rhs.ptr, N, c_bar.ptr)
                        ctx.bn256_koe_split(c_bar.ptr, N, d_u.ptr)
                    row["product_ms"], row["product_spread_ms"], _ = timed(product)
                    row["q_msm_ms"], row["q_msm_spread_ms"], _ = timed(lambda: koe._side(ctx, pp, "pp_lhs").msm((c_bar, 2 * N)))
                    row["prove_ms"], row["prove_spread_ms"], proof = timed(
                        lambda: cs.circuit_sat_prover(pp, sc, x, gf_n, "koe"))
                    row["verify_ms"], row["verify_spread_ms"], verdict = timed(
                        lambda: cs.circuit_sat_verifier(proof, pp, sc, gf_n, "koe"))
                    row["verified"] = verdict == {"y1*y2=y3": True, "L_wellformed_from_Cfgh_forms": True,
                                                  "pivot_verification": {"restriction_arg_check": True, "PRQ_check": True}}
                    row["pivot_proof_bytes"] = sum(len(proof["pivot_proof"][q].to_bytes()) for q in ("P", "pi", "Q"))
                    row["proof_bytes"] = row["pivot_proof_bytes"] + 32 * (3 + len(proof["outputs"]) + N + 1)
                    emit(row)
                    del z, a, b, forms, L, c_bar, proof
            del pp, sc, d
            ctx.trim()

            # the same circuit shape over Ed25519 with the compressed pivot, same run
            sc_l = cs.SparseCircuit(n_x, A, B, O)
            x_l = sc_l.pad([3])
            N_l = len(x_l) + 3 + 2 * m
            exps = rng.integers(0, 256, size=(N_l, 32), dtype=np.uint8)
            exps[:, 31] &= 0x0f
            g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
            gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 12345)}
            g.precompute([gens["h"], gens["k"]], wide=N_l >= (1 << 19) - 1)
            row = {"pivot": "compressed", "modes": "default", "m": m, "N": N_l, "reps": args.reps, "warmup": args.warmup}
            row["prove_ms"], row["prove_spread_ms"], proof = timed(lambda: cs.circuit_sat_prover(gens, sc_l, x_l, gf_l))
            row["verify_ms"], row["verify_spread_ms"], verdict = timed(
                lambda: cs.circuit_sat_verifier(proof, gens, sc_l, gf_l))
            row["verified"] = all(verdict.values()) and len(verdict) == 3
            pv = proof["pivot_proof"]
            rounds = (N_l + 1).bit_length() - 1
            # Protocol 5's proof: t, A, and per halving round A_i, B_i (32-byte points), then the two last scalars
            row["pivot_proof_points"] = sum(1 for v in _flatten(pv) if hasattr(v, "normalize") or hasattr(v, "coords"))
            row["pivot_proof_bytes"] = 32 * len(list(_flatten(pv)))
            row["halving_rounds"] = rounds
            row["proof_bytes"] = row["pivot_proof_bytes"] + 32 * (1 + 3 + len(proof["outputs"]) + N_l + 1)
            emit(row)
            del g, gens, proof, sc_l
            ctx.trim()


def _flatten(v):
    """the group elements and scalars of a pivot proof, one by one (each is 32 bytes on the wire)"""
    if isinstance(v, dict):
        for w in v.values():
            yield from _flatten(w)
    elif isinstance(v, (list, tuple)):
        for w in v:
            yield from _flatten(w)
    elif hasattr(v, "to_ints"):
        yield from v.to_ints()
    else:
        yield v


if __name__ == "__main__":
    main()
