"""Stage times of Protocol 8 on the device (verifiable_mpc_amd/circuit_sat_gpu.py) -> profiles/circuit_sat_probe.jsonl.

    python scripts/circuit_sat_probe.py [--sizes 10,12,14,16] [--reps 5] [--out profiles/circuit_sat_probe.jsonl]

Per circuit (an inner product: depth 1; a product chain: depth = m) and m = 2^k: medians over `reps` runs, each
bracketed by a stream synchronisation, of the triples (with the number of launches), the extension, the Lagrange
vectors + form assembly, the commitment, the compressed pivot's prove on its own (protocol_5_prover with its masks
supplied), and the whole circuit_sat_prover / circuit_sat_verifier (medians too, after a warm-up run).  `--host-naive
64,128` times the restatement's naive route (tests/p8_ref.py: interpolate, multiply, evaluate - what the reference
does, cubic in m) on the host for scale.  Beside the extension, in
the same run: vmpc_bn256_fr_poly_mul_dev on two m-term vectors (m^2 multiply-accumulates over the other 254-bit field;
the extension does 2 m^2) - the ratio of time per multiply-accumulate is the figure DESIGN.md section 15 reports."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def circuits(kind, m):
    if kind == "inner":        # sum x_i y_i: m independent gates, one output
        n_x = 2 * m
        A = (list(range(m + 1)), list(range(m)), np.ones(m, np.int64))
        B = (list(range(m + 1)), list(range(m, 2 * m)), np.ones(m, np.int64))
        O = ([0, m], list(range(n_x, n_x + m)), np.ones(m, np.int64))
    else:                      # x^(m+1): gate i = gate (i-1) * x
        n_x = 1
        A = (list(range(m + 1)), [0] + list(range(1, m)), np.ones(m, np.int64))
        B = (list(range(m + 1)), [0] * m, np.ones(m, np.int64))
        O = ([0, 1], [m], np.ones(1, np.int64))
    return n_x, A, B, O


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,12,14,16")
    ap.add_argument("--kinds", default="inner,chain")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-naive", default="")
    ap.add_argument("--out", default="profiles/circuit_sat_probe.jsonl")
    args = ap.parse_args()
    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    ctx = vm.get_context()
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    rng = np.random.default_rng(8)

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), r

    with open(args.out, "w") as f:        # a run replaces the file
        for m in [int(v) for v in args.host_naive.split(",") if v]:
            import random
            from tests import p8_ref
            hr = random.Random(m)
            av, bv = ([hr.randrange(p8_ref.ELL) for _ in range(m)] for _ in range(2))
            t0 = time.perf_counter()
            p8_ref.z_tail_naive(av, bv, 5, 7)
            line = json.dumps({"kind": "host_naive_z_tail", "m": m, "seconds": time.perf_counter() - t0})
            print(line, flush=True)
            f.write(line + "\n")
        for k in [int(s) for s in args.sizes.split(",")]:
            m = 1 << k
            for kind in args.kinds.split(","):
                n_x, A, B, O = circuits(kind, m)
                t0 = time.perf_counter()
                sc = cs.SparseCircuit(n_x, A, B, O)
                d = sc.device()
                ctx.sync()
                host_ms = (time.perf_counter() - t0) * 1e3
                x = sc.pad([3] * n_x if kind == "inner" else [1])
                n_in, N = len(x), len(x) + 3 + 2 * m
                exps = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
                exps[:, 31] &= 0x0f
                g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
                gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 12345)}
                g.precompute([gens["h"], gens["k"]], wide=N >= (1 << 19) - 1)
                z = vm.ScalarVector.empty(N, ctx)
                ctx.upload_into(z.ptr, vm.sparse.residue_array(x, group.order))
                a, b = vm.ScalarVector.from_ints([0] * m + [5], ctx), vm.ScalarVector.from_ints([0] * m + [7], ctx)
                levels = len(sc.level_ptr) - 1

                def triples():
                    for lv in range(levels):
                        lo, hi = int(sc.level_ptr[lv]), int(sc.level_ptr[lv + 1])
                        ctx.cs_triples(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, n_x, n_in + 3, z.ptr,
                                       a.ptr, b.ptr)
                reps = args.reps if k <= 16 else 1
                row = {"kind": kind, "m": m, "N": N, "levels": levels, "circuit_setup_ms": host_ms, "reps": reps}
                row["triples_ms"], _ = timed(triples, reps)
                row["extension_ms"], _ = timed(lambda: ctx.cs_extend(a.ptr, b.ptr, m, d["fact"].ptr, d["ifact"].ptr,
                                                                     z.ptr + 32 * n_in), reps)
                # the relative: an m x m product over BN-256's scalar field, same run
                pa = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
                pa[:, 31] &= 0x1f                   # below 2^253 < n: canonical operands
                pa = ctx.upload(pa)
                pout = ctx.alloc(32 * 2 * m)
                p = ctypes.c_void_p
                row["bn_poly_mul_ms"], _ = timed(lambda: ctx.lib.vmpc_bn256_fr_poly_mul_dev(
                    ctx.handle, p(pa.ptr), m, p(pa.ptr), m, p(pout.ptr)), reps)
                row["ns_per_mac_extension"] = row["extension_ms"] * 1e6 / (2.0 * m * m)
                row["ns_per_mac_bn_poly_mul"] = row["bn_poly_mul_ms"] * 1e6 / (1.0 * m * m)
                row["extension_over_poly_mul"] = row["ns_per_mac_extension"] / row["ns_per_mac_bn_poly_mul"]
                c = 2 * m + 12345
                row["lagrange_assembly_ms"], forms = timed(lambda: cs._Forms(sc, n_in, c, gf.order), reps)
                row["commitment_ms"], _ = timed(lambda: vm.pivot.vector_commitment(z, 99, g, gens["h"]), reps)
                # the pivot on its own: Protocol 5 over (z, [z], L) as Protocol 8 hands them over, masks supplied
                p8 = cs.protocol_8_excl_pivot_prover(gens, sc, x, gf)
                _, zc, L, zv, gm = p8
                y = L(zv)
                row["pivot_prove_ms"], _ = timed(lambda: vm.compressed_pivot.protocol_5_prover(
                    gens, zc, L, y, zv, gm, gf, transcript="compact", r=vm.compressed_pivot.masks(N, ctx), rho=12345), reps)
                row["p8_excl_pivot_ms"], _ = timed(lambda: cs.protocol_8_excl_pivot_prover(gens, sc, x, gf), reps)
                proof = cs.circuit_sat_prover(gens, sc, x, gf)          # warm-up
                row["prove_total_ms"], proof = timed(lambda: cs.circuit_sat_prover(gens, sc, x, gf), reps)
                row["verify_total_ms"], verdict = timed(lambda: cs.circuit_sat_verifier(proof, gens, sc, gf), reps)
                row["verified"] = all(verdict.values()) and len(verdict) == 3
                if levels > 1:
                    row["us_per_level"] = row["triples_ms"] * 1e3 / levels
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                del g, gens, proof, forms, p8, zc, L, zv
                ctx.trim()


if __name__ == "__main__":
    main()
