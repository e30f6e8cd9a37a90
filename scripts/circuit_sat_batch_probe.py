"""The batch Protocol 8 prover against K single calls of the same build -> profiles/circuit_sat_batch_probe.jsonl.

    python scripts/circuit_sat_batch_probe.py [--sizes 10,12] [--kinds inner,chain] [--batch 1,8,64] [--reps 3]

Per circuit (an inner product: depth 1; a product chain: depth = m), m = 2^k and K witnesses with distinct inputs: the
median over `reps` runs after one warm-up run, each run bracketed by a stream synchronisation, of every stage done once
for all K (`*_batch_ms`) and done K times the single way (`*_single_ms`):

    triples       one launch per depth level (batch: for all K; single: per witness)
    extension     vmpc_fr_cs_extend_batch_dev against K vmpc_fr_cs_extend_dev
    commitments   K commitments queued and collected together against K pivot.vector_commitment calls
    forms         K _Forms queued, their five scalars per witness read back together, against K _Forms + values()
    pivots        compressed_pivot.protocol_5_prover per witness, masks supplied: the same code on both sides, timed once
    p8            protocol_8_excl_pivot_prover_batch (xs as lists, and as one uint8 array) against K
                  protocol_8_excl_pivot_prover
    prove         circuit_sat_prover_batch against K circuit_sat_prover

The single entries run the batch entries' kernels with K = 1 (csrc/circuit_sat.hip)."""
import argparse
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
    ap.add_argument("--sizes", default="10,12")
    ap.add_argument("--kinds", default="inner,chain")
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/circuit_sat_batch_probe.jsonl")
    args = ap.parse_args()
    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    ctx = vm.get_context()
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    order = group.order
    rng = np.random.default_rng(9)

    def timed(fn):
        out = []
        for i in range(args.reps + 1):          # the first run warms up
            ctx.sync()
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            if i:
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), r

    with open(args.out, "w") as f:        # a run replaces the file
        for k in [int(s) for s in args.sizes.split(",")]:
            m = 1 << k
            for kind in args.kinds.split(","):
                n_x, A, B, O = circuits(kind, m)
                sc = cs.SparseCircuit(n_x, A, B, O)
                d = sc.device()
                n_in = n_x + sc.padding()
                N, M, g_off = n_in + 3 + 2 * m, m + 1, n_in + 3
                exps = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
                exps[:, 31] &= 0x0f
                g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
                gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 12345)}
                g.precompute([gens["h"], gens["k"]])
                levels = len(sc.level_ptr) - 1
                for K in [int(s) for s in args.batch.split(",")]:
                    rows = np.zeros((K, n_in, 32), np.uint8)
                    rows[:, :n_x] = rng.integers(0, 256, size=(K, n_x, 32), dtype=np.uint8)
                    rows[:, :, 31] &= 0x0f
                    xs = [[int.from_bytes(rows[p, i].tobytes(), "little") for i in range(n_in)] for p in range(K)]
                    draws = [(5 + 3 * p, 7 + 3 * p, 9 + 3 * p) for p in range(K)]
                    row = {"kind": kind, "m": m, "N": N, "levels": levels, "K": K, "reps": args.reps}
                    # ---- stage by stage, on one Z of K rows and on K vectors z
                    Z = cs._witnesses_on_device(sc, rows, n_in, draws)
                    a, b = (vm.ScalarVector.from_array(np.zeros((K * M, 32), np.uint8), ctx) for _ in range(2))
                    zs = [Z[p * N:(p + 1) * N] for p in range(K)]

                    def triples_batch():
                        for lv in range(levels):
                            lo, hi = int(sc.level_ptr[lv]), int(sc.level_ptr[lv + 1])
                            ctx.cs_triples_batch(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, n_x, g_off,
                                                 Z.ptr, N, a.ptr, b.ptr, M, K)

                    def triples_single():
                        for p in range(K):
                            for lv in range(levels):
                                lo, hi = int(sc.level_ptr[lv]), int(sc.level_ptr[lv + 1])
                                ctx.cs_triples(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, n_x, g_off,
                                               zs[p].ptr, a.ptr + 32 * p * M, b.ptr + 32 * p * M)
                    row["triples_batch_ms"], _ = timed(triples_batch)
                    row["triples_single_ms"], _ = timed(triples_single)
                    row["extension_batch_ms"], _ = timed(lambda: ctx.cs_extend_batch(
                        a.ptr, b.ptr, M, m, d["fact"].ptr, d["ifact"].ptr, Z.ptr + 32 * n_in, N, K))
                    row["extension_single_ms"], _ = timed(lambda: [ctx.cs_extend(
                        a.ptr + 32 * p * M, b.ptr + 32 * p * M, m, d["fact"].ptr, d["ifact"].ptr, zs[p].ptr + 32 * n_in)
                        for p in range(K)])
                    Z = cs._witnesses_on_device(sc, rows, n_in, draws)      # a, b above held no r_a, r_b
                    zs = [Z[p * N:(p + 1) * N] for p in range(K)]
                    h = vm.pivot._as_point(gens["h"])
                    row["commitments_batch_ms"], _ = timed(lambda: [pc.result() for pc in [
                        vm.pivot._commit_launch(z, dr[2], g, h, ctx) for z, dr in zip(zs, draws)]])
                    row["commitments_single_ms"], _ = timed(lambda: [
                        vm.pivot.vector_commitment(z, dr[2], g, gens["h"]) for z, dr in zip(zs, draws)])
                    c = 2 * m + 12345

                    def forms_batch():
                        Y = vm.ScalarVector.empty(5 * K, ctx)
                        keep = []
                        for p, z in enumerate(zs):
                            fm = cs._Forms(sc, n_in, c + p, order, Y.ptr + 32 * (5 * p + 3))
                            for i, V in enumerate((fm.F, fm.G, fm.H)):
                                ctx.fr_dot_into(V.ptr, z.ptr, N, Y.ptr + 32 * (5 * p + i))
                            keep.append(fm)
                        return Y.to_ints()

                    row["forms_batch_ms"], _ = timed(forms_batch)
                    row["forms_single_ms"], _ = timed(lambda: [cs._Forms(sc, n_in, c + p, order).values(z)
                                                               for p, z in enumerate(zs)])
                    # ---- whole calls
                    row["p8_batch_ms"], p8 = timed(lambda: cs.protocol_8_excl_pivot_prover_batch(gens, sc, xs, gf))
                    row["p8_batch_array_ms"], _ = timed(lambda: cs.protocol_8_excl_pivot_prover_batch(gens, sc, rows, gf))
                    row["p8_single_ms"], _ = timed(lambda: [cs.protocol_8_excl_pivot_prover(gens, sc, x, gf) for x in xs])
                    ys = [L(z) for _, _, L, z, _ in p8]
                    row["pivots_ms"], _ = timed(lambda: [vm.compressed_pivot.protocol_5_prover(
                        gens, zc, L, y, z, gm, gf, transcript="compact", r=vm.compressed_pivot.masks(N, ctx), rho=12345)
                        for (_, zc, L, z, gm), y in zip(p8, ys)])
                    row["prove_batch_ms"], proofs = timed(lambda: cs.circuit_sat_prover_batch(gens, sc, xs, gf))
                    row["prove_single_ms"], _ = timed(lambda: [cs.circuit_sat_prover(gens, sc, x, gf) for x in xs])
                    verdicts = cs.circuit_sat_verifier_batch(proofs, gens, sc, gf)
                    row["verified"] = all(len(v) == 3 and all(v.values()) for v in verdicts)
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                    del Z, zs, p8, proofs, a, b
                del g, gens
                ctx.trim()


if __name__ == "__main__":
    main()
