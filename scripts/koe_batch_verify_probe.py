"""Batch verification of knowledge-of-exponent proofs against the loop of single calls
-> profiles/koe_batch_verify_probe.jsonl.

    python scripts/koe_batch_verify_probe.py [--parts rows,opening,circuit] [--reps 7] [--warmup 2] [--out FILE]

Medians of `reps` runs after `warmup` runs, each bracketed by a stream synchronisation, of
    rows      PPVector.msm_rows (vmpc_bn256_table_msm_rows_dev) against a loop of vmpc_bn256_table_msm_dev over the same
              rows, G2 and G1, m = 2^10, 2^13, 2^16 terms, rows = 1, 16, 64, 256; with the stage split of one profiled
              run of each (sort = recoding, histogram, partition, fine sort, plan)
    opening   opening_linear_form_verifier_batch against the loop of opening_linear_form_verifier, n = 2^10, 2^14,
              K = 1, 16, 64, 256 honest proofs of one pp (device forms)
    circuit   circuit_sat_verifier_batch against the loop of circuit_sat_verifier on the product chain, m = 2^10, K = 64
Inputs are random (timing only; correctness is tests/test_gpu_bn256_msm_rows.py and tests/test_gpu_koe_batch_verify.py)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SORT_STAGES = ("msm_recode", "msm_hist", "msm_part", "msm_sort", "msm_plan")


def chain(m):
    return 1, (list(range(m + 1)), [0] + list(range(1, m)), np.ones(m, np.int64)), \
        (list(range(m + 1)), [0] * m, np.ones(m, np.int64)), ([0, 1], [m], np.ones(1, np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="rows,opening,circuit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/koe_batch_verify_probe.jsonl")
    args = ap.parse_args()
    parts = args.parts.split(",")
    import verifiable_mpc_amd as vm
    from oracle import bn256_ref as bn
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    from verifiable_mpc_amd import knowledge_of_exponent as koe
    from verifiable_mpc_amd.device import BnScalarVector
    ctx = vm.get_context()
    P = vm.pynocchio
    order = P.ORDER
    g1, g2 = P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2)
    rng = np.random.default_rng(31)
    koe.prng = random.Random(31)

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

    def stage_split(fn):
        ctx.profile(True)
        ctx.profile_read(reset=True)
        fn()
        ctx.sync()
        st = ctx.profile_read(reset=True)
        ctx.profile(False)
        ms = lambda names: round(sum(st[k][0] for k in names if k in st), 4)       # noqa: E731
        return {"sort_ms": ms(SORT_STAGES), "bucket_ms": ms(["bn_bucket"]), "reduce_ms": ms(["bn_reduce"]),
                "final_ms": ms(["bn_final"])}

    def scalars(count):
        a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
        a[:, 31] &= 0x7F
        return a

    with open(args.out, "w") as f:        # a run replaces the file
        def emit(row):
            row.update(reps=args.reps, warmup=args.warmup)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if "rows" in parts:
            for k in (10, 13, 16):
                m = 1 << k
                pp = koe.trusted_setup(g1, g2, m // 2, order)          # m points a side
                for name, group in (("pp_rhs", 2), ("pp_lhs", 1)):
                    side = pp[name]
                    for rows in (1, 16, 64, 256):
                        mat = ctx.upload(scalars(rows * m))
                        side.msm_rows(mat, m, 1)                       # (builds the table)
                        out = ctx.alloc(side.width * rows)

                        def batch():
                            ctx.bn256_table_msm_rows(group, side._table.ptr, m, mat.ptr, m, m, rows, out.ptr)

                        def loop():
                            for r in range(rows):
                                ctx.bn256_table_msm(group, side._table.ptr, m, mat.ptr + 32 * m * r, m,
                                                    out.ptr + side.width * r, None)
                        row = {"what": "msm_rows", "group": group, "m": m, "rows": rows}
                        row["rows_ms"], row["rows_spread_ms"], _ = timed(batch)
                        row["loop_ms"], row["loop_spread_ms"], _ = timed(loop)
                        row["loop_over_rows"] = round(row["loop_ms"] / row["rows_ms"], 3)
                        row["rows_stages"], row["loop_stages"] = stage_split(batch), stage_split(loop)
                        emit(row)
                        del mat, out
                del pp, side
                ctx.trim()

        if "opening" in parts:
            for k in (10, 14):
                n = 1 << k
                pp = koe.trusted_setup(g1, g2, n, order)
                x = BnScalarVector.from_array(scalars(n), ctx)
                made = []
                for _ in range(4):         # four distinct openings, repeated to K proofs: the verifier's work is the same
                    L = vm.pivot.LinearForm(BnScalarVector.from_array(scalars(n), ctx))
                    proof, u = koe.opening_linear_form_prover(L, x, 12345, pp)
                    made.append((L, proof, int(u)))
                for K in (1, 16, 64, 256):
                    items = [made[i % 4] for i in range(K)]
                    Ls, proofs, us = [a for a, _, _ in items], [b for _, b, _ in items], [c for _, _, c in items]
                    row = {"what": "opening_linear_form_verifier_batch", "n": n, "K": K}
                    row["batch_ms"], row["batch_spread_ms"], got = timed(
                        lambda: koe.opening_linear_form_verifier_batch(Ls, pp, proofs, us))
                    row["loop_ms"], row["loop_spread_ms"], want = timed(
                        lambda: [koe.opening_linear_form_verifier(L, pp, p, u) for L, p, u in items])
                    row["loop_over_batch"] = round(row["loop_ms"] / row["batch_ms"], 3)
                    row["same_answers"] = got == want and all(all(v.values()) for v in got)
                    emit(row)
                del pp, made, x
                ctx.trim()

        if "circuit" in parts:
            m, K = 1 << 10, 64
            n_x, A, B, O = chain(m)
            N = 1 + 3 + 2 * m
            pp = koe.trusted_setup(g1, g2, N, order)
            sc = cs.SparseCircuit(n_x, A, B, O, order=order)
            gf_n = vm.GF(order)
            proofs = [cs.circuit_sat_prover(pp, sc, [3 + i], gf_n, "koe") for i in range(K)]
            row = {"what": "circuit_sat_verifier_batch", "m": m, "N": N, "K": K}
            row["batch_ms"], row["batch_spread_ms"], got = timed(lambda: cs.circuit_sat_verifier_batch(proofs, pp, sc, gf_n))
            row["loop_ms"], row["loop_spread_ms"], want = timed(
                lambda: [cs.circuit_sat_verifier(p, pp, sc, gf_n, "koe") for p in proofs])
            row["loop_over_batch"] = round(row["loop_ms"] / row["batch_ms"], 3)
            row["same_answers"] = got == want and all(v["pivot_verification"] == {"restriction_arg_check": True,
                                                                                 "PRQ_check": True} for v in got)
            emit(row)


if __name__ == "__main__":
    main()
