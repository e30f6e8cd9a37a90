"""The jointly made pp and the M-party knowledge-of-exponent prover, stage by stage (verifiable_mpc_amd/mpc_koe.py,
mpc_circuit_sat.py, csrc/bn256_scale.hip) -> profiles/mpc_koe_probe.jsonl.

    python scripts/mpc_koe_probe.py [--sizes 10,14,16] [--reps 7] [--warmup 2] [--out profiles/mpc_koe_probe.jsonl]

Per N = 2^k scalars in the committed vector (a pp of 2N points a side): medians of `reps` runs after `warmup` runs, each
bracketed by a stream synchronisation, of
    update_setup   one party's pass, per group: the vmpc_bn256_scale_points_dev launch over 2N points alone
                   (`scale_g1_ms`, `scale_g2_ms`), the mixed additions per second it amounts to - 256 doublings and 256
                   mixed additions a point, counted as 512 - beside vmpc_bn256_madd_rate of the same session, and the
                   whole update_setup call (`update_ms`: powers, both launches, two synchronisations)
    prover         M = 3, t = 1 parties in one process on one GPU (LocalHub) on the inner product of m = N / 4 terms
                   (depth 1; n_x = N / 2 - 3 inputs, N = n_x + 3 + 2m): the stages of mpc_circuit_sat.STAGE_HOOK -
                   triples, extension, schur, commitment, pivot (which holds the opening of the y's and the assembly of
                   L) - and the total, with the single prover's total beside it."""
import argparse
import asyncio
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inner(m, n_x):
    """<x[0:m], x[n_x-m:n_x]> as m gates of depth 1 and one output, in CSR"""
    ptr = list(range(m + 1))
    return n_x, (ptr, list(range(m)), np.ones(m, np.int64)), (ptr, list(range(n_x - m, n_x)), np.ones(m, np.int64)), \
        ([0, m], list(range(n_x, n_x + m)), np.ones(m, np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/mpc_koe_probe.jsonl")
    args = ap.parse_args()
    import verifiable_mpc_amd as vm
    from oracle import bn256_ref as bn
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    from verifiable_mpc_amd import knowledge_of_exponent as koe
    from verifiable_mpc_amd import mpc_ac20, mpc_circuit_sat as mcs, mpc_koe
    ctx = vm.get_context()
    P = vm.pynocchio
    order = P.ORDER
    gf = vm.GF(order)
    g1, g2 = P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2)
    M, t = 3, 1
    loop = asyncio.new_event_loop()

    def timed(fn):
        out, r = [], None
        for i in range(args.warmup + args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            if i >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), r

    def together(rts, fn):
        async def everybody():
            return await asyncio.gather(*[fn(p, rt) for p, rt in enumerate(rts)])
        return loop.run_until_complete(everybody())

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    madd = {1: ctx.bn256_madd_rate(1), 2: ctx.bn256_madd_rate(2)}
    with open(args.out, "w") as f:
        for k in [int(s) for s in args.sizes.split(",")]:
            N = 1 << k
            row = {"N": N, "pp_points_a_side": 2 * N, "reps": args.reps, "parties": M, "threshold": t,
                   "madd_rate_g1": madd[1], "madd_rate_g2": madd[2]}
            pp = koe.trusted_setup(g1, g2, N, order)
            draws = [random.Random(k).randrange(1, order) for _ in range(3)]

            # ---- one party's pass over the pp ---------------------------------------------------------------------
            for group, side in ((1, pp["pp_lhs"]), (2, pp["pp_rhs"])):
                exps = koe.fr_powers(draws[2], draws[0], 2 * N, ctx)
                out = ctx.alloc(side.width * 2 * N)
                ms, _ = timed(lambda: ctx.bn256_scale_points(group, side.buf.ptr, exps.ptr, 2 * N, out.ptr))
                row[f"scale_g{group}_ms"] = ms
                row[f"scale_g{group}_madd_per_s"] = 512 * 2 * N / (ms * 1e-3)
                row[f"scale_g{group}_of_madd_rate"] = row[f"scale_g{group}_madd_per_s"] / madd[group]
            row["update_ms"], _ = timed(lambda: koe.update_setup(pp, *draws))

            # ---- the provers ----------------------------------------------------------------------------------------
            m = N // 4
            n_x = N - 3 - 2 * m
            sc = cs.SparseCircuit(*inner(m, n_x), order=order)
            x = [3 + i for i in range(n_x)]
            row["m"], row["n_x"] = m, n_x
            row["single_total_ms"], proof1 = timed(lambda: cs.circuit_sat_prover(pp, sc, x, gf, "koe"))
            hub = mpc_ac20.LocalHub(M)
            rts = [mpc_koe.Runtime(p, M, t, random.Random(p), hub) for p in range(M)]
            rng = random.Random(5)
            coeff = [rng.randrange(order) for _ in range(n_x)]
            xs = [mpc_koe.SharedVector.from_shares([(v + c * (p + 1)) % order for v, c in zip(x, coeff)], rts[p])
                  for p in range(M)]
            names = ("triples", "extension", "schur", "commitment", "pivot")
            stage = {name: [] for name in names + ("total",)}

            def run_once():
                spans, clock = {}, {}

                # the parties run in step between exchanges and in party order: the last party ends a stage last
                def hook(rt, name):
                    if rt.pid == M - 1:
                        ctx.sync()
                        now = time.perf_counter()
                        spans[name] = (now - clock["t"]) * 1e3
                        clock["t"] = now
                mcs.STAGE_HOOK = hook
                try:
                    ctx.sync()
                    t0 = clock["t"] = time.perf_counter()
                    proofs = together(rts, lambda p, rt: mcs.circuit_sat_prover(pp, sc, xs[p], gf, "koe", rt=rt))
                    ctx.sync()
                    spans["total"] = (time.perf_counter() - t0) * 1e3
                finally:
                    mcs.STAGE_HOOK = None
                return spans, proofs

            for _ in range(args.warmup):
                run_once()
            for _ in range(args.reps):
                spans, proofs = run_once()
                for name in stage:
                    stage[name].append(spans[name])
            med = {name: statistics.median(v) for name, v in stage.items()}
            row["mpc"] = {name + "_ms": v for name, v in med.items()}
            verdict = cs.circuit_sat_verifier(proofs[0], pp, sc, gf, "koe")
            row["verified"] = verdict["y1*y2=y3"] and verdict["L_wellformed_from_Cfgh_forms"] and \
                all(verdict["pivot_verification"].values())
            row["exchanges"] = rts[0].exchanges // (args.warmup + args.reps)
            row["total_over_single"] = med["total"] / row["single_total_ms"]
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            del pp, proofs, proof1, xs, sc
            ctx.trim()


if __name__ == "__main__":
    main()
