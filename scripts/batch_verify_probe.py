#!/usr/bin/env python3
"""Developer probe: K compact Protocol-5 proofs over one CRS through protocol_5_verifier_batch (one N-term MSM for all of
them, csrc/batch_verify.hip) against the loop over the unchanged protocol_5_verifier, by shape.

For each N = 2^k asked for (default 16 20) and each K (default 1 4 16 64), in ONE process and after warm-up of both paths:
K proofs of one witness under K DISTINCT linear forms, then RUNS timed regions per path, the two paths alternating region
by region; a region is one call of the path (the batch: all K proofs; the loop: K single verifications) ended by the
verdicts themselves.  The figure is the median per PROOF.  At K = 16 one more row has a single bad proof (its t changed)
among the 16: the batch then bisects.  The per-stage figures are vmpc_stage_scope's (HIP events, profiling on, a run of
their own on the main context): bv_tables / bv_u / bv_dots are the batch kernels, the rest the commitment.  One line per
measurement; `--out FILE` appends them as JSON lines."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import verifiable_mpc_amd as vm                                       # noqa: E402

WARM, RUNS = 2, 7
cp = vm.compressed_pivot


def rand_scalars(rng, n):
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x0F                                                # below 2^252 < l: canonical
    return raw


def regions(fns):
    """{name: [ms per call]} - RUNS regions each, alternating between the functions"""
    out = {name: [] for name in fns}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    for _ in range(RUNS):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            out[name].append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", nargs="+", type=int, default=[16, 20])
    ap.add_argument("--K", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    rng = np.random.default_rng(1717)
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    lines = []

    def report(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for k in args.log2n:
        N = 1 << k
        n = N - 1
        g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(rand_scalars(rng, n)), keep_proj=False)
        gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 0x1234567)}
        g.precompute([gens["h"], gens["k"]])                          # CRS setup
        cp.generators_digest(gens)
        x = vm.ScalarVector.from_array(rand_scalars(rng, n))
        gamma = 0x7654321
        P = vm.pivot.vector_commitment(x, gamma, g, gens["h"])
        statements = []
        for _ in range(max(args.K)):
            L = vm.pivot.LinearForm(vm.ScalarVector.from_array(rand_scalars(rng, n)))
            y = gf(L(x))
            proof = cp.protocol_5_prover(gens, P, L, y, x, gamma, gf, transcript="compact", r=cp.masks(n, ctx), rho=0x1111)
            statements.append((P, L, y, proof))
        ctx.sync()

        def measure(st, what, want):
            K = len(st)

            def batch():
                assert cp.protocol_5_verifier_batch(gens, st, gf, transcript="compact") == want

            def loop():
                assert [cp.protocol_5_verifier(gens, *s, gf, transcript="compact") for s in st] == want
            ts = regions({"batch": batch, "loop": loop})
            b, l = statistics.median(ts["batch"]), statistics.median(ts["loop"])
            ctx.profile(True)
            ctx.profile_read(reset=True)
            batch()
            ctx.sync()
            stages = {name: round(ms, 4) for name, (ms, cnt) in ctx.profile_read(reset=True).items() if cnt}
            ctx.profile(False)
            report(N=N, K=K, what=what, batch_ms_per_proof=round(b / K, 4), loop_ms_per_proof=round(l / K, 4),
                   batch_ms=round(b, 4), loop_ms=round(l, 4), loop_over_batch=round(l / b, 3),
                   batch_min_ms=round(min(ts["batch"]), 4), loop_min_ms=round(min(ts["loop"]), 4),
                   batch_stage_ms=stages)

        for K in args.K:
            measure(statements[:K], "all valid", [True] * K)
            if K == 16:
                Pb, Lb, yb, pb = statements[5]
                bad = statements[:5] + [(Pb, Lb, yb, dict(pb, t=pb["t"] + 1))] + statements[6:16]
                measure(bad, "one bad proof among 16", [i != 5 for i in range(16)])
        del statements, g, gens
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
