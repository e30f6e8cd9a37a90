#!/usr/bin/env python3
"""Developer probe: K Pinocchio proofs from secret-shared witnesses in one trinocchio.prove_batch,
beside one trinocchio.prove, over h_probe.py's synthetic SATISFIABLE R1CS and a synthetic prepared key, and the
recombination kernel alone.

M = 3, t = 1, the three parties as coroutines in ONE process on one GPU over one LocalHub and one context, as
scripts/trinocchio_probe.py runs them (their stages run one after the other; `wall` is the three parties together).
For each d = 2^k asked for (default 10 14), after one warm-up run, the median of three runs (min and max kept) of
  batch        for K in --batch (default 1 16 64): per stage the MEAN over parties (each stage ended by a stream
               synchronisation), the wall time, and the wall time per proof.  The K witnesses are one witness dealt K
               times with different polynomials.
  single       one trinocchio.prove with its stages, `recombine` among them (the eight general-path MSMs before)
  yardstick    with --parent FILE, the jsonl that scripts/trinocchio_probe.py wrote AT THE PARENT COMMIT: its wall time
               of one prove is the cost of each of K single calls; every batch line then carries the ratio
               (batch wall per proof) / (parent wall per proof), printed as it is, above 1 included.
  kernel       vmpc_bn256_recombine_dev alone: n in {8, 512} elements, M in {3, 5}, both groups, with the Lagrange
               weights of 1..M (signed, a few bits) and with full-size weights (a 256-bit chain per party); microseconds
               per launch, the mean over 20 launches queued between two synchronisations.
Timing only - correctness is tests/test_gpu_trinocchio_batch.py and tests/test_gpu_bn256_recombine.py.  One JSON line per
measurement; `--out FILE` appends them."""
import argparse
import asyncio
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verifiable_mpc_amd as vm                                       # noqa: E402
from verifiable_mpc_amd import pynocchio as pn                        # noqa: E402
from verifiable_mpc_amd import trinocchio as tn                       # noqa: E402
from oracle import bn256_ref as bn                                    # noqa: E402
from h_probe import circuit                                           # noqa: E402

STAGES = ("residual", "h_share", "masks", "proof_share", "exchange", "recombine")
M, T = 3, 1


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med3(vals):
    return dict(median=round(statistics.median(vals), 3), min=round(min(vals), 3), max=round(max(vals), 3))


def parent_walls(path):
    """d -> wall_ms of one 3-party prove, from the `derived` lines of the parent's probe"""
    walls = {}
    if path:
        with open(path) as f:
            for line in f:
                rec = json.loads(line)
                if rec.get("what") == "derived":
                    walls[rec["d"]] = rec["wall_ms"]
    return walls


def kernel_alone(ctx, report):
    for group, E, G, enc, width in ((1, bn.E1, bn.G1, bn.g1_to_bytes, 64), (2, bn.E2, bn.G2, bn.g2_to_bytes, 128)):
        for parties in (3, 5):
            rng = random.Random(parties)
            rows = [np.frombuffer(enc(E.mul(p + 2, G)), np.uint8) for p in range(parties)]
            sets = {"lagrange": tn.recombination_vector(list(range(1, parties + 1))),
                    "full": [rng.randrange(pn.ORDER >> 1, pn.ORDER) for _ in range(parties)]}
            for n in (8, 512):
                table = ctx.upload(np.stack([np.tile(r, (n, 1)) for r in rows]))
                out = ctx.alloc(width * n)
                for name, wts in sets.items():
                    ctx.bn256_recombine(group, table.ptr, parties, n, n, wts, out.ptr)
                    ctx.sync()
                    us = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        for _ in range(20):
                            ctx.bn256_recombine(group, table.ptr, parties, n, n, wts, out.ptr)
                        ctx.sync()
                        us.append((time.perf_counter() - t0) * 1e6 / 20)
                    report(what="kernel", group=group, parties=parties, n=n, weights=name, us_per_launch=med3(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, nargs="+", default=[10, 14])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--parent", help="jsonl of scripts/trinocchio_probe.py at the parent commit")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    lines = []
    walls = parent_walls(args.parent)

    def report(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for k in args.log_d:
        d = 1 << k
        V, W, Y, out_ix, m, c = circuit(d, seed=k)
        qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
        key = pn.PreparedKey.synthetic(ctx, m + 1)
        c_ints = [int.from_bytes(row.tobytes(), "little") for row in c]

        def parties(seed, shares, K):
            hub = tn.LocalHub(M)
            rts = [tn.Runtime(p, M, T, random.Random(100 * seed + p), hub) for p in range(M)]
            for rt in rts:
                rt.stage_log = []

            async def run():
                if K is None:
                    return await asyncio.gather(*(tn.prove(rts[p], qap, key, shares[p]) for p in range(M)))
                return await asyncio.gather(*(tn.prove_batch(rts[p], qap, key, shares[p]) for p in range(M)))
            wall = timed_ms(lambda: asyncio.run(run()))
            per = {s: sum(sec for rt in rts for name, sec in rt.stage_log if name == s) * 1e3 / M for s in STAGES}
            return per, wall

        def measure(shares, K):
            parties(0, shares, K)                                     # warm-up: plans, t, tables, allocations
            runs = [parties(1 + i, shares, K) for i in range(3)]
            return {s: med3([r[0][s] for r in runs]) for s in STAGES}, med3([r[1] for r in runs])

        rng = random.Random(k)
        stages, wall = measure(tn.deal_witness(c_ints, T, M, rng), None)
        report(d=d, what="single", parties=M, stages_ms_per_party=stages, wall_ms=wall,
               parent_wall_ms=walls.get(d))
        for K in args.batch:
            dealt = [tn.deal_witness(c_ints, T, M, rng) for _ in range(K)]
            shares = [np.stack([dealt[w][p] for w in range(K)]) for p in range(M)]
            stages, wall = measure(shares, K)
            rec = dict(d=d, what="batch", K=K, parties=M, stages_ms_per_party=stages, wall_ms=wall,
                       wall_ms_per_proof=round(wall["median"] / K, 3))
            if d in walls:
                rec.update(parent_wall_ms_per_proof=walls[d], ratio=round(wall["median"] / K / walls[d], 3))
            report(**rec)
        del key
    if not args.no_kernel:
        kernel_alone(ctx, report)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
