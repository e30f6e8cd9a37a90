#!/usr/bin/env python3
"""Developer probe: the M-party Pinocchio prover over a secret-shared witness (verifiable_mpc_amd/trinocchio.py) by
size, beside the single prover, over h_probe.py's synthetic SATISFIABLE R1CS and a synthetic prepared key.

M = 3, t = 1, the three parties as coroutines in ONE process on one GPU (so their stages run one after the other and
"total" is the sum over the parties).  For each d = 2^k asked for (default 10 14), after one warm-up run, the median of
three runs of
  residual      vmpc_bn256_qap_residual_dev and the masking of its result
  h_share       witness upload, row values, then compute_h_share's weights -> moments -> combination
  masks         dealing deltas, rho and the sharings of zero (host draws, vmpc_bn256_fr_share_mul_deal_dev, download),
                adding what arrived, and the masking combination of h
  proof_share   compute_proof on the shares
  exchange      the local work after an exchange: the recombinations of opened scalars and of the eight proof points
per party (each stage ended by a stream synchronisation; the median over runs of the MEAN over parties), and in the
same run the single prover's compute_h and compute_proof at the same d.  Derived:
  parties_over_single   (sum over the M parties of all stages) / (M x (compute_h + compute_proof))
  h_share_over_h        (h_share stage) / compute_h - both include the witness upload and the row values
Timing only - correctness is tests/test_gpu_trinocchio.py.  One JSON line per measurement; `--out FILE` appends them."""
import argparse
import asyncio
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verifiable_mpc_amd as vm                                       # noqa: E402
from verifiable_mpc_amd import pynocchio as pn                        # noqa: E402
from verifiable_mpc_amd import trinocchio as tn                       # noqa: E402
from h_probe import circuit                                           # noqa: E402

STAGES = ("residual", "h_share", "masks", "proof_share", "exchange")
M, T = 3, 1


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, nargs="+", default=[10, 14])
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    lines = []

    def report(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for k in args.log_d:
        d = 1 << k
        V, W, Y, out_ix, m, c = circuit(d, seed=k)
        qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
        key = pn.PreparedKey.synthetic(ctx, m + 1)
        c_ints = [int.from_bytes(row.tobytes(), "little") for row in c]
        shares = tn.deal_witness(c_ints, T, M, random.Random(k))

        def parties(seed):
            hub = tn.LocalHub(M)
            rts = [tn.Runtime(p, M, T, random.Random(100 * seed + p), hub) for p in range(M)]
            for rt in rts:
                rt.stage_log = []

            async def run():
                return await asyncio.gather(*(tn.prove(rts[p], qap, key, shares[p]) for p in range(M)))
            wall = timed_ms(lambda: asyncio.run(run()))
            per = {s: sum(sec for rt in rts for name, sec in rt.stage_log if name == s) * 1e3 for s in STAGES}
            return per, wall

        deltas = pn.SampleDeltas(pn.ORDER)

        def single():
            box = {}
            ms_h = timed_ms(lambda: box.setdefault("h", pn.compute_h(qap, c, deltas)))
            ms_p = timed_ms(lambda: pn.compute_proof(qap, c, box["h"], key, deltas))
            return ms_h, ms_p

        parties(0)
        single()                                                      # warm-up: plans, t, tables, allocations
        runs_p = [parties(1 + i) for i in range(3)]
        runs_s = [single() for _ in range(3)]
        med = {s: statistics.median(r[0][s] for r in runs_p) for s in STAGES}
        spread = {s: (min(r[0][s] for r in runs_p), max(r[0][s] for r in runs_p)) for s in STAGES}
        for s in STAGES:
            report(d=d, what=s, parties=M, median_ms_per_party=round(med[s] / M, 3),
                   min_ms_per_party=round(spread[s][0] / M, 3), max_ms_per_party=round(spread[s][1] / M, 3))
        total = statistics.median(sum(r[0].values()) for r in runs_p)
        wall = statistics.median(r[1] for r in runs_p)
        h_ms = [r[0] for r in runs_s]
        p_ms = [r[1] for r in runs_s]
        report(d=d, what="compute_h", median_ms=round(statistics.median(h_ms), 3), min_ms=round(min(h_ms), 3),
               max_ms=round(max(h_ms), 3))
        report(d=d, what="compute_proof", median_ms=round(statistics.median(p_ms), 3), min_ms=round(min(p_ms), 3),
               max_ms=round(max(p_ms), 3))
        one = statistics.median(h_ms) + statistics.median(p_ms)
        report(d=d, what="derived", parties=M, threshold=T, stages_total_ms=round(total, 3), wall_ms=round(wall, 3),
               single_ms=round(one, 3), parties_over_single=round(total / (M * one), 3),
               h_share_over_h=round(med["h_share"] / M / statistics.median(h_ms), 3),
               h_share_spread=round((spread["h_share"][1] - spread["h_share"][0]) / M / statistics.median(h_ms), 3),
               h_spread=round((max(h_ms) - min(h_ms)) / statistics.median(h_ms), 3))
        del key
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
