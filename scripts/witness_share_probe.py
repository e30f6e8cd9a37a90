"""The R1CS solve on Shamir shares (trinocchio.calculate_witness_shares, csrc/bn256_r1cs_share.hip)
stage by stage, against two yardsticks from code it does not touch -> profiles/witness_share_probe.jsonl.

    python scripts/witness_share_probe.py [--log-d 10,14] [--batch 1,64] [--reps 3] [--workloads power,chain,layers]

M = 3 parties with t = 1 as coroutines of ONE process over one LocalHub and one context; the workloads of
scripts/witness_probe.py at d = 2^log_d constraints, K input vectors per call.  Per workload and K, after one warm-up
run, `reps` runs; every stage of a party ends in a stream synchronisation (Runtime.stage_log).  Per party and stage
(local, coeffs - the draw and upload of the dealt coefficients -, mul_deal, download, exchange, upload, finish) the
run's total is divided by the number of rounds: the median over the runs of that per-round time, with the lowest and
highest run (`party*_us_per_round`: [median, min, max]).  In one process the parties run one after another, so a party's
`exchange` is the time the OTHER parties spend in their own stages before the hub releases it - it is kept as measured
and left out of `own_us_per_round`, party 0's sum of the other stages: what one party's GPU and host do for a round.
`wall_us_per_round`: the whole M-party call, wall clock, per round (all M parties' work, in sequence), with the stage
log on; `unlogged_wall_us_per_round`: the same with the stage log off, i.e. without the extra synchronisations.
The yardsticks, measured in the same run:
    clear_us_per_level     pynocchio.calculate_witness_batch end to end on the same circuit and K, per SolvePlan level
    random_shares_wall_us  one rt.random_shares(1) of the same M parties in the same process, wall clock: an exchange
                           round trip (deal, download, hub, upload, combine) with almost no arithmetic
`own_over_clear_level` = own_us_per_round / clear_us_per_level; `wall_over_random_shares` = wall_us_per_round /
random_shares_wall_us (both are M parties in sequence).  Before a line is written, the parties' outputs are recombined
on the device and compared byte for byte with calculate_witness_batch on the recombined inputs."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STAGES = ("local", "coeffs", "mul_deal", "download", "exchange", "upload", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", default="10,14")
    ap.add_argument("--batch", default="1,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="power,chain,layers")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default="profiles/witness_share_probe.jsonl")
    args = ap.parse_args()

    import witness_probe as WP
    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import pynocchio as pn
    from verifiable_mpc_amd import trinocchio as tn
    ctx = vm.get_context()
    M, t = 3, 1
    make = {"power": WP.power_r1cs, "chain": WP.chain_rows, "layers": WP.layers_r1cs}
    out = os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not args.append:
        open(out, "w").close()

    def spread(runs):
        return [round(statistics.median(runs), 3), round(min(runs), 3), round(max(runs), 3)]

    def parties(seed):
        hub = tn.LocalHub(M)
        return [tn.Runtime(p, M, t, random.Random(seed + p), hub, ctx) for p in range(M)]

    async def gather(calls):
        return await asyncio.gather(*calls)

    # yardstick 2: one dealt random share, exchanged and combined
    rts = parties(1)
    trips = []
    for i in range(4 * args.reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        asyncio.run(gather([rt.random_shares(1) for rt in rts]))
        ctx.sync()
        if i:
            trips.append(1e6 * (time.perf_counter() - t0))
    random_shares_wall_us = spread(trips)

    for log_d in [int(s) for s in args.log_d.split(",")]:
        d = 1 << log_d
        for name in args.workloads.split(","):
            V, W, Y, out_ix, m, n_in = make[name](d)
            qap = pn.R1CSQAP(WP.csr(V), WP.csr(W), WP.csr(Y), out_ix, m=m)
            t0 = time.perf_counter()
            plan = pn.ShareSolvePlan(qap, n_in)
            plan_ms = 1e3 * (time.perf_counter() - t0)
            levels = pn.SolvePlan(qap, n_in).n_levels
            D = plan.n_rounds
            for K in [int(s) for s in args.batch.split(",")]:
                rng = random.Random(d + K)
                line = [(rng.randrange(pn.ORDER), rng.randrange(pn.ORDER)) for _ in range(K * n_in)]   # degree t = 1
                x = [pn.scalars_to_array([(a + b * (p + 1)) % pn.ORDER for a, b in line]).reshape(K, n_in, 32)
                     for p in range(M)]
                rec = {"workload": name, "d": d, "K": K, "parties": M, "t": t, "rounds": D, "levels": levels,
                       "local_levels": plan.n_local_levels, "product_rows": int(plan.round_ptr[-1]),
                       "widest_round": int(np.diff(plan.round_ptr).max()) if D else 0, "plan_ms": round(plan_ms, 3),
                       "reps": args.reps}
                walls, unlogged, per = [], [], {(p, s): [] for p in range(M) for s in STAGES}
                for i in range(2 * args.reps + 1):                   # the first run warms up; then logged, unlogged, ..
                    logged = i % 2 == 1
                    rts = parties(10 * i)
                    for rt in rts:
                        rt.stage_log = [] if logged else None
                    ctx.sync()
                    t0 = time.perf_counter()
                    outs = asyncio.run(gather([tn.calculate_witness_shares(rts[p], qap, x[p], ctx=ctx) for p in range(M)]))
                    ctx.sync()
                    if not i:
                        continue
                    (walls if logged else unlogged).append(1e6 * (time.perf_counter() - t0) / max(D, 1))
                    assert [rt.exchanges for rt in rts] == [D] * M
                    for p, rt in enumerate(rts if logged else []):
                        for s in STAGES:
                            total = sum(sec for stage, sec in rt.stage_log if stage == s)
                            per[p, s].append(1e6 * total / max(D, 1))
                rec["wall_us_per_round"], rec["unlogged_wall_us_per_round"] = spread(walls), spread(unlogged)
                for p in range(M):
                    rec[f"party{p}_us_per_round"] = {s: spread(per[p, s]) for s in STAGES}
                own_us = sum(rec["party0_us_per_round"][s][0] for s in STAGES if s != "exchange")
                rec["own_us_per_round"] = round(own_us, 3)
                # the outputs and the inputs recombined: the clear solve of the one must give the other
                opened = []
                for arrs in (x, outs):
                    n = arrs[0].size // 32
                    parts, res = ctx.upload(np.stack(arrs)), ctx.alloc(32 * n)
                    ctx.bn256_share_combine(parts.ptr, M, n, n, rts[0].weights, None, None, res.ptr)
                    opened.append(ctx.download(res.ptr, 32 * n, arrs[0].shape))
                clear = []
                for i in range(args.reps + 1):
                    ctx.sync()
                    t0 = time.perf_counter()
                    want = pn.calculate_witness_batch(qap, opened[0], ctx=ctx)
                    ctx.sync()
                    if i:
                        clear.append(1e6 * (time.perf_counter() - t0) / levels)
                rec["equal"] = bool(np.array_equal(want, opened[1]))
                rec["clear_us_per_level"] = spread(clear)
                rec["random_shares_wall_us"] = random_shares_wall_us
                rec["own_over_clear_level"] = round(own_us / rec["clear_us_per_level"][0], 2)
                rec["wall_over_random_shares"] = round(rec["wall_us_per_round"][0] / random_shares_wall_us[0], 2)
                print(json.dumps(rec), flush=True)
                with open(out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                assert rec["equal"], "the recombined shares are not the clear witness"


if __name__ == "__main__":
    main()
