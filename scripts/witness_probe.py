"""The R1CS solve (csrc/bn256_r1cs_solve.hip) under its three schedules, against the host loop a
user ran before it -> profiles/witness_probe.jsonl.

    python scripts/witness_probe.py [--log-d 10,14] [--batch 1,16,64,256] [--reps 3] [--append]

Workloads, each at d = 2^log_d constraints:
    power    y = x^k + x + 5 as the reference's flattener lays it out: a chain of products of depth d (one row per level)
    chain    tests/pinocchio_batch_ref.chain_r1cs: random sparse products, a few dozen levels of 1 to a few hundred rows
    layers   d / 8 rows in each of 8 levels: the levels that the default rule has to decide about
Per workload and K (the witnesses of one call), the median over `reps` runs after one warm-up run, each run bracketed by
stream synchronisations, of the solve on a device-resident batch (inputs in place; solving again changes nothing)
    default_ms   wide_rows = 0, the library's rule          (launches: default_launches)
    level_ms     wide_rows = 1, one launch per level        (Protocol 8's way, by the same build)
    fused_ms     wide_rows = SIZE_MAX, one launch
with each column's lowest and highest run (`*_range_ms`: the probe's own spread), of calculate_witness_batch end to end
(upload, solve, status words, download: e2e_ms), and of the host loop: Python ints, one product per constraint and
witness, timed on min(K, host_witnesses) witnesses and scaled to K (host_loop_ms; host_loop_timed says on how many).
Every schedule's witnesses are compared byte for byte, and witness 0 with the host loop's, before a line is written."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def power_r1cs(d):
    """x = wire 1, out = wire 2; rows 0 .. d-3: t_(j+1) = t_j * x (t_0 = x); row d-2: u = (t + x) * 1; row d-1:
    out = (u + 5) * 1 -> (V, W, Y as CSR with int values, out_ix, m, n_in)"""
    assert d >= 3
    t = lambda j: 1 if j == 0 else 2 + j              # t_1 .. t_(d-2) on wires 3 .. d, u on wire d + 1
    V = [[(t(j), 1)] for j in range(d - 2)] + [[(t(d - 2), 1), (1, 1)], [(d + 1, 1), (0, 5)]]
    W = [[(1, 1)] for _ in range(d - 2)] + [[(0, 1)], [(0, 1)]]
    Y = [[(t(j + 1), 1)] for j in range(d - 2)] + [[(d + 1, 1)], [(2, 1)]]
    return V, W, Y, 2, d + 1, 1


def layers_r1cs(d, levels=8):
    """`levels` levels of d / levels rows: row i of a level multiplies wires i and i + 1 (cyclic) of the level before"""
    w = d // levels
    n_in = w
    V, W, Y = [], [], []
    for lv in range(levels):
        prev, cur = 1 + lv * w, 1 + (lv + 1) * w
        for i in range(w):
            V.append([(prev + i, 1), (0, 3)])
            W.append([(prev + (i + 1) % w, 1)])
            Y.append([(cur + i, 1)])
    return V, W, Y, n_in, (levels + 1) * w, n_in


def chain_rows(d):
    from tests import pinocchio_batch_ref as B
    V, W, Y, n_io, m = B.chain_r1cs(d, seed=2100 + d)
    rows = lambda M: [[(M[1][e], M[2][e]) for e in range(M[0][j], M[0][j + 1])] for j in range(d)]
    return rows(V), rows(W), rows(Y), n_io, m, n_io


def csr(M):
    ptr, col, vals = [0], [], []
    for row in M:
        for wire, x in row:
            col.append(wire)
            vals.append(x)
        ptr.append(len(col))
    return np.asarray(ptr, np.int64), np.asarray(col, np.int64), vals


def host_loop(order, plan_rows, m, inputs, n):
    """what a user ran before: walk the constraints in solve order, Python ints (rows that define a wire of Y with
    coefficient 1 - all three workloads)"""
    c = [0] * (m + 1)
    c[0] = 1
    c[1:1 + len(inputs)] = inputs
    for V, W, s in plan_rows:
        a = sum(x * c[k] for k, x in V) % n
        b = sum(x * c[k] for k, x in W) % n
        c[s] = a * b % n
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", default="10,14")
    ap.add_argument("--batch", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-witnesses", type=int, default=4)
    ap.add_argument("--workloads", default="power,chain,layers")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default="profiles/witness_probe.jsonl")
    args = ap.parse_args()

    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import _native as nat
    from verifiable_mpc_amd import pynocchio as pn
    ctx = vm.get_context()
    n = pn.ORDER
    make = {"power": power_r1cs, "chain": chain_rows, "layers": layers_r1cs}
    batches = [int(s) for s in args.batch.split(",")]

    def timed(fn):
        runs = []
        for i in range(args.reps + 1):          # the first run warms up
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            if i:
                runs.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(runs), [min(runs), max(runs)]

    lines = []
    for log_d in [int(s) for s in args.log_d.split(",")]:
        d = 1 << log_d
        for name in args.workloads.split(","):
            V, W, Y, out_ix, m, n_in = make[name](d)
            qap = pn.R1CSQAP(csr(V), csr(W), csr(Y), out_ix, m=m)
            t0 = time.perf_counter()
            plan = pn.SolvePlan(qap, n_in)
            plan_ms = 1e3 * (time.perf_counter() - t0)
            ptrs, _ = plan.device(ctx)
            assert set(plan.kind.tolist()) == {pn.KIND_Y} and all(len(Y[j]) == 1 and Y[j][0][1] == 1 for j in range(d))
            plan_rows = [(V[j], W[j], Y[j][0][0]) for j in plan.row.tolist()]
            widths = (plan.level_ptr[1:] - plan.level_ptr[:-1]).tolist()
            rng = np.random.default_rng(d + len(name))
            for K in batches:
                inputs = rng.integers(0, 256, size=(K, n_in, 32), dtype=np.uint8)
                inputs[:, :, 31] &= 0x7F
                host = np.zeros((K, m + 1, 32), np.uint8)
                host[:, 1:n_in + 1] = inputs
                dc, bad = ctx.upload(host), ctx.alloc(4 * K)
                rec = {"workload": name, "d": d, "K": K, "levels": plan.n_levels, "widest_level": max(widths),
                       "plan_ms": round(plan_ms, 3), "reps": args.reps}
                results = {}
                for col, wide in (("default", 0), ("level", 1), ("fused", nat.R1CS_WIDE_ALL)):
                    solve = lambda: ctx.bn256_r1cs_solve_batch(ptrs, plan.level_ptr, n_in, m, dc.ptr, m + 1, K, wide,
                                                               bad.ptr)
                    med, span = timed(solve)
                    rec[col + "_ms"], rec[col + "_range_ms"] = round(med, 4), [round(x, 4) for x in span]
                    rec[col + "_launches"] = nat.bn256_r1cs_solve_launches(plan.level_ptr, K, wide)
                    assert (ctx.download(bad.ptr, 4 * K).view("<u4") == 0xFFFFFFFF).all()
                    results[col] = ctx.download(dc.ptr, host.nbytes)
                rec["equal"] = bool(np.array_equal(results["default"], results["level"]) and
                                    np.array_equal(results["default"], results["fused"]))
                rec["fused_us_per_level"] = round(1e3 * rec["fused_ms"] / plan.n_levels, 4)
                rec["level_us_per_level"] = round(1e3 * rec["level_ms"] / plan.n_levels, 4)
                rec["e2e_ms"] = round(timed(lambda: pn.calculate_witness_batch(qap, inputs, ctx=ctx))[0], 3)
                n_host = min(K, args.host_witnesses)
                ints = [[int.from_bytes(inputs[w, i].tobytes(), "little") for i in range(n_in)] for w in range(n_host)]
                t0 = time.perf_counter()
                cs = [host_loop(None, plan_rows, m, ints[w], n) for w in range(n_host)]
                rec["host_loop_timed"] = n_host
                rec["host_loop_ms"] = round(1e3 * (time.perf_counter() - t0) / n_host * K, 3)
                got0 = results["default"][:32 * (m + 1)].tobytes()
                rec["equal"] = rec["equal"] and got0 == b"".join(x.to_bytes(32, "little") for x in cs[0])
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del dc, bad
    out = os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a" if args.append else "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
