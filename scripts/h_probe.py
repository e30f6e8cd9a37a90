#!/usr/bin/env python3
"""Developer probe: the Pinocchio prover's h on the GPU (verifiable_mpc_amd/pynocchio.py compute_h,
csrc/bn256_qap_h.hip) by size, over a synthetic SATISFIABLE R1CS (V and W rows read two input wires, Y writes one output
wire).

For each d = 2^k asked for (default 10 12 14 16 18), medians of timed runs after warm-up runs, every run ended by a
device synchronisation, all in ONE process:
  t_coeffs      vmpc_bn256_qap_t_coeffs_dev - one run, it is made once per (context, QAP)
  row_values    a = V c, b = W c, y = Y c (vmpc_bn256_qap_colsum_dev over the row-ordered plan)
  check         vmpc_bn256_qap_check_dev
  weights       vmpc_bn256_qap_h_weights_dev (both vectors)
  moments       vmpc_bn256_qap_moments_dev, both vectors, n_out = d
  product       vmpc_bn256_fr_poly_mul_dev at d x d - the yardstick, the entry as it stands
  combine       vmpc_bn256_qap_h_combine_dev (the halves it reads of two such products and two elementwise kernels)
  compute_h     the whole call, witness upload, check and its host read-back included
  compute_proof over a synthetic prepared key, h read from the device
and derived: non_product = compute_h - 2 product (what the acceptance ratio of DESIGN.md section 14 compares with one
product) and h_share = compute_h / (compute_h + compute_proof).
Timing only - correctness is tests/test_gpu_pinocchio_h.py.  One JSON line per measurement; `--out FILE` appends them."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import verifiable_mpc_amd as vm                                       # noqa: E402
from verifiable_mpc_amd import pynocchio as pn                        # noqa: E402

N = pn.ORDER


def median_ms(fn, runs, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def to_array(ints):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), np.uint8).reshape(-1, 32)


def circuit(d, seed, n_io=4):
    """-> (V, W, Y as CSR tuples, out_ix, m, witness (m + 1, 32) uint8) with the witness satisfying every row"""
    rng = np.random.default_rng(seed)
    m = n_io + 2 * d
    c = [1] + [int(x) ** 3 % N for x in rng.integers(1, 1 << 62, size=n_io + d)]
    ptr = np.arange(0, 2 * d + 1, 2)
    mats, rows = [], []
    for _ in range(2):
        col = rng.integers(0, n_io + d + 1, size=2 * d)
        vals = rng.integers(-(1 << 62), 1 << 62, size=2 * d).astype(np.int64)
        mats.append((ptr, col, vals))
        cl, vl = col.tolist(), vals.tolist()
        rows.append([(vl[2 * r] * c[cl[2 * r]] + vl[2 * r + 1] * c[cl[2 * r + 1]]) % N for r in range(d)])
    Y = (np.arange(d + 1), n_io + d + 1 + np.arange(d), np.ones(d, np.int64))
    c += [a * b % N for a, b in zip(*rows)]
    return mats[0], mats[1], Y, n_io, m, to_array(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, nargs="+", default=[10, 12, 14, 16, 18])
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    lines = []

    def report(d, what, med, lo, hi, **extra):
        rec = dict(d=d, what=what, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), **extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def run(fn):
        def timed():
            fn()
            ctx.sync()
        return timed

    for k in args.log_d:
        d = 1 << k
        runs, warm = (3, 1) if k >= 18 else (7, 2)
        V, W, Y, out_ix, m, c = circuit(d, seed=k)
        qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
        deltas = types.SimpleNamespace(v=3 ** 100 % N, w=5 ** 100 % N, y=7 ** 100 % N)
        scratch_t, t = ctx.alloc(64 * (d + (d + 127) // 128)), ctx.alloc(32 * (d + 1))
        ctx.sync()
        t0 = time.perf_counter()
        ctx.bn256_qap_t_coeffs(d, scratch_t.ptr, t.ptr)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        report(d, "t_coeffs", ms, ms, ms)
        dc = ctx.upload(c)
        plan = pn._row_plan(ctx, qap)
        aby = ctx.alloc(32 * 3 * d)
        a, b, y = aby.ptr, aby.ptr + 32 * d, aby.ptr + 64 * d
        report(d, "row_values", *median_ms(run(lambda: plan.run(dc.ptr, m + 1, aby.ptr)), runs, warm))
        bad = ctx.alloc(4)
        report(d, "check", *median_ms(run(lambda: ctx.bn256_qap_check(a, b, y, d, bad.ptr)), runs, warm))
        u, mom = ctx.alloc(64 * d), ctx.alloc(64 * d)
        report(d, "weights", *median_ms(run(lambda: ctx.bn256_qap_h_weights(a, b, d, u.ptr, u.ptr + 32 * d)), runs, warm))
        mo = median_ms(run(lambda: ctx.bn256_qap_moments(u.ptr, u.ptr + 32 * d, d, d, mom.ptr, mom.ptr + 32 * d)),
                       runs, warm)
        report(d, "moments", *mo, steps_per_ns=round(2 * d * d / (mo[0] * 1e6), 3))
        prod_out = ctx.alloc(32 * (2 * d - 1))
        pr = median_ms(run(lambda: ctx.bn256_fr_poly_mul(mom.ptr, d, mom.ptr + 32 * d, d, prod_out.ptr)), runs, warm)
        report(d, "product", *pr, steps_per_ns=round(d * d / (pr[0] * 1e6), 3))
        scratch, out = ctx.alloc(32 * 5 * d), ctx.alloc(32 * (d + 1))
        dd = pn._scalar_buf(ctx, [deltas.v, deltas.w, deltas.y])
        report(d, "combine", *median_ms(run(lambda: ctx.bn256_qap_h_combine(mom.ptr, mom.ptr + 32 * d, t.ptr, d, dd.ptr,
                                                                           scratch.ptr, out.ptr)), runs, warm))
        pn.compute_h(qap, c, deltas)          # (makes and caches the plan and t)
        ch = median_ms(lambda: pn.compute_h(qap, c, deltas), runs, warm)
        report(d, "compute_h", *ch)
        key = pn.PreparedKey.synthetic(ctx, m + 1)
        h = pn.compute_h(qap, c, deltas)
        cp = median_ms(lambda: pn.compute_proof(qap, c, h, key, deltas), runs, warm)
        report(d, "compute_proof", *cp)
        non_product = ch[0] - 2 * pr[0]
        rec = dict(d=d, what="derived", non_product_ms=round(non_product, 3), product_ms=round(pr[0], 3),
                   non_product_over_product=round(non_product / pr[0], 3),
                   h_share_of_proof=round(ch[0] / (ch[0] + cp[0]), 3))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        del key
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
