#!/usr/bin/env python3
"""Developer probe: the knowledge-of-exponent pivot over BN-256 (verifiable_mpc_amd/knowledge_of_exponent.py) by size.

For each n = 2^k asked for (default 10 12 14 16), medians of timed runs after warm-up runs, every run ended by a device
synchronisation:
  setup     trusted_setup (2n exponents, 2n G1 and 2n G2 fixed-base products) - one run, it is a one-off
  prove     opening_linear_form_prover on a prepared pp (tables built by the warm-up), and its four parts timed on
            their own: the G1 and the G2 restriction MSM, the polynomial product (vmpc_bn256_fr_poly_mul_dev on device
            buffers), the Q MSM over 2n points
  verify    opening_linear_form_verifier (one G2 MSM over n points, five Miller loops, two final exponentiations)
The product kernel's rate is 64 (n+1) n limb multiply-adds over its time; `--mad-rate R` (lane-instructions per second
of v_mad_u64_u32, as scripts/valu_rates.hip prints it in the same session) turns it into a fraction of that rate.
Inputs are random (timing only - correctness is tests/test_gpu_koe.py).  One line per measurement; `--out FILE` appends
them as JSON lines."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import verifiable_mpc_amd as vm                                       # noqa: E402
from oracle import bn256_ref as bn                                    # noqa: E402
from verifiable_mpc_amd import knowledge_of_exponent as koe           # noqa: E402
from verifiable_mpc_amd import pynocchio as pn                        # noqa: E402

WARM, RUNS = 2, 7


def median_ms(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[10, 12, 14, 16])
    ap.add_argument("--mad-rate", type=float, default=0.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    rng = np.random.default_rng(12)
    lines = []

    def report(n, what, med, lo, hi, **extra):
        rec = dict(n=n, what=what, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), **extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def scalars(count):
        a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
        a[:, 31] &= 0x7F
        return a

    for k in args.log_n:
        n = 1 << k
        koe.prng = random.Random(k)
        t0 = time.perf_counter()
        pp = koe.trusted_setup(pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2), n, pn.ORDER)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        report(n, "setup", ms, ms, ms)
        x, coeffs, gamma = scalars(n), scalars(n), 12345
        # the prover takes the reference's lists of scalars
        xs = [int.from_bytes(r.tobytes(), "little") for r in x]
        L = vm.pivot.LinearForm([int.from_bytes(r.tobytes(), "little") for r in coeffs])
        out = {}

        def prove():
            out["proof"], out["u"] = koe.opening_linear_form_prover(L, xs, gamma, pp)
        report(n, "prove", *median_ms(prove))
        sc = np.concatenate([scalars(1), x])
        report(n, "prove: restriction MSM G1 (n+1 points)", *median_ms(lambda: pp["pp_lhs"].msm(sc)))
        report(n, "prove: restriction MSM G2 (n+1 points)", *median_ms(lambda: pp["pp_rhs"].msm(sc)))
        da, db, dc = ctx.upload(sc), ctx.upload(coeffs), ctx.alloc(32 * 2 * n)

        def product():
            ctx.bn256_fr_poly_mul(da.ptr, n + 1, db.ptr, n, dc.ptr)
            ctx.sync()
        med, lo, hi = median_ms(product)
        macs = 64.0 * (n + 1) * n
        extra = {"limb_macs_per_s": round(macs / (med * 1e-3), 0)}
        if args.mad_rate:
            extra["fraction_of_mad_u64_rate"] = round(macs / (med * 1e-3) / args.mad_rate, 4)
        report(n, "prove: polynomial product", med, lo, hi, **extra)
        report(n, "prove: Q MSM G1 (2n points)", *median_ms(lambda: pp["pp_lhs"].msm((dc, 2 * n))))
        report(n, "verify", *median_ms(lambda: koe.opening_linear_form_verifier(L, pp, out["proof"], out["u"])))
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
