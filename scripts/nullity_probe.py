#!/usr/bin/env python3
"""Developer probe: Pi_Nullity's two products over a dense form matrix (verifiable_mpc_amd/nullity.py, csrc/nullity.hip)
against the composed device path the package offered before them, by shape.

For each (s, n) asked for (default 4x2^20 16x2^20 64x2^16), in ONE process and after warm-up of every shape and path:
  combine   FormMatrix.combine(rho)                      vs  sum(L_i * rho**i) over device forms (s scale + s axpy launches)
  values    FormMatrix.values(x)                         vs  [L_i(x)] (s inner products, a host round trip each)
A timed region is REPS calls ended by one device synchronisation; the figure is the median of RUNS regions per call, the
two paths alternating region by region.  Bytes are what the algorithm has to move, from the shape: 32 s n + 32 n for
either fused product (the matrix once, plus the output / x once), and the fraction is of the 8.0 TB/s HBM peak.  The
results of both paths are compared before anything is timed.  One line per measurement; `--out FILE` appends them as
JSON lines."""
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
HBM_PEAK = 8.0e12
ELL = vm.groups.ORDER


def regions(ctx, fns, reps):
    """{name: [ms per call]} - RUNS regions each, alternating between the functions"""
    out = {name: [] for name in fns}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    ctx.sync()
    for _ in range(RUNS):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ctx.sync()
            out[name].append((time.perf_counter() - t0) * 1e3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4x20", "16x20", "64x16"], help="<s>x<log2 n>")
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    rng = np.random.default_rng(17)
    lines = []

    def report(s, n, what, ts, **extra):
        rec = dict(s=s, n=n, what=what, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                   max_ms=round(max(ts), 4), **extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for shape in args.shapes:
        s, k = (int(v) for v in shape.split("x"))
        n = 1 << k
        raw = rng.integers(0, 256, size=(s * n + n, 32), dtype=np.uint8)
        raw[:, 31] &= 0x0F                                            # below 2^252 < l: canonical
        data = vm.ScalarVector.from_array(raw[:s * n], ctx)
        xs = vm.ScalarVector.from_array(raw[s * n:], ctx)
        fm = vm.FormMatrix.from_device(data, s, n)
        forms = fm.forms()
        rho = int.from_bytes(rng.bytes(32), "little") % ELL

        def composed_combine():
            return sum(L_i * rho ** i for i, L_i in enumerate(forms)).coeffs

        def composed_values():
            return [L_i(xs) for L_i in forms]

        got, want = fm.combine(rho), composed_combine()      # (held: a dropped vector's memory is reused at once)
        diff = ctx.cs_first_diff(got.ptr, want.ptr, n)
        assert diff is None, (shape, diff, hex(got[diff]), hex(want[diff]))
        assert fm.values(xs) == composed_values()
        reps = max(1, (1 << 28) // (s * n))          # a region is tens of milliseconds, not a fraction of one
        nbytes = 32 * s * n + 32 * n
        for what, fused, composed in (("combine", lambda: fm.combine(rho), composed_combine),
                                      ("values", lambda: fm.values(xs), composed_values)):
            ts = regions(ctx, {"fused": fused, "composed": composed}, reps)
            f, c = statistics.median(ts["fused"]), statistics.median(ts["composed"])
            report(s, n, what + ": fused", ts["fused"], bytes=nbytes, bytes_per_s=round(nbytes / (f * 1e-3)),
                   fraction_of_hbm_peak=round(nbytes / (f * 1e-3) / HBM_PEAK, 4), reps=reps)
            report(s, n, what + ": composed", ts["composed"], reps=reps, composed_over_fused=round(c / f, 3))
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
