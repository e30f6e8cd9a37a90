#!/usr/bin/env python3
"""Developer probe: the polynomial product over the BN-256 scalar field by the multi-prime NTT (csrc/bn256_ntt.hip)
against the schoolbook kernel (csrc/bn256_koe.hip), in ONE process -> profiles/ntt_probe.jsonl.

    python scripts/ntt_probe.py [--log-d 10 12 14 16 18] [--callers-log-d 12 14 16 18] [--out profiles/ntt_probe.jsonl]

  product     one d x d product through each entry on the same device buffers, the two entries alternating run by run:
              medians of timed runs after warm-up runs, a host clock around `reps` calls and one device synchronisation
              (reps chosen so that a run lasts some 20 ms or more), reported per call.  Then the NTT once more with the
              context's stage profile on: its four stages from HIP events, per call.
  threshold   the smallest power of two d (from 2) at which the NTT's median is below the schoolbook's, measured the
              same way, against the library's VMPC_BN256_FR_NTT_MIN.
  callers     compute_h, vmpc_bn256_qap_t_coeffs_dev and opening_linear_form_prover under mode 0 (schoolbook) and mode 1
              (auto), same inputs, the outputs compared byte for byte.
Inputs are random (timing only - correctness is tests/test_gpu_poly_mul_ntt.py).  The first line records the device
and, where the tool is there, the clocks it reports before and after."""
import argparse
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import verifiable_mpc_amd as vm                                       # noqa: E402
from oracle import bn256_ref as bn                                    # noqa: E402
from verifiable_mpc_amd import _native                                # noqa: E402
from verifiable_mpc_amd import knowledge_of_exponent as koe           # noqa: E402
from verifiable_mpc_amd import pynocchio as pn                        # noqa: E402
from h_probe import circuit                                           # noqa: E402

N = pn.ORDER
NTT_STAGES = ("bn_fr_ntt_split", "bn_fr_ntt_fwd", "bn_fr_ntt_inv", "bn_fr_ntt_crt")


def clocks():
    tool = shutil.which("rocm-smi")
    if not tool:
        return None
    try:
        out = subprocess.run([tool, "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "clock" in k.lower()}
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, nargs="+", default=[10, 12, 14, 16, 18])
    ap.add_argument("--callers-log-d", type=int, nargs="+", default=[12, 14, 16, 18])
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    rng = np.random.default_rng(25)
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    emit(what="session", device=_native.backend_info()[1], ntt_min=_native.BN256_FR_NTT_MIN, clocks_before=clocks())

    def timed(fn, reps, runs, warm):
        """median / min / max ms per call of `runs` timed runs of `reps` calls and one synchronisation each"""
        ts = []
        for i in range(warm + runs):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ctx.sync()
            if i >= warm:
                ts.append((time.perf_counter() - t0) * 1e3 / reps)
        return ts

    def pair(d):
        """the two entries on one pair of d-coefficient operands, alternating -> (schoolbook runs, NTT runs, reps)"""
        a = ctx.upload(rng.integers(0, 256, size=(d, 32), dtype=np.uint8))
        b = ctx.upload(rng.integers(0, 256, size=(d, 32), dtype=np.uint8))
        out_s, out_n = ctx.alloc(32 * (2 * d - 1)), ctx.alloc(32 * (2 * d - 1))
        school = lambda: ctx.bn256_fr_poly_mul(a.ptr, d, b.ptr, d, out_s.ptr)
        ntt = lambda: ctx.bn256_fr_poly_mul_ntt(a.ptr, d, b.ptr, d, out_n.ptr)
        school(), ntt(), ctx.sync()
        same = bool(np.array_equal(ctx.download(out_s.ptr, 32 * (2 * d - 1)), ctx.download(out_n.ptr, 32 * (2 * d - 1))))
        t0 = time.perf_counter()
        school(), ctx.sync()
        one = max((time.perf_counter() - t0) * 1e3, 0.02)
        reps = max(1, min(200, int(20 / one)))
        runs, warm = (5, 1) if one > 100 else (9, 2)
        ts_s, ts_n = [], []
        for i in range(warm + runs):                    # alternate the two: the same clocks and neighbours for both
            s, n = timed(school, reps, 1, 0)[0], timed(ntt, reps, 1, 0)[0]
            if i >= warm:
                ts_s.append(s)
                ts_n.append(n)
        return ts_s, ts_n, reps, same, ntt

    def stat(ts):
        return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))

    assert ctx.get_poly_product() == 0
    for k in args.log_d:
        d = 1 << k
        ts_s, ts_n, reps, same, ntt = pair(d)
        emit(what="product", d=d, entry="schoolbook", reps=reps, **stat(ts_s))
        emit(what="product", d=d, entry="ntt", reps=reps, same_bytes=same, **stat(ts_n),
             schoolbook_over_ntt=round(statistics.median(ts_s) / statistics.median(ts_n), 2))
        ctx.profile(True)
        ctx.profile_read(reset=True)
        for _ in range(reps):
            ntt()
        ctx.sync()
        prof = ctx.profile_read(reset=True)
        ctx.profile(False)
        emit(what="ntt stages", d=d, reps=reps, **{s: round(prof[s][0] / reps, 4) for s in NTT_STAGES if s in prof})

    found = None
    for k in range(1, 17):
        ts_s, ts_n, reps, same, _ = pair(1 << k)
        ms, mn = statistics.median(ts_s), statistics.median(ts_n)
        emit(what="threshold scan", d=1 << k, schoolbook_ms=round(ms, 4), ntt_ms=round(mn, 4), reps=reps, same_bytes=same)
        if found is None and mn < ms:
            found = 1 << k
    emit(what="threshold", measured=found, library=_native.BN256_FR_NTT_MIN)

    # ---- the callers, mode 0 against mode 1 ----
    deltas = types.SimpleNamespace(v=3 ** 100 % N, w=5 ** 100 % N, y=7 ** 100 % N)
    for k in args.callers_log_d:
        d = 1 << k
        runs, warm = (3, 1) if k >= 18 else (7, 2)
        V, W, Y, out_ix, m, c = circuit(d, seed=k)
        got = {}
        for mode in ("schoolbook", "auto"):
            with vm.device.poly_product(mode):
                scratch_t, t = ctx.alloc(64 * (d + (d + 127) // 128)), ctx.alloc(32 * (d + 1))
                ts = timed(lambda: ctx.bn256_qap_t_coeffs(d, scratch_t.ptr, t.ptr), 1, runs, warm)
                emit(what="t_coeffs", d=d, mode=mode, **stat(ts))
                qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
                pn.compute_h(qap, c, deltas)          # (makes and caches the plan and t)
                ts = timed(lambda: got.__setitem__(mode, pn.compute_h(qap, c, deltas)), 1, runs, warm)
                emit(what="compute_h", d=d, mode=mode, **stat(ts))
                got[mode] = (ctx.download(t.ptr, 32 * (d + 1)).tobytes(), got[mode].coeffs)
        emit(what="callers agree", d=d, same_bytes=got["schoolbook"] == got["auto"])
        del got
        if k > 16:
            continue
        koe.prng = random.Random(k)
        pp = koe.trusted_setup(pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2), d, pn.ORDER)
        rows = rng.integers(0, 256, size=(2 * d, 32), dtype=np.uint8)
        vals = [int.from_bytes(r.tobytes(), "little") % N for r in rows]
        L, xs = vm.pivot.LinearForm(vals[:d]), vals[d:]
        res = {}
        for mode in ("schoolbook", "auto"):
            with vm.device.poly_product(mode):
                ts = timed(lambda: res.__setitem__(mode, koe.opening_linear_form_prover(L, xs, 12345, pp)), 1, runs, warm)
                emit(what="opening_linear_form_prover", n=d, mode=mode, **stat(ts))
        emit(what="callers agree", n=d, same_bytes=all(
            res["schoolbook"][0][p].coords == res["auto"][0][p].coords for p in ("P", "pi", "Q")))
        del pp, res

    emit(what="session end", clocks_after=clocks())
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
