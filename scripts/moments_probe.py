#!/usr/bin/env python3
"""Developer probe: the moment transform by the subproduct tree (csrc/bn256_qap_mtree.hip) against the direct kernel
(csrc/bn256_qap_h.hip), in ONE process -> profiles/moments_tree_probe.jsonl.

    python scripts/moments_probe.py [--log-d 10 12 14 16 18] [--k 1 8] [--proof-log-d 16 18] [--out FILE]

  moments     two vectors of d scalars, n_out = d, K witnesses: the two entries on the same device buffers, alternating
              run by run, the plan cached; medians of timed runs after warm-up runs, a host clock around `reps` calls and
              one device synchronisation, per call, with the run-to-run spread (min, max).  The outputs compared byte for
              byte.  Then the tree once more with the context's stage profile on: leaves, levels, the reversal and the
              series product (the NTT's four stages, which only the series product runs here) from HIP events.
  plan build  once per d, a host clock around the call and a synchronisation.
  threshold   the smallest power of two of the grid from which the tree's median (K = 1) stays below the direct
              kernel's, against the library's VMPC_BN256_QAP_MTREE_MIN.
  compute_h   under poly_product("auto"), moment_transform "direct" against "tree", same inputs, same bytes; and
              compute_h + compute_proof over a synthetic prepared key at --proof-log-d.
Inputs are random (timing only - correctness is tests/test_gpu_moments_tree.py)."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import verifiable_mpc_amd as vm                                       # noqa: E402
from verifiable_mpc_amd import _native                                # noqa: E402
from verifiable_mpc_amd import pynocchio as pn                        # noqa: E402
from h_probe import circuit                                           # noqa: E402

N = pn.ORDER
TREE_STAGES = ("bn_qap_mtree_nleaf", "bn_qap_mtree_level", "bn_qap_mtree_reverse", "bn_fr_ntt_split", "bn_fr_ntt_fwd",
               "bn_fr_ntt_inv", "bn_fr_ntt_crt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, nargs="+", default=[10, 12, 14, 16, 18])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--proof-log-d", type=int, nargs="+", default=[16, 18])
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = vm.get_context()
    rng = np.random.default_rng(26)
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def once(fn, reps=1):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    def stat(ts):
        return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))

    emit(what="session", device=_native.backend_info()[1], mtree_min=_native.BN256_QAP_MTREE_MIN)
    medians = {}
    for k in args.log_d:
        d = 1 << k
        plan = ctx.alloc(_native.bn256_qap_mtree_bytes(d, d))
        ctx.sync()
        emit(what="plan build", d=d, bytes=plan.nbytes, ms=round(once(lambda: ctx.bn256_qap_mtree_build(d, d, plan.ptr)), 3))
        for K in args.k:
            u = ctx.upload(rng.integers(0, 256, size=(K, 2 * d, 32), dtype=np.uint8))
            out_d, out_t = ctx.alloc(64 * d * K), ctx.alloc(64 * d * K)
            scratch = ctx.alloc(_native.bn256_qap_moments_tree_scratch_bytes(d, K))
            direct = lambda: ctx.bn256_qap_moments_batch(u.ptr, u.ptr + 32 * d, 2 * d, d, d, out_d.ptr,
                                                         out_d.ptr + 32 * d, 2 * d, K)
            tree = lambda: ctx.bn256_qap_moments_tree_batch(plan.ptr, d, d, u.ptr, u.ptr + 32 * d, 2 * d, d, out_t.ptr,
                                                            out_t.ptr + 32 * d, 2 * d, scratch.ptr, K)
            one = max(once(direct), 0.02)
            once(tree)
            same = bool(np.array_equal(ctx.download(out_d.ptr, 64 * d * K), ctx.download(out_t.ptr, 64 * d * K)))
            reps = max(1, min(100, int(20 / one)))
            runs, warm = (3, 1) if one > 500 else (5, 1) if one > 100 else (9, 2)
            ts_d, ts_t = [], []
            for i in range(warm + runs):                # alternate the two: the same clocks and neighbours for both
                a, b = once(direct, reps), once(tree, reps)
                if i >= warm:
                    ts_d.append(a)
                    ts_t.append(b)
            emit(what="moments", d=d, K=K, entry="direct", reps=reps, **stat(ts_d))
            emit(what="moments", d=d, K=K, entry="tree", reps=reps, same_bytes=same, **stat(ts_t),
                 direct_over_tree=round(statistics.median(ts_d) / statistics.median(ts_t), 2))
            medians[d, K] = (statistics.median(ts_d), statistics.median(ts_t))
            ctx.profile(True)
            ctx.profile_read(reset=True)
            for _ in range(reps):
                tree()
            ctx.sync()
            prof = ctx.profile_read(reset=True)
            ctx.profile(False)
            emit(what="tree stages", d=d, K=K, reps=reps,
                 **{s: round(prof[s][0] / reps, 4) for s in TREE_STAGES if s in prof})
            del u, out_d, out_t, scratch
        del plan

    ds = sorted(d for d, K in medians if K == 1)
    found = None
    for d in reversed(ds):
        if medians[d, 1][1] < medians[d, 1][0]:
            found = d
        else:
            break
    emit(what="threshold", measured=found, library=_native.BN256_QAP_MTREE_MIN)

    deltas = types.SimpleNamespace(v=3 ** 100 % N, w=5 ** 100 % N, y=7 ** 100 % N)
    with vm.device.poly_product("auto"):
        for k in args.log_d:
            d = 1 << k
            runs, warm = (3, 1) if k >= 18 else (7, 2)
            V, W, Y, out_ix, m, c = circuit(d, seed=k)
            qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
            got, med = {}, {}
            for mode in ("direct", "tree"):
                with vm.device.moment_transform(mode):
                    pn.compute_h(qap, c, deltas)          # (makes and caches the plans and t)
                    ts = [once(lambda: got.__setitem__(mode, pn.compute_h(qap, c, deltas))) for _ in range(warm + runs)]
                    med[mode] = statistics.median(ts[warm:])
                    emit(what="compute_h", d=d, moment_transform=mode, **stat(ts[warm:]))
            emit(what="compute_h agrees", d=d, same_coeffs=got["direct"].coeffs == got["tree"].coeffs)
            if k in args.proof_log_d:
                key = pn.PreparedKey.synthetic(ctx, m + 1)
                ts = [once(lambda: pn.compute_proof(qap, c, got["tree"], key, deltas)) for _ in range(warm + runs)]
                cp = statistics.median(ts[warm:])
                emit(what="compute_proof", d=d, **stat(ts[warm:]))
                emit(what="compute_h + compute_proof", d=d, direct_ms=round(med["direct"] + cp, 3),
                     tree_ms=round(med["tree"] + cp, 3))
                del key
            del got, qap

    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
