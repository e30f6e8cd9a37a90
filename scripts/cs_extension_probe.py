#!/usr/bin/env python3
"""Developer probe: Protocol 8's extension of f, g, h (csrc/circuit_sat.hip) by the multi-prime NTT against the direct
correlation kernel, in ONE process -> profiles/cs_extension_probe.jsonl.

    python scripts/cs_extension_probe.py [--out profiles/cs_extension_probe.jsonl] [--skip-largest] [--skip-prover]

  extension   vmpc_fr_cs_extend_dev at m = 2^6, 2^8, .., 2^18 and 2^19 - 2 under "direct" and "ntt" on the same device
              buffers, the two modes alternating run by run: medians of timed runs after warm-up runs, a host clock
              around `reps` calls and one device synchronisation (reps chosen so that a run lasts some 20 ms or more),
              reported per call; the z tails compared byte for byte.  At 2^19 - 2 the direct kernel runs ONCE (the
              comparison run is the timed one).  Then the NTT once more with the context's stage profile on: its four
              stages from HIP events, per call.
  threshold   the smallest power of two on that grid at which the NTT's median is below the direct kernel's and stays
              below at every larger grid size, against the library's VMPC_FR_CS_EXT_NTT_MIN.
  batch       vmpc_fr_cs_extend_batch_dev at K = 16 for m = 2^10 and 2^14, the same way.
  prover      circuit_sat_prover end to end on the "inner" circuit of scripts/circuit_sat_probe.py at m = 2^14 and 2^16
              under both modes, every random draw fixed, the proofs compared field by field.
Inputs are random (timing only - correctness is tests/test_gpu_cs_extension_ntt.py)."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import verifiable_mpc_amd as vm                                       # noqa: E402
from verifiable_mpc_amd import _native                                # noqa: E402
from verifiable_mpc_amd import circuit_sat_gpu as cs                  # noqa: E402
from verifiable_mpc_amd import wire                                   # noqa: E402
from circuit_sat_probe import circuits                                # noqa: E402

NTT_STAGES = ("cs_extend_ntt_split", "cs_extend_ntt_fwd", "cs_extend_ntt_inv", "cs_extend_ntt_crt")
MODES = ("direct", "ntt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-largest", action="store_true")
    ap.add_argument("--skip-prover", action="store_true")
    args = ap.parse_args()
    ctx = vm.get_context()
    rng = np.random.default_rng(28)
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    emit(what="session", device=_native.backend_info()[1], ntt_min=_native.FR_CS_EXT_NTT_MIN)

    def timed(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    def stat(ts):
        return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                    runs=len(ts))

    def canonical(shape):
        a = rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)
        a[..., 31] &= 0x0f
        return a

    def alternate(call, read, direct_once=False):
        """call(mode) under each mode alternating -> ({mode: runs}, reps, same bytes)"""
        out, first = {}, {}
        for mode in MODES:
            with vm.device.cs_extension(mode):
                first[mode] = timed(lambda: call(mode), 1)
            out[mode] = read(mode)
        same = bool(np.array_equal(out["direct"], out["ntt"]))
        if direct_once:
            reps = 1
            ts = {"direct": [first["direct"]], "ntt": []}
            for i in range(1 + 5):
                with vm.device.cs_extension("ntt"):
                    t = timed(lambda: call("ntt"), 1)
                if i >= 1:
                    ts["ntt"].append(t)
            return ts, reps, same
        with vm.device.cs_extension("direct"):
            one = max(timed(lambda: call("direct"), 1), 0.02)
        reps = max(1, min(200, int(20 / one)))
        runs, warm = (5, 1) if one > 100 else (9, 2)
        ts = {mode: [] for mode in MODES}
        for i in range(warm + runs):                    # alternate the two: the same clocks and neighbours for both
            for mode in MODES:
                with vm.device.cs_extension(mode):
                    t = timed(lambda: call(mode), reps)
                if i >= warm:
                    ts[mode].append(t)
        return ts, reps, same

    def stages(call, reps):
        with vm.device.cs_extension("ntt"):
            ctx.profile(True)
            ctx.profile_read(reset=True)
            for _ in range(reps):
                call("ntt")
            ctx.sync()
            prof = ctx.profile_read(reset=True)
            ctx.profile(False)
        return {s: round(prof[s][0] / reps, 4) for s in ("cs_extend_prep",) + NTT_STAGES + ("cs_extend_finish",) if s in prof}

    assert ctx.get_cs_extension() == 0
    grid = [1 << k for k in range(6, 19, 2)] + ([] if args.skip_largest else [(1 << 19) - 2])
    medians = {}
    for m in grid:
        fact, ifact = ctx.alloc(32 * (2 * m + 2)), ctx.alloc(32 * (2 * m + 2))
        ctx.cs_tables(2 * m + 1, fact.ptr, ifact.ptr)
        a, b = ctx.upload(canonical((m + 1,))), ctx.upload(canonical((m + 1,)))
        z = {mode: ctx.alloc(32 * (2 * m + 3)) for mode in MODES}

        def call(mode):
            ctx.cs_extend(a.ptr, b.ptr, m, fact.ptr, ifact.ptr, z[mode].ptr)

        def read(mode):
            # (the gammas' places are not the entry's: compare what it writes)
            t = ctx.download(z[mode].ptr, 32 * (2 * m + 3)).reshape(-1, 32)
            return np.concatenate([t[:3], t[m + 3:]])
        ts, reps, same = alternate(call, read, direct_once=m > (1 << 18))
        medians[m] = {mode: statistics.median(ts[mode]) for mode in MODES}
        emit(what="extension", m=m, L=ctx.cs_extend_ntt_len(m), mode="direct", reps=reps, **stat(ts["direct"]))
        emit(what="extension", m=m, L=ctx.cs_extend_ntt_len(m), mode="ntt", reps=reps, same_bytes=same, **stat(ts["ntt"]),
             direct_over_ntt=round(medians[m]["direct"] / medians[m]["ntt"], 2))
        emit(what="ntt stages", m=m, reps=reps, **stages(call, reps))
        del fact, ifact, a, b, z
        ctx.trim()

    pow2 = [m for m in grid if m & (m - 1) == 0]
    found = None
    for m in reversed(pow2):
        if not all(medians[g]["ntt"] < medians[g]["direct"] for g in grid if g >= m):
            break
        found = m
    emit(what="threshold", measured=found, library=_native.FR_CS_EXT_NTT_MIN,
         ntt_slower_at=[g for g in grid if medians[g]["ntt"] >= medians[g]["direct"]])

    K = 16
    for m in (1 << 10, 1 << 14):
        fact, ifact = ctx.alloc(32 * (2 * m + 2)), ctx.alloc(32 * (2 * m + 2))
        ctx.cs_tables(2 * m + 1, fact.ptr, ifact.ptr)
        a, b = ctx.upload(canonical((K, m + 1))), ctx.upload(canonical((K, m + 1)))
        z = {mode: ctx.alloc(32 * K * (2 * m + 3)) for mode in MODES}

        def call(mode):
            ctx.cs_extend_batch(a.ptr, b.ptr, m + 1, m, fact.ptr, ifact.ptr, z[mode].ptr, 2 * m + 3, K)

        def read(mode):
            t = ctx.download(z[mode].ptr, 32 * K * (2 * m + 3)).reshape(K, -1, 32)
            return np.concatenate([t[:, :3], t[:, m + 3:]], axis=1)
        ts, reps, same = alternate(call, read)
        emit(what="batch", m=m, K=K, mode="direct", reps=reps, **stat(ts["direct"]))
        emit(what="batch", m=m, K=K, mode="ntt", reps=reps, same_bytes=same, **stat(ts["ntt"]),
             direct_over_ntt=round(statistics.median(ts["direct"]) / statistics.median(ts["ntt"]), 2))
        emit(what="ntt stages", m=m, K=K, reps=reps, **stages(call, reps))
        del fact, ifact, a, b, z
        ctx.trim()

    if not args.skip_prover:
        group = vm.EllipticCurve("Ed25519", "projective")
        gf = vm.GF(group.order)
        real_masks = vm.compressed_pivot.masks

        def proof_bytes(proof):
            pp = proof["pivot_proof"]
            return [wire.compress_point(proof["z_commitment"])] + [int(proof[k]) % gf.order for k in ("y1", "y2", "y3")] + \
                [int(o) % gf.order for o in proof["outputs"]] + \
                [[int(v) % gf.order for v in pp[k]] if k == "z_prime" else int(pp[k]) % gf.order if k == "t" else
                 wire.compress_point(pp[k]) for k in pp]

        for m in (1 << 14, 1 << 16):
            n_x, A, B, O = circuits("inner", m)
            sc = cs.SparseCircuit(n_x, A, B, O)
            x = sc.pad([3] * n_x)
            N = len(x) + 3 + 2 * m
            exps = canonical((N,))
            g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
            gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 12345)}
            g.precompute([gens["h"], gens["k"]], wide=N >= (1 << 19) - 1)

            def prove():
                """every draw fixed: r_a, r_b, gamma, the pivot's masks and rho"""
                cs.prng = random.Random(m)
                vm.compressed_pivot.prng = random.Random(m + 1)
                mask_rng = np.random.default_rng(m + 2)

                def masks(n, c):
                    raw = mask_rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
                    raw[:, 31] &= 0x0f
                    return vm.ScalarVector.from_array(raw, c)
                vm.compressed_pivot.masks = masks
                try:
                    return cs.circuit_sat_prover(gens, sc, x, gf)
                finally:
                    vm.compressed_pivot.masks = real_masks
            proofs, ts = {}, {mode: [] for mode in MODES}
            for i in range(1 + 5):
                for mode in MODES:
                    with vm.device.cs_extension(mode):
                        ctx.sync()
                        t0 = time.perf_counter()
                        proofs[mode] = prove()
                        ctx.sync()
                        if i >= 1:
                            ts[mode].append((time.perf_counter() - t0) * 1e3)
            same = proof_bytes(proofs["direct"]) == proof_bytes(proofs["ntt"])
            for mode in MODES:
                emit(what="circuit_sat_prover", circuit="inner", m=m, N=N, mode=mode, **stat(ts[mode]),
                     **({"same_proof": same} if mode == "ntt" else {}))
            del g, gens, proofs, sc
            ctx.trim()

    emit(what="session end")
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
