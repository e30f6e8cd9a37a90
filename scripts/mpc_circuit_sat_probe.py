"""Stage times of Protocol 8 over a secret-shared witness (verifiable_mpc_amd/mpc_circuit_sat.py): M = 3 parties,
t = 1, all in one process on ONE GPU (LocalHub) -> profiles/mpc_circuit_sat_probe.jsonl.

    python scripts/mpc_circuit_sat_probe.py [--sizes 10,14] [--kinds inner,chain] [--reps 3] [--out ...]

Per circuit of scripts/circuit_sat_probe.py (an inner product: depth 1; a product chain: depth = m): medians of `reps`
runs after a warm-up, every stage bracketed by a stream synchronisation, of the stages AS THE THREE PARTIES RUN THEM
TOGETHER (wall time of the three coroutines on the shared GPU, exchanges included):
    triples      the wires' forms by level and their schur_prod (one exchange per level)
    extension    r_a, r_b (random_shares), the gate-order wires, vmpc_fr_cs_extend_fg_dev
    schur        the one product (f(0), f(m+1..2m)) x g's
    commitment   gamma and [z]
    pivot        y's, outputs, L, and the MPC Protocol 5
(the pivot's span includes the y's, the outputs and L) beside the single-party circuit_sat_prover's stages on the same
circuit in the same run.  One GPU serves all three parties here, so the local work is done three times over on it;
`replicated_share` = M x the single-party total / the M-party total says how much of the M-party time that is."""
import argparse
import asyncio
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.circuit_sat_probe import circuits      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14")
    ap.add_argument("--kinds", default="inner,chain")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parties", type=int, default=3)
    ap.add_argument("--threshold", type=int, default=1)
    ap.add_argument("--out", default="profiles/mpc_circuit_sat_probe.jsonl")
    args = ap.parse_args()
    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    from verifiable_mpc_amd import mpc_ac20, mpc_circuit_sat as mcs
    ctx = vm.get_context()
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    rng = np.random.default_rng(8)
    M, t = args.parties, args.threshold
    loop = asyncio.new_event_loop()

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), r

    def together(rts, fn):
        async def everybody():
            return await asyncio.gather(*[fn(p, rt) for p, rt in enumerate(rts)])
        return loop.run_until_complete(everybody())

    with open(args.out, "w") as f:
        for k in [int(s) for s in args.sizes.split(",")]:
            m = 1 << k
            for kind in args.kinds.split(","):
                n_x, A, B, O = circuits(kind, m)
                sc = cs.SparseCircuit(n_x, A, B, O)
                x = sc.pad([3] * n_x if kind == "inner" else [1])
                n_in, N = len(x), len(x) + 3 + 2 * m
                exps = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
                exps[:, 31] &= 0x0f
                g = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
                gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 12345)}
                g.precompute([gens["h"], gens["k"]])
                levels = len(sc.level_ptr) - 1
                row = {"kind": kind, "m": m, "N": N, "levels": levels, "parties": M, "threshold": t, "reps": args.reps}

                # ---- one prover who knows x -----------------------------------------------------------------------
                single = {}
                cs.circuit_sat_prover(gens, sc, x, gf)           # warm-up
                single["witness_ms"], _ = timed(lambda: cs._witness_on_device(sc, x, gf.order), args.reps)
                p8 = cs.protocol_8_excl_pivot_prover(gens, sc, x, gf)
                _, zc, L, zv, gm = p8
                single["commitment_ms"], _ = timed(lambda: vm.pivot.vector_commitment(zv, gm, g, gens["h"]), args.reps)
                single["pivot_ms"], _ = timed(lambda: vm.compressed_pivot.protocol_5_prover(
                    gens, zc, L, L(zv), zv, gm, gf, transcript="compact", r=vm.compressed_pivot.masks(N, ctx), rho=12345),
                    args.reps)
                single["total_ms"], proof1 = timed(lambda: cs.circuit_sat_prover(gens, sc, x, gf), args.reps)
                row["single"] = single

                # ---- M parties ----------------------------------------------------------------------------------------
                hub = mpc_ac20.LocalHub(M)
                rts = [mpc_ac20.PartyRuntime(p, M, t, random.Random(p), hub) for p in range(M)]
                dealt = mpc_ac20.deal(x, t, M, random.Random(5))
                xs = [mpc_ac20.SecureVector.from_shares(dealt[p], rts[p]) for p in range(M)]
                names = ("triples", "extension", "schur", "commitment", "pivot")
                stage = {name: [] for name in names + ("total",)}

                def run_once():
                    spans, clock = {}, {}

                    # the parties run in step between exchanges and in party order: the last party ends a stage last
                    def hook(rt, name):
                        if rt.pid == M - 1:
                            ctx.sync()
                            now = time.perf_counter()
                            spans[name] = (now - clock["t"]) * 1e3
                            clock["t"] = now
                    mcs.STAGE_HOOK = hook
                    try:
                        ctx.sync()
                        t0 = clock["t"] = time.perf_counter()
                        proofs = together(rts, lambda p, rt: mcs.circuit_sat_prover(gens, sc, xs[p], gf, rt=rt))
                        ctx.sync()
                        spans["total"] = (time.perf_counter() - t0) * 1e3
                    finally:
                        mcs.STAGE_HOOK = None
                    return spans, proofs

                run_once()                                          # warm-up
                for _ in range(args.reps):
                    spans, proofs = run_once()
                    for name in stage:
                        stage[name].append(spans[name])
                med = {name: statistics.median(v) for name, v in stage.items()}
                row["mpc"] = {name + "_ms": v for name, v in med.items()}
                verdict = cs.circuit_sat_verifier(proofs[0], gens, sc, gf)
                row["verified"] = all(verdict.values()) and len(verdict) == 3
                row["total_over_single"] = med["total"] / single["total_ms"]
                row["replicated_share"] = M * single["total_ms"] / med["total"]
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                del g, gens, proofs, p8, zc, L, zv, xs
                ctx.trim()


if __name__ == "__main__":
    main()
