"""The batch Protocol 8 prover over BN-256 against the loop of single calls
-> profiles/koe_prover_batch_probe.jsonl.

    python scripts/koe_prover_batch_probe.py [--log-m 12] [--Ks 1,4,16,64] [--reps 5] [--warmup 1] [--out FILE]

One layered random circuit of m = 2^log_m multiplication gates (16 depth levels, n_x = 8, two outputs; N = n_x + 3 + 2m),
one pp, the default modes.  Medians of `reps` runs after `warmup` runs, each bracketed by a stream synchronisation, with
the spread (max - min), of
    batch     circuit_sat_prover_batch(pp, circuit, xs, gf, koe)
    loop      [circuit_sat_prover(pp, circuit, x, gf, koe) for x in xs], same process, same inputs
The pp's tables and the circuit's device state exist before anything is timed.  At K = 16 one run of each under the
library's stage scopes: milliseconds and launches per stage group (triples, extension, staging, product, split, the
three row-MSMs together, forms), and the host time spent inside the per-witness form assembly (_Forms, combine and the
inner products queued around them).  Inputs and draws are random (timing only; correctness is
tests/test_gpu_circuit_sat_koe_batch.py)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = 16
GROUPS = (("triples", ("cs_triples",)), ("extension", ("cs_extend",)), ("staging", ("bn_koe_stage",)),
          ("product", ("bn_fr_poly", "bn_ntt")), ("split", ("bn_koe_split",)),
          ("row_msms", ("msm_", "bn_prep", "bn_bucket", "bn_reduce", "bn_final")))


def layered(rng, n_x, m, n_out):
    """CSR forms of m gates in LEVELS layers of m / LEVELS: a gate's left wire reads one gate of the layer before (so
    the depth levels ARE the layers) and one column among the inputs and the earlier layers, its right wire two such
    columns"""
    per = m // LEVELS

    def rows(count, limit_of, chained):
        ptr, col, vals = [0], [], []
        for i in range(count):
            cols = set(int(v) for v in rng.integers(0, limit_of(i), size=2))
            if chained and i >= per:
                cols.add(n_x + (i // per - 1) * per + int(rng.integers(0, per)))
            for c in sorted(cols):
                col.append(c)
                vals.append(int(rng.integers(1, 1 << 62)))
            ptr.append(len(col))
        return ptr, col, vals, [int(v) for v in rng.integers(0, 1 << 62, size=count)]
    below = lambda i: n_x + (i // per) * per        # noqa: E731
    return rows(m, below, True), rows(m, below, False), rows(n_out, lambda i: n_x + m, False)


def group_of(name):
    for group, prefixes in GROUPS:
        if name.startswith(prefixes):
            return group
    return "forms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", type=int, default=12)
    ap.add_argument("--Ks", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="profiles/koe_prover_batch_probe.jsonl")
    args = ap.parse_args()
    import verifiable_mpc_amd as vm
    from oracle import bn256_ref as bn
    from verifiable_mpc_amd import circuit_sat_gpu as cs
    from verifiable_mpc_amd import knowledge_of_exponent as koe
    ctx = vm.get_context()
    P = vm.pynocchio
    order = P.ORDER
    rng = np.random.default_rng(32)
    koe.prng = random.Random(32)
    cs.prng = random.Random(33)
    n_x, m, n_out = 8, 1 << args.log_m, 2
    N = n_x + 3 + 2 * m
    A, B, O = layered(rng, n_x, m, n_out)
    sc = cs.SparseCircuit(n_x, A, B, O, order=order)
    assert len(sc.level_ptr) - 1 == LEVELS
    gf = vm.GF(order)
    pp = koe.trusted_setup(P.BN256Point(bn.G1), P.BN256TwistPoint(bn.G2), N, order)
    Ks = [int(k) for k in args.Ks.split(",")]
    inputs = rng.integers(0, 256, size=(max(Ks + [16]), n_x, 32), dtype=np.uint8)
    inputs[:, :, 31] &= 0x7F
    lists = [[int.from_bytes(v.tobytes(), "little") for v in row] for row in inputs]

    def batch(K):
        return cs.circuit_sat_prover_batch(pp, sc, inputs[:K], gf, "koe")

    def loop(K):
        return [cs.circuit_sat_prover(pp, sc, x, gf, "koe") for x in lists[:K]]

    def timed(fn):
        out = []
        for i in range(args.warmup + args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            if i >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(out), 3), round(max(out) - min(out), 3)

    def staged(fn):
        """one run under the stage scopes -> ({group: [ms, launches]}, {stage: [ms, launches]}, host ms in the forms)"""
        host = [0.0]

        def clocked(real):
            def wrapper(*a, **kw):
                t0 = time.perf_counter()
                try:
                    return real(*a, **kw)
                finally:
                    host[0] += (time.perf_counter() - t0) * 1e3
            return wrapper
        real_init, real_combine = cs._Forms.__init__, cs._Forms.combine
        cs._Forms.__init__, cs._Forms.combine = clocked(real_init), clocked(real_combine)
        ctx.profile(True)
        ctx.profile_read(reset=True)
        try:
            fn()
            ctx.sync()
            st = ctx.profile_read(reset=True)
        finally:
            ctx.profile(False)
            cs._Forms.__init__, cs._Forms.combine = real_init, real_combine
        groups = {}
        for name, (ms, count) in st.items():
            g = groups.setdefault(group_of(name), [0.0, 0])
            g[0] += ms
            g[1] += count
        return ({k: [round(v[0], 4), v[1]] for k, v in groups.items()},
                {k: [round(v[0], 4), v[1]] for k, v in sorted(st.items())}, round(host[0], 3))

    # everything that is made once: the pp's tables (both sides), the circuit's device state, the arena
    loop(1)
    batch(max(Ks))
    verdict = cs.circuit_sat_verifier(batch(1)[0], pp, sc, gf, "koe")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:        # a run replaces the file
        def emit(row):
            row.update(m=m, N=N, levels=LEVELS, reps=args.reps, warmup=args.warmup)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit({"what": "proof_verifies", "verdict": verdict})
        for K in Ks:
            row = {"what": "circuit_sat_prover_batch_koe", "K": K}
            row["batch_ms"], row["batch_spread_ms"] = timed(lambda: batch(K))
            row["loop_ms"], row["loop_spread_ms"] = timed(lambda: loop(K))
            row["loop_over_batch"] = round(row["loop_ms"] / row["batch_ms"], 3)
            emit(row)
        for name, fn in (("batch", batch), ("loop", loop)):
            groups, stages, host_forms_ms = staged(lambda: fn(16))
            emit({"what": "stages", "path": name, "K": 16, "groups_ms_launches": groups, "stages_ms_launches": stages,
                  "host_ms_in_forms": host_forms_ms})


if __name__ == "__main__":
    main()
