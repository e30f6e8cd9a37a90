"""The batch Pinocchio prover against K single calls of the same build -> profiles/pinocchio_batch_probe.jsonl.

    python scripts/pinocchio_batch_probe.py --log-d 10 [--batch 1,8,64] [--reps 3] [--append]

One circuit size per run (a run is one process and one GPU step; --append adds its lines to the file instead of
replacing it).  d = 2^log_d constraints, each the product of two 2-term combinations of free input wires that defines
its own output wire, K witnesses with distinct inputs.  The median over `reps` runs after one warm-up run, each run
bracketed by synchronisations of the three streams, of every stage done once for all K (`*_batch_ms`) and done K times
the single way (`*_single_ms`):

    check, weights, moments, combine   the *_batch_dev entries of csrc/bn256_qap_h.hip against K single entries, on
                                       device-resident rows
    h                                  compute_h_batch against K compute_h (upload, row values and read-back included)
    proof                              compute_proof_batch against K compute_proof over one PreparedKey (a synthetic one:
                                       the sums cost what a generated key's cost), h read in place on the device
    prove                              prove_batch against K x (compute_h, compute_proof)

Every batch result is compared with the single one before its line is written (`equal`).  The single entries run the
batch entries' kernels with K = 1, so at K = 1 the two columns of a stage time the same launches."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def circuit(d, k, seed, order, n_io=4):
    """-> (V, W, Y as CSR with int64 values, out_ix, m, K witnesses as one (K, m + 1, 32) uint8 array)"""
    rng = np.random.default_rng(seed)
    n_free = n_io + d
    m = n_free + d
    ptr = np.arange(0, 2 * d + 1, 2)
    mats = []
    for _ in range(2):
        mats.append((ptr, rng.integers(0, n_free + 1, size=2 * d), rng.integers(1, 1 << 62, size=2 * d).astype(np.int64)))
    Y = (np.arange(d + 1), n_free + 1 + np.arange(d), np.ones(d, np.int64))
    cs = np.zeros((k, m + 1, 32), np.uint8)
    for w in range(k):
        c = [1] + [int(x) ** 4 % order for x in rng.integers(1, 1 << 62, size=n_free)]
        rows = []
        for _, col, vals in mats:
            cl, vl = col.tolist(), vals.tolist()
            rows.append([(vl[2 * r] * c[cl[2 * r]] + vl[2 * r + 1] * c[cl[2 * r + 1]]) % order for r in range(d)])
        c += [a * b % order for a, b in zip(*rows)]
        cs[w] = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in c), np.uint8).reshape(-1, 32)
    return mats[0], mats[1], Y, n_io, m, cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, required=True)
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default="profiles/pinocchio_batch_probe.jsonl")
    args = ap.parse_args()
    import types

    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import pynocchio as pn
    from verifiable_mpc_amd.device import get_aux_context
    ctx = vm.get_context()
    streams = [ctx, get_aux_context(20), get_aux_context(21)]
    d = 1 << args.log_d
    batches = [int(s) for s in args.batch.split(",")]

    def sync():
        for c in streams:
            c.sync()

    def timed(fn):
        out = []
        for i in range(args.reps + 1):          # the first run warms up
            sync()
            t0 = time.perf_counter()
            r = fn()
            sync()
            if i:
                out.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(out), 3), round(max(out) - min(out), 3), r

    V, W, Y, out_ix, m, cs_all = circuit(d, max(batches), 21 + args.log_d, pn.ORDER)
    qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
    key = pn.PreparedKey.synthetic(ctx, m + 1, seed=5)
    rng = np.random.default_rng(3)
    t = pn._t_coeffs(ctx, qap)
    with open(args.out, "a" if args.append else "w") as f:
        for K in batches:
            cs = cs_all[:K]
            dls = [types.SimpleNamespace(**{n: int(x) for n, x in zip("vwy", rng.integers(1, 1 << 62, size=3))})
                   for _ in range(K)]
            row = {"d": d, "K": K, "reps": args.reps}
            spread = {}

            def both(name, batch, single, same):
                row[name + "_batch_ms"], spread[name + "_batch"], rb = timed(batch)
                row[name + "_single_ms"], spread[name + "_single"], rs = timed(single)
                row["equal"] = row.get("equal", True) and bool(same(rb, rs))

            # ---- the stages on device-resident rows: a || b || y per witness, as compute_h_batch lays them out
            dc = ctx.upload(cs)
            aby = ctx.alloc(32 * 3 * d * K)
            plan = pn._per_ctx(qap, "rows", ctx, lambda: pn._row_plan(ctx, qap))
            for w in range(K):
                plan.run(dc.ptr + 32 * (m + 1) * w, m + 1, aby.ptr + 32 * 3 * d * w)
            dd = pn._scalar_buf(ctx, [getattr(dl, n) for dl in dls for n in "vwy"])
            ub, us, mb, ms_ = (ctx.alloc(32 * 2 * d * K) for _ in range(4))
            hb, hs_ = ctx.alloc(32 * (d + 1) * K), ctx.alloc(32 * (d + 1) * K)
            sb, ss = ctx.alloc(32 * 3 * d * K), ctx.alloc(32 * 5 * d)
            bad_b, bad_s = ctx.alloc(4 * K), ctx.alloc(4 * K)
            A = lambda buf, w, off=0: buf.ptr + 32 * (2 * d * w + off)
            R = lambda w, off: aby.ptr + 32 * (3 * d * w + off)
            get = lambda buf, n: ctx.download(buf.ptr, n).tobytes()
            both("check", lambda: ctx.bn256_qap_check_batch(R(0, 0), R(0, d), R(0, 2 * d), 3 * d, d, bad_b.ptr, K),
                 lambda: [ctx.bn256_qap_check(R(w, 0), R(w, d), R(w, 2 * d), d, bad_s.ptr + 4 * w) for w in range(K)],
                 lambda *_: get(bad_b, 4 * K) == get(bad_s, 4 * K) == b"\xff" * (4 * K))
            both("weights", lambda: ctx.bn256_qap_h_weights_batch(R(0, 0), R(0, d), 3 * d, d, A(ub, 0), A(ub, 0, d), 2 * d, K),
                 lambda: [ctx.bn256_qap_h_weights(R(w, 0), R(w, d), d, A(us, w), A(us, w, d)) for w in range(K)],
                 lambda *_: get(ub, 64 * d * K) == get(us, 64 * d * K))
            both("moments", lambda: ctx.bn256_qap_moments_batch(A(ub, 0), A(ub, 0, d), 2 * d, d, d, A(mb, 0), A(mb, 0, d),
                                                               2 * d, K),
                 lambda: [ctx.bn256_qap_moments(A(us, w), A(us, w, d), d, d, A(ms_, w), A(ms_, w, d)) for w in range(K)],
                 lambda *_: get(mb, 64 * d * K) == get(ms_, 64 * d * K))
            both("combine", lambda: ctx.bn256_qap_h_combine_batch(A(mb, 0), A(mb, 0, d), 2 * d, t.ptr, d, dd.ptr, sb.ptr,
                                                                 hb.ptr, d + 1, K),
                 lambda: [ctx.bn256_qap_h_combine(A(ms_, w), A(ms_, w, d), t.ptr, d, dd.ptr + 96 * w, ss.ptr,
                                                  hs_.ptr + 32 * (d + 1) * w) for w in range(K)],
                 lambda *_: get(hb, 32 * (d + 1) * K) == get(hs_, 32 * (d + 1) * K))
            del dc, aby, ub, us, mb, ms_, hb, hs_, sb, ss
            # ---- whole calls
            coeffs = lambda hs: [ctx.download(h.buf.ptr, 32 * len(h)).tobytes() for h in hs]
            both("h", lambda: pn.compute_h_batch(qap, cs, dls), lambda: [pn.compute_h(qap, c, dl) for c, dl in zip(cs, dls)],
                 lambda rb, rs: coeffs(rb) == coeffs(rs))
            hs = pn.compute_h_batch(qap, cs, dls)
            both("proof", lambda: pn.compute_proof_batch(qap, cs, hs, key, dls),
                 lambda: [pn.compute_proof(qap, c, h, key, dl) for c, h, dl in zip(cs, hs, dls)],
                 lambda rb, rs: rb == rs)
            both("prove", lambda: pn.prove_batch(qap, cs, key, dls),
                 lambda: [pn.compute_proof(qap, c, pn.compute_h(qap, c, dl), key, dl) for c, dl in zip(cs, dls)],
                 lambda rb, rs: rb == rs)
            row["spread_ms"] = spread
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            del hs


if __name__ == "__main__":
    main()
