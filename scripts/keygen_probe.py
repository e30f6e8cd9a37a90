#!/usr/bin/env python3
"""Developer probe: Pinocchio key generation on the GPU (verifiable_mpc_amd/pynocchio.py PreparedKey.generate,
csrc/bn256_keygen.hip) by size, and the reference's Python key generation for comparison.

GPU mode (default): for each d asked for (--d, or --log-d: default 2^12 2^16 2^18), a synthetic R1CS of d constraints and about d wires
(tests/keygen_ref.synthetic_r1cs: 1 to 3 entries per row, wire 0 in 3/4 of the rows), medians of timed runs after a
warm-up, each ended by a device synchronisation:
  generate          PreparedKey.generate: evaluation at s, exponents, fixed-base launches, validation and tables
  lagrange          vmpc_bn256_qap_lagrange_dev (l_j(s), t(s))
  colsum            vmpc_bn256_qap_colsum_dev over the three matrices
  powers            vmpc_bn256_fr_powers_dev (s^1 .. s^d)
  exps              vmpc_bn256_keygen_exps_dev (seven vectors)
  fixed_base        the eight bn256_fixed_base launches of the key vectors
  evalkey+verikey   generate_evalkey + generate_verikey (the reference's dict API, points to the host), d <= 4096
  host_plan         R1CSQAP construction (host transposition) and the upload of its column plan (once per circuit)
Reference mode (--reference, a host with the reference checkout named by VMPC_REFERENCE): the reference's code_to_qap
.QAP and Generators + generate_evalkey + generate_verikey over the mpyc shim, for programs y = x^k + x + 5 (d = k + 1),
until one run of QAP + keygen passes --budget seconds.  One JSON line per measurement; `--out FILE` appends them."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, RUNS = 1, 3


def median_ms(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def gpu(args, report):
    import numpy as np
    import verifiable_mpc_amd as vm
    from oracle import bn256_ref as bn
    from tests import keygen_ref as K
    from verifiable_mpc_amd import pynocchio as pn
    ctx = vm.get_context()
    for d in args.d or [1 << k for k in args.log_d]:
        V, W, Y, out_ix, m = K.synthetic_r1cs(d, seed=d)
        t0 = time.perf_counter()
        qap = pn.R1CSQAP(V, W, Y, out_ix, m=m)
        plan = qap._plan(ctx)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        report(d, "host_plan", ms, ms, ms, nnz=plan.nnz, items=plan.n_items, long_cols=plan.n_long)
        r = random.Random(d)
        td = K.TD(*(r.randrange(K.N) for _ in range(8)))
        gen = pn.Generators(td, pn.BN256Point(bn.G1), pn.BN256TwistPoint(bn.G2))

        def generate():
            pn.PreparedKey.generate(td, qap, gen)
            ctx.sync()
        report(d, "generate", *median_ms(generate))
        if d <= 4096:
            report(d, "evalkey+verikey dicts", *median_ms(lambda: (pn.generate_evalkey(td, qap, gen),
                                                                    pn.generate_verikey(td, qap, gen))))
        at = pn._QAPAtS(ctx, qap, td.s)
        ctx.sync()
        sb = ctx.upload(K.to_array([td.s, 1]))
        ell, t, pw = ctx.alloc(32 * d), ctx.alloc(32), ctx.alloc(32 * d)

        def run(fn):
            def go():
                fn()
                ctx.sync()
            return go
        report(d, "lagrange", *median_ms(run(lambda: ctx.bn256_qap_lagrange(sb.ptr, d, ell.ptr, t.ptr))))
        report(d, "colsum", *median_ms(run(lambda: plan.run(ell.ptr, d, at.vwyt.ptr))))
        report(d, "powers", *median_ms(run(lambda: ctx.bn256_fr_powers(sb.ptr, sb.ptr + 32, d, pw.ptr))))
        mid = list(qap.indices_mid)
        report(d, "exps", *median_ms(run(lambda: at.exps(ctx, td, mid))))
        exps = at.exps(ctx, td, mid)
        n = len(mid)
        g1 = ctx.upload(np.frombuffer(bn.g1_to_bytes(bn.G1), np.uint8))
        g2 = ctx.upload(np.frombuffer(bn.g2_to_bytes(bn.G2), np.uint8))
        outs = [ctx.alloc(128 * (n + 3)) for _ in range(7)] + [ctx.alloc(64 * (d + 1))]

        def fixed_base():
            for j in range(7):
                grp, base = (2, g2) if j == 1 else (1, g1)
                ctx.bn256_fixed_base(grp, base.ptr, exps.ptr + 32 * j * (n + 3), n + (1 if j == 1 else 3), outs[j].ptr)
            ctx.bn256_fixed_base(1, g1.ptr, at.powers.ptr, d + 1, outs[7].ptr)
        report(d, "fixed_base", *median_ms(run(fixed_base)))


def reference(args, report):
    os.environ.setdefault("VMPC_REFERENCE", "")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_pairing_fixtures as mpf                               # checks VMPC_REFERENCE
    sys.modules["verifiable_mpc.ac20.pairing"] = mpf.load_reference_pairing()
    from mpyc.finfields import GF                                    # (shim)
    from mpyc.fingroups import EllipticCurve                         # (shim)
    import verifiable_mpc.trinocchio.pynocchio as rp                 # (reference)
    import verifiable_mpc.tools.code_to_qap as c2q
    bn_curve, bn_twist = EllipticCurve("BN256", "jacobian"), EllipticCurve("BN256_twist", "jacobian")
    n = bn_curve.order
    gf = GF(modulus=n)
    gf.is_signed = False
    for k in args.ref_k:
        code = f"\ndef qeval(x):\n    y = x**{k}\n    return y + x + 5\n"
        t0 = time.perf_counter()
        qap = c2q.QAP(code, gf)
        t_qap = time.perf_counter() - t0
        rp.prng = random.Random(k)
        td = rp.Trapdoor(n)
        t0 = time.perf_counter()
        gen = rp.Generators(td, bn_curve.generator, bn_twist.generator)
        rp.generate_evalkey(td, qap, gen)
        rp.generate_verikey(td, qap, gen)
        t_key = time.perf_counter() - t0
        report(qap.d, "reference keygen", t_key * 1e3, t_key * 1e3, t_key * 1e3, m=qap.m, qap_ms=round(t_qap * 1e3, 1))
        if t_qap + t_key > args.budget:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, nargs="+", default=[12, 16, 18])
    ap.add_argument("--d", type=int, nargs="+", help="sizes d themselves (instead of --log-d)")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-k", type=int, nargs="+", default=[15, 31, 63, 95, 127])
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def report(d, what, med, lo, hi, **extra):
        rec = dict(d=d, what=what, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), **extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    (reference if args.reference else gpu)(args, report)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
