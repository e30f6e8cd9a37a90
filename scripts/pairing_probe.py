#!/usr/bin/env python3
"""Developer probe: BN-256 pairing latency and Pinocchio verifier throughput (csrc/bn256_pairing.hip).

Reports medians of timed runs after warm-up runs, each run bracketed by a device synchronisation:
  * one pairing at the C-ABI (vmpc_bn256_pairing_dev, inputs already on the device);
  * one verify at the C-ABI (vmpc_bn256_pairing_product_dev: 12 pairs, 5 products) and through Python
    (pynocchio.verify: key upload and validation, IO sums, pair assembly, the product launch);
  * verify_batch throughput in proofs/s for B = 64, 1024, 4096.
Inputs: the reference-made Pinocchio instance of tests/golden/bn256_pairing.json (timing only - correctness is
tests/test_gpu_bn256_pairing.py).  Prints one line per measurement; `--out FILE` also writes them as JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import verifiable_mpc_amd as vm                            # noqa: E402
from verifiable_mpc_amd import pynocchio as pn             # noqa: E402

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
    ctx = vm.get_context()
    case = json.load(open(os.path.join(ROOT, "tests", "golden", "bn256_pairing.json")))["pinocchio"]

    def mk(v, name):
        cls = pn.BN256TwistPoint if name.endswith("g2") else pn.BN256Point
        return cls(None if v is None else [int(x, 16) for x in v])

    class Q:
        indices_io = case["indices_io"]
    verikey = {k: mk(v, k) for k, v in case["verikey"].items()}
    proof = {k: mk(v, k) for k, v in case["proof"].items()}
    c = [int(v, 16) for v in case["c"]]
    out = {}

    g1 = np.frombuffer((1).to_bytes(32, "little") + (pn.P - 2).to_bytes(32, "little"), np.uint8)
    g2 = np.frombuffer(verikey["g2"].to_bytes(), np.uint8)
    d1, d2, gt = ctx.upload(g1), ctx.upload(g2), ctx.alloc(384)

    def one_pairing():
        ctx.bn256_pairing(d1.ptr, d2.ptr, 1, gt.ptr)
        ctx.sync()
    out["pairing_cabi_ms"] = median_ms(one_pairing)

    # one verify's 12 pairs / 5 products at the C-ABI
    d12a, d12b = ctx.upload(np.tile(g1, (12, 1))), ctx.upload(np.tile(g2, (12, 1)))
    doff, dones = ctx.upload(np.array([0, 3, 5, 7, 9, 12], np.uint32)), ctx.alloc(5)

    def one_product():
        ctx.bn256_pairing_product(d12a.ptr, d12b.ptr, 12, doff.ptr, 5, dones.ptr, None)
        ctx.sync()
    out["verify_cabi_ms"] = median_ms(one_product)
    out["verify_python_ms"] = median_ms(lambda: pn.verify(Q, verikey, proof, c))

    for B in (64, 1024, 4096):
        ms = median_ms(lambda: pn.verify_batch(Q, verikey, [proof] * B, [c] * B), runs=3, warm=1)
        out[f"verify_batch_{B}"] = {"ms": ms, "proofs_per_s": B / (ms[0] / 1e3)}
    # the product launch alone at B = 4096 (12 B pairs, 5 B products): the GPU part of verify_batch
    B = 4096
    dA, dB = ctx.upload(np.tile(g1, (12 * B, 1))), ctx.upload(np.tile(g2, (12 * B, 1)))
    off = (np.arange(B)[:, None] * 12 + np.array([0, 3, 5, 7, 9])).reshape(-1)
    doffB, donesB = ctx.upload(np.append(off, 12 * B).astype(np.uint32)), ctx.alloc(5 * B)

    def product_b():
        ctx.bn256_pairing_product(dA.ptr, dB.ptr, 12 * B, doffB.ptr, 5 * B, donesB.ptr, None)
        ctx.sync()
    ms = median_ms(product_b, runs=3, warm=1)
    out["product_launch_4096"] = {"ms": ms, "proofs_per_s": B / (ms[0] / 1e3)}
    for k, v in out.items():
        print(k, json.dumps(v))
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
