"""CPU check of csrc/scale_chain.h, the per-point chain of vmpc_bn256_scale_points_dev (no GPU).

The header is `__host__ __device__`; tests/native/scale_chain_host_test.cpp compiles it with g++ (AddressSanitizer and
UndefinedBehaviorSanitizer) over the fields the kernel computes in and takes a case from memory bytes to memory bytes
as the kernel does.  Every case is compared with the program's own plain double-and-add (a branch per bit) and with
oracle/bn256_ref.py's affine law on Python ints, on the scalars that take the branch-free chain through the special
cases of the group law: 0, 1, 2, n - 1, n, n + 1, 2^255, 2^256 - 1 (used as they stand, not reduced) and random ones,
on a point, on its negative and on infinity."""
import os
import random
import subprocess

import pytest

from oracle import bn256_ref as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "scale_chain_host_test.cpp")
N = bn.N
TOP = (1 << 256) - 1
EDGE = [0, 1, 2, N - 1, N, N + 1, 1 << 255, TOP]
CURVE = {1: (bn.E1, bn.G1, bn.g1_to_bytes), 2: (bn.E2, bn.G2, bn.g2_to_bytes)}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "scale_chain_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])

    def run(cases):
        """cases: (group, point bytes, scalar) -> list of (chain's bytes, plain double-and-add's bytes)"""
        lines = [f"{g} {pt.hex()} {k.to_bytes(32, 'little').hex()}" for g, pt, k in cases]
        res = subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                      UBSAN_OPTIONS="print_stacktrace=1"))
        assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
            res.stderr[-2000:]
        out = res.stdout.strip().split("\n")
        assert len(out) == len(cases), (len(out), len(cases))
        return [tuple(bytes.fromhex(h) for h in o.split()) for o in out]
    return run


@pytest.mark.parametrize("group", [1, 2])
def test_chain_equals_plain_double_and_add_and_the_oracle(harness, group):
    E, G, enc = CURVE[group]
    rng = random.Random(30 + group)
    P = E.mul(rng.randrange(1, N), G)
    scalars = EDGE + [rng.getrandbits(256) | 1 << 255, rng.randrange(1, N), rng.getrandbits(64)]
    cases, want = [], []
    for pt in (P, E.neg(P), None):
        for k in scalars:
            cases.append((group, enc(pt), k))
            want.append(enc(E.mul(k, pt) if pt is not None else None))
    got = harness(cases)
    for (chain, plain), w, (_, _, k) in zip(got, want, cases):
        assert chain == plain == w, hex(k)


def test_the_edge_scalars_give_what_they_should(harness):
    """n - 1 gives -P, n infinity, n + 1 P again, 0 infinity; infinity stays infinity under every scalar"""
    E, G, enc = CURVE[1]
    P = E.mul(5, G)
    got = [c for c, _ in harness([(1, enc(P), k) for k in (0, 1, N - 1, N, N + 1)] + [(1, bytes(64), k) for k in EDGE])]
    assert got[:5] == [bytes(64), enc(P), enc(E.neg(P)), bytes(64), enc(P)]
    assert got[5:] == [bytes(64)] * len(EDGE)
