"""CPU check of the small multiplication and the lazy sum of csrc/fr_bn.h (frbn_mul_small, frbn_wide), the arithmetic
of the moment transform (csrc/bn256_qap_h.hip).

Built with g++ under AddressSanitizer and UndefinedBehaviorSanitizer (tests/native/frbn_small_host_test.cpp) and
compared with Python integers at the extremes the kernel relies on: operands n - 1 and 2^256 - 1, the multiplier
2^21 - 1, and the largest number of summands (4 values per lane, 64 lanes, 4 waves, 1024 chunks of a workgroup)."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "frbn_small_host_test.cpp")
N = 65000549695646603732796438742359905742570406053903786389881062969044166799969
TOP = (1 << 256) - 1
JMAX = (1 << 21) - 1
EDGE = [0, 1, N - 1, N, N + 1, TOP, 1 << 255, (1 << 192) - 1, 1 << 192]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "frbn_small_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\nquit\n", text=True, capture_output=True,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                      UBSAN_OPTIONS="print_stacktrace=1"))
        assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
            res.stderr[-2000:]
        out = res.stdout.strip().split("\n")
        assert len(out) == len(lines), (len(out), len(lines))
        return [int(o, 16) for o in out]
    return run


def test_small_multiplication(harness):
    rng = random.Random(1)
    js = [0, 1, 2, 3, 255, 65535, 65536, (1 << 20), JMAX - 1, JMAX]
    pairs = [(a, j) for a in EDGE for j in js]
    pairs += [(rng.randrange(1 << 256), rng.randrange(1 << 21)) for _ in range(2000)]
    pairs += [(rng.randrange(1 << 256), JMAX) for _ in range(200)]
    # operands whose product sits just below / above a multiple of n: the quotient estimate's worst cases
    for _ in range(300):
        j = rng.randrange(1, 1 << 21)
        q = rng.randrange(1, j)
        for delta in (-1, 0, 1):
            a = (q * N + j - 1) // j + delta
            if 0 <= a <= TOP:
                pairs.append((a, j))
    got = harness([f"muls {a:x} {j}" for a, j in pairs])
    assert got == [a * j % N for a, j in pairs]


def test_chain_of_small_multiplications(harness):
    """the running value u j^k over many steps stays canonical"""
    rng = random.Random(2)
    cases = [(N - 1, JMAX, 5000), (TOP, JMAX, 1000), (rng.randrange(N), 3, 4000), (rng.randrange(N), 1 << 20, 4000)]
    got = harness([f"chain {a:x} {j} {r}" for a, j, r in cases])
    assert got == [a * pow(j, r, N) % N for a, j, r in cases]


def test_lazy_sum_at_the_kernels_extremes(harness):
    rng = random.Random(3)
    cases = []
    for vals in ([TOP] * 4, [N - 1] * 4, [0] * 4, [TOP, 0, N - 1, 1], [rng.randrange(1 << 256) for _ in range(4)]):
        for lanes, reps in ((64, 4 * 1024), (64, 1), (1, 1), (37, 513)):
            cases.append((lanes, reps, vals))
    got = harness([f"lazy {lanes} {reps} " + " ".join(f"{v:x}" for v in vals) for lanes, reps, vals in cases])
    assert got == [sum(vals) * lanes * reps % N for lanes, reps, vals in cases]


def test_cut_and_join_are_inverse(harness):
    rng = random.Random(4)
    vals = EDGE + [rng.randrange(1 << 256) for _ in range(200)] + [(1 << (26 * i)) - 1 for i in range(1, 10)] + \
        [1 << (26 * i) for i in range(1, 10)]
    assert harness([f"split {v:x}" for v in vals]) == [v % N for v in vals]
