"""CPU check of csrc/r1cs_share.h, the per-element steps of vmpc_bn256_r1cs_share_mul_deal_dev and
vmpc_bn256_r1cs_share_finish_dev: the header is `__host__ __device__`; tests/native/r1cs_share_host_test.cpp (a program
of its own, built here with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run directly) holds what a
party deals against d + sum_k coeffs[k-1] x^k in plain limb arithmetic through unsigned __int128 and the finished wire
against its defining equation - for 1, 3, 4 and 64 parties, degrees 0, 1 and parties - 1, random operands and every
operand n - 1, empty V and Y dots, inverse coefficients 1 and full size, and a non-canonical part (reported, nothing
stored)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "r1cs_share_host_test.cpp")


def test_share_steps_against_limb_arithmetic(tmp_path):
    exe = str(tmp_path / "r1cs_share_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    res = subprocess.run([exe], text=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    degrees = {1: (0,), 3: (0, 1, 2), 4: (0, 1, 3), 64: (0, 1, 63)}
    want = []
    for parties, ts in degrees.items():
        want += [f"deal {name} P={parties} t={t} ok" for t in ts for name in ("random", "worst", "unit", "empty-v")]
        want += [f"finish {name} P={parties} t=0 ok" for name in ("random", "worst", "inv-1", "empty-y", "empty-y-inv-1",
                                                                  "noncanonical-part")]
    assert sorted(lines) == sorted(want), res.stdout
