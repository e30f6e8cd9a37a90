"""CPU check of csrc/ntt31.h, the arithmetic of the multi-prime NTT's kernels (csrc/bn256_ntt.hip): the header is
`__host__ __device__`; tests/native/ntt31_host_test.cpp (a program of its own, built here with g++ under
AddressSanitizer and UndefinedBehaviorSanitizer and run directly) holds against unsigned __int128 and its own limb
arithmetic: the Montgomery product at 0, 1, p - 1, 2p - 1 and random operands for all 18 primes, the 256-bit reduction
on 0, n - 1, n, 2^256 - 1 and random values, a length-8 and a length-64 transform (forward against the definition at
the bit-reversed index, then back) through the header's butterflies, Garner plus Horner on 0, on the largest admissible
coefficient 2^20 (2^256 - 1)^2, on all digits p_i - 1 and on random values, and frbn_mul_small by a 31-bit word."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ntt31_host_test.cpp")

GROUPS = ("montgomery", "reduce256", "transform 8", "transform 64", "crt zero", "crt largest", "crt all-top-digits",
          "crt random", "prefix products", "mul word")


def test_ntt31_against_limb_arithmetic(tmp_path):
    exe = str(tmp_path / "ntt31_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    res = subprocess.run([exe], text=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert lines == [g + " ok" for g in GROUPS], res.stdout
