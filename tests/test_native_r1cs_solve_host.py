"""CPU check of csrc/r1cs_solve.h, the per-row step of vmpc_bn256_r1cs_solve_batch_dev (both of its kernels call it):
the header is `__host__ __device__`; tests/native/r1cs_solve_host_test.cpp (a program of its own, built here with g++
under AddressSanitizer and UndefinedBehaviorSanitizer and run directly) holds each kind's stored wire against the row's
defining equation in plain limb arithmetic through unsigned __int128 - on random operands, with every operand n - 1,
on empty dots, on a divisor that cancels to zero (failed, 0 stored), on passing and failing check rows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "r1cs_solve_host_test.cpp")


def test_row_step_against_limb_arithmetic(tmp_path):
    exe = str(tmp_path / "r1cs_solve_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    res = subprocess.run([exe], text=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == 3 * 7 + 4 + 1 and all(ln.endswith(" ok") for ln in lines), res.stdout
    for kind in (1, 2, 3):
        for name in ("random", "unit", "unit-empty-y", "worst", "empty", "zero-divisor", "column>m"):
            assert f"{name} kind={kind} ok" in lines
    for name in ("check-pass", "check-fail", "check-empty", "check-worst"):
        assert f"{name} kind=0 ok" in lines
    assert "prepare ok" in lines
