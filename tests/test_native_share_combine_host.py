"""CPU check of csrc/share_combine.h, the per-element step of vmpc_bn256_fr_share_combine_dev: the header is
`__host__ __device__`; tests/native/share_combine_host_test.cpp (a program of its own, built here with g++ under
AddressSanitizer and UndefinedBehaviorSanitizer and run directly) holds it against plain limb arithmetic through
unsigned __int128 at 1, 3, 4 and 64 parties with every operand n - 1 - four products of n - 1 are the first sum that
a 16-limb accumulator loses - with and without an addend, on random operands and on a part that is not canonical."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "share_combine_host_test.cpp")


def test_worst_case_sums_need_513_bits():
    """the premise, in Python ints"""
    n = 65000549695646603732796438742359905742570406053903786389881062969044166799969
    assert (3 * (n - 1) ** 2).bit_length() == 512 and (4 * (n - 1) ** 2).bit_length() == 513


def test_combine_element_against_limb_arithmetic(tmp_path):
    exe = str(tmp_path / "share_combine_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    res = subprocess.run([exe], text=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == 4 * 6 and all(ln.endswith(" ok") for ln in lines), res.stdout
    for parties in (1, 3, 4, 64):
        assert f"worst parties={parties} ok" in lines
