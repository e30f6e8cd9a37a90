"""CPU check of the bucket loop's field and point forms (csrc/fe25519.h fe_mul_cols, csrc/ge25519.h ge_madd_cols and
ge_ext_from_niels_neg): the headers are `__host__ __device__`, and the host branch of fe_mul_cols is the plain C
statement of the column order the device issues as multiply-adds with a carry-in.
tests/native/fe_cols_host_test.cpp (a program of its own, built here with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer and run directly) holds fe_mul_cols<1..4> against fe_mul limb for limb - reduced operands,
the corners of fe_mul's operand contract with every limb maximal and with random limbs, zero operands - the column
form of the mixed addition against ge_madd limb for limb, and the first-entry formulas against ge_madd(identity, +-q)
as affine points."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fe_cols_host_test.cpp")


def test_column_products_and_first_entry_against_fe_mul_and_ge_madd(tmp_path):
    exe = str(tmp_path / "fe_cols_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    res = subprocess.run([exe], text=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert lines == ["reduced 2000 ok", "bounds_maximal 5 ok", "bounds_random 2000 ok", "zero 2 ok",
                     "first_entry 48 ok", "madd_chain 96 ok"], res.stdout
