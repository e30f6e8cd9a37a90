"""CPU check of the GF(l) instantiation of csrc/ntt31.h's reconstruction, the last step of the Protocol 8 extension's
NTT route (csrc/circuit_sat.hip): tests/native/ntt31_fr_host_test.cpp (a program of its own, built
here with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run directly) holds against unsigned __int128 and
its own limb arithmetic, with l = 2^252 + 27742317777372353535851937790883648493 restated there:
fr_mul_small at a in {0, 1, l - 1, random} x j in {0, 1, 2^31 - 1, each of the 18 primes} and at random pairs (a seventh
of them just below l); Garner plus the GF(l) Horner on the residues of 0, l, l^2, 2^20 (l - 1)^2 (which the primes'
product exceeds) and of random 18-tuples of digits; and on every one of those tuples that the GF(n) instantiation -
under its old names and as the template - still gives the value mod n."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ntt31_fr_host_test.cpp")

GROUPS = ("fr mul small", "crt fixed", "crt largest", "crt random")


def test_ntt31_gf_l_against_limb_arithmetic(tmp_path):
    exe = str(tmp_path / "ntt31_fr_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    res = subprocess.run([exe], text=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert lines == [g + " ok" for g in GROUPS], res.stdout
