"""CPU check of the comparison with p behind the BN-256 point validation: fp_raw_is_canonical (csrc/sw256.h) through
Fp1Ops / Fp2Ops and Fp29Ops / Fp29x2Ops ::raw_canonical (csrc/fp29.h), the first thing gk_validate asks of an encoding.

Built with g++ under AddressSanitizer and UndefinedBehaviorSanitizer (tests/native/bn_canonical_host_test.cpp) and
compared with `v < P` on Python integers.  p is a full 256-bit number, so canonical and non-canonical values share the
top bit and uniform data decides the word-by-word comparison in the top word; the values of
tests/bn256_encodings.word_boundary_values push the decision into each of the eight words in turn, from either side."""
import os
import subprocess

import pytest

from tests import bn256_encodings as enc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "bn_canonical_host_test.cpp")
P = enc.P


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "bn_canonical_host_test")
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
        return [tuple(int(v) for v in o.split()) for o in out]
    return run


def test_one_residue(harness):
    vals = enc.probe_values()
    assert P in vals and P - 1 in vals and P + 1 in vals
    got = harness([f"one {v:x}" for v in vals])
    wrong = [(hex(v), g) for v, g in zip(vals, got) if g != (int(v < P),) * 2]
    assert not wrong, wrong[:8]


def test_a_pair_of_residues(harness):
    """F_p2: both residues must be canonical - every combination of a canonical and a non-canonical value, both orders"""
    vals = enc.probe_values(n_random=20, seed=512)
    low, high = [v for v in vals if v < P], [v for v in vals if v >= P]
    assert len(low) >= 12 and len(high) >= 12
    pairs = [(a, b) for a in low for b in high] + [(b, a) for a in low for b in high]
    pairs += [(low[i], low[-1 - i]) for i in range(len(low))] + [(high[i], high[-1 - i]) for i in range(len(high))]
    got = harness([f"two {a:x} {b:x}" for a, b in pairs])
    wrong = [(hex(a), hex(b), g) for (a, b), g in zip(pairs, got) if g != (int(a < P and b < P),) * 2]
    assert not wrong, wrong[:8]
    assert {g for g in got} == {(0, 0), (1, 1)}
