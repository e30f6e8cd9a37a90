"""CPU check of csrc/qap_mtree_plan.h - the geometry of the moment transform's subproduct tree (s, L, d', the offset of
every level's T nodes, of D^-1 and of the build's scalars, the total, the caller's scratch) and the bound on the integer
coefficients the tree asks the NTT to rebuild - against the restatement in tests/moments_tree_ref.py.

The header is plain C++; this test builds it with g++ (AddressSanitizer and UndefinedBehaviorSanitizer) into
tests/native/qap_mtree_plan_host_test.cpp, a program of its own."""
import os
import subprocess

import pytest

from tests import moments_tree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "qap_mtree_plan_host_test.cpp")
DS = list(range(1, 1026)) + [(1 << 20) - 1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "qap_mtree_plan_host_test")
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
        return out
    return run


def test_the_headers_own_invariants_and_the_coefficient_bound(harness):
    """levels tile the buffer, d' >= d, d' - d < 2^L, s <= S_MAX, s > S_MAX / 2 whenever L > 0, and 2^(512 + ceil(log2
    d')) stays below the product of the 18 primes of csrc/ntt31_consts.h, for every d in 1..1025 and 2^20 - 1"""
    verdict, m_bits = harness(["check"])[0].rsplit(" ", 1)
    assert verdict == "ok"
    assert int(m_bits) == 551                     # csrc/ntt31.h: the primes' product has 551 bits


def test_sizes_agree_with_the_restatement(harness):
    cases = [(d, n_max) for d in DS for n_max in (1, d, 2 * d)]
    got = harness(["plan %d %d" % c for c in cases])
    for (d, n_max), line in zip(cases, got):
        s, L, dp = R.geometry(d)
        levels, dinv, tmp, total = R.plan_scalars(d, n_max)
        bits = 512 + (dp - 1).bit_length()
        want = [s, L, dp] + [levels[l] for l in range(L + 1)] + [dinv, tmp, total, R.scratch_scalars(d, 3), bits]
        assert [int(x) for x in line.split()] == want, (d, n_max)
        assert dp << 512 <= 1 << bits <= 1 << 532


def test_unknown_requests_are_refused(harness):
    assert harness(["plam 1 1"]) == ["inval"]
