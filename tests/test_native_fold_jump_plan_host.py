"""CPU check of csrc/fold_jump_plan.h - the digit width, the geometry (n_digits, O, e1, the share count S, n_blocks,
the grid), the signed-digit recoding and the per-offset schedule that table_fold() (csrc/fold_jump.hip) hands to its
kernels - against the restatement in tests/fold_jump_ref.py.

The header is plain C++; this test builds it with g++ (AddressSanitizer and UndefinedBehaviorSanitizer) into
tests/native/fold_jump_plan_host_test.cpp, a program of its own, and compares what it prints word for word with the
restatement on the shapes and the scalar patterns of tests/test_gpu_fold_jump.py, for every (rows, digit width) pair
and k = 1..6.  A scalar that is not below l, and arguments table_fold() refuses, are reported as such."""
import os
import random
import subprocess

import pytest

from tests import fold_jump_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fold_jump_plan_host_test.cpp")
ELL = ref.ELL
PAIRS = [(1, 8), (2, 8), (4, 8), (8, 8), (16, 8), (1, 4), (2, 4), (4, 4), (8, 4)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "fold_jump_plan_host_test")
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


def request(rows, n_cols, k, knob, scalars):
    return "plan %d %d %d %d %s" % (rows, n_cols, k, knob, " ".join(format(s, "x") for s in scalars))


def expected(rows, n_cols, k, knob, scalars):
    g = ref.geometry(rows, n_cols, k, knob)
    sched = ref.schedule(g, rows, scalars)
    if sched is None:
        return "noncanon"
    head = [g[f] for f in ("digit_bits", "n_digits", "O", "e1", "S", "n_blocks", "grid_x", "m_out", "sched_words")]
    return " ".join([str(v) for v in head] + [format(int(w), "x") for w in sched.ravel()])


def compare(harness, cases):
    got = harness([request(*c) for c in cases])
    for c, g in zip(cases, got):
        want = expected(*c)
        if g != want:       # name the first word that differs, not two 1000-word lines
            gw, ww = g.split(), want.split()
            at = next((i for i, (a, b) in enumerate(zip(gw, ww)) if a != b), min(len(gw), len(ww)))
            raise AssertionError("rows=%d n_cols=%d k=%d knob=%d: word %d is %s, the restatement has %s (%d / %d words)"
                                 % (c[0], c[1], c[2], c[3], at, gw[at:at + 1], ww[at:at + 1], len(gw), len(ww)))


@pytest.mark.parametrize("rows,knob", PAIRS)
def test_schedule_of_every_pattern_word_for_word(harness, rows, knob):
    rng = random.Random(100 * rows + knob)
    cases = []
    for k in range(1, 7):
        bits = 8 if rows <= 8 and knob == 8 else 4
        for _, scalars in ref.patterns(k, bits, rng):
            cases.append((rows, 64 << k, k, knob, scalars))
        for scalars in ref.dup_opposite_scalars(k, rng):
            cases.append((rows, 64 << k, k, knob, scalars))
    compare(harness, cases)


def test_geometry_of_the_gpu_shapes_and_of_the_share_rules(harness):
    rng = random.Random(7)
    cases = [(rows, n_cols, k, knob, [rng.randrange(ELL) for _ in range(1 << k)])
             for rows, k, n_cols, knob in ref.SHAPES]
    # the lane cap and the entries rule, one step to either side
    for rows in (1, 2, 4, 8, 16):
        for k in range(1, 7):
            for log_m in (0, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16, 17):
                for knob in (8, 4):
                    cases.append((rows, 1 << (log_m + k), k, knob, [rng.randrange(ELL) for _ in range(1 << k)]))
    compare(harness, cases)
    got = harness([request(*c) for c in cases[:len(ref.SHAPES)]])
    for (key, want), line in zip(ref.SHAPES.items(), got):
        w = [int(v) for v in line.split()[:9]]
        assert (w[0], w[2], w[4], w[7], w[5]) == want, key        # digit_bits, O, S, m_out, n_blocks


@pytest.mark.parametrize("bits", [8, 4])
def test_recoding_digit_by_digit(harness, bits):
    rng = random.Random(bits)
    vals = ref.EDGE_SCALARS + ref.LEVEL_SCALARS + [0, 1, 1 << (bits - 1), (1 << (bits - 1)) - 1, (1 << bits) - 1] + \
        [rng.randrange(ELL) for _ in range(100)]
    got = harness(["recode %d %x" % (bits, v) for v in vals])
    for v, line in zip(vals, got):
        assert [int(d) for d in line.split()] == ref.recode(v, bits)[0], hex(v)


def test_noncanonical_scalars_and_bad_arguments_are_refused(harness):
    for bad in (ELL, ELL + 1, 1 << 253, (1 << 256) - 1):
        for pos in (0, 3):
            scalars = [5, 6, 7, 8]
            scalars[pos] = bad
            assert harness([request(4, 64, 2, 8, scalars)]) == ["noncanon"]
            assert expected(4, 64, 2, 8, scalars) == "noncanon"
        assert harness(["recode 8 %x" % bad]) == ["noncanon"]
    assert harness([request(4, 64, 2, 8, [5, 6, 7, ELL - 1])])[0].split()[0] == "8"
    for rows, n_cols, k in ((3, 64, 2), (4, 48, 2), (4, 64, 0), (4, 64, 7), (4, 2, 2), (32, 64, 2), (0, 64, 2)):
        assert harness(["plan %d %d %d 8 1 1 1 1" % (rows, n_cols, k)]) == ["inval"]
