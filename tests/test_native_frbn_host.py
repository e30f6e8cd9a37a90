"""CPU check of csrc/fr256.h as csrc/fr_bn.h instantiates it (GF(n) for the BN-256 group order n, and the wide
accumulator of the polynomial product) and, for the accumulator and the inverse, as csrc/fr.h does (GF(l), l the
Ed25519 order).

The header is `__host__ __device__`; this test builds it with g++ (AddressSanitizer and UndefinedBehaviorSanitizer)
into tests/native/frbn_host_test.cpp and compares every operation with Python integers, on random operands and on the
edge operands 0, 1, n-1, n, n+1 and 2^256-1 (n fills all 256 bits, so sums carry out of 256 bits and loads of values
>= n are one subtraction), so that arithmetic bugs are caught before GPU time is spent."""
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "frbn_host_test.cpp")
N = 65000549695646603732796438742359905742570406053903786389881062969044166799969
L = (1 << 252) + 27742317777372353535851937790883648493
TOP = (1 << 256) - 1
EDGE = [0, 1, N - 1, N, N + 1, TOP]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "frbn_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])

    def run(lines, field="frbn"):
        res = subprocess.run([exe, field], input="\n".join(lines) + "\nquit\n", text=True, capture_output=True,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                      UBSAN_OPTIONS="print_stacktrace=1"))
        assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
            res.stderr[-2000:]
        out = res.stdout.strip().split("\n")
        assert len(out) == len(lines), (len(out), len(lines))
        return [int(o, 16) for o in out]
    return run


def hx(*vals):
    return " ".join(format(v, "x") for v in vals)


def operand_pairs(rng, n_random=200):
    pairs = list(itertools.product(EDGE, EDGE))
    pairs += [(rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(n_random)]
    pairs += [(rng.choice(EDGE), rng.randrange(1 << 256)) for _ in range(40)]
    pairs += [(N - 1 - rng.randrange(4), N - 1 - rng.randrange(4)) for _ in range(20)]
    return pairs


def test_load_reduces_any_256_bit_value(harness):
    rng = random.Random(1)
    vals = EDGE + [N + 2, TOP - 1, 2 * N - (1 << 256)] + [rng.randrange(N, 1 << 256) for _ in range(50)] + \
        [rng.randrange(N) for _ in range(50)]
    assert harness([f"load {hx(v)}" for v in vals]) == [v % N for v in vals]


def test_add_sub_mul(harness):
    rng = random.Random(2)
    lines, want = [], []
    for a, b in operand_pairs(rng):
        lines += [f"add {hx(a, b)}", f"sub {hx(a, b)}", f"mul {hx(a, b)}"]
        want += [(a + b) % N, (a - b) % N, (a * b) % N]
    assert harness(lines) == want


def test_accumulator_sums_of_products(harness):
    rng = random.Random(3)
    lines, want = [], []
    for k in (0, 1, 2, 3, 17, 64):
        for pick in (lambda: rng.randrange(1 << 256), lambda: rng.choice(EDGE)):
            ops = [(pick(), pick()) for _ in range(k)]
            lines.append(f"mac {k} " + " ".join(hx(a, b) for a, b in ops))
            want.append(sum((a % N) * (b % N) for a, b in ops) % N)
    assert harness(lines) == want


def test_accumulator_beyond_544_bits(harness):
    """2^16 and more products of the largest operands: the sum passes 16 and then 17 limbs (the row carries pass 2^32)"""
    lines, want = [], []
    for r in (1, 65535, 65536, 65537, 200000):
        lines += [f"macrep {r} {hx(N - 1, N - 1)}", f"macraw {r} {hx(TOP, TOP)}", f"macraw {r} {hx(TOP, 1)}"]
        want += [r * (N - 1) * (N - 1) % N, r * TOP * TOP % N, r * TOP % N]
    assert harness(lines) == want


# ---- GF(l): the same header under csrc/fr.h's parameters.  fr_load copies, so add / sub / mul / inv take residues
# below l; the accumulator takes any limbs ----
def test_gf_l_add_sub_mul(harness):
    rng = random.Random(4)
    edge = [0, 1, 2, L - 2, L - 1]
    pairs = list(itertools.product(edge, edge)) + [(rng.randrange(L), rng.randrange(L)) for _ in range(200)]
    lines, want = [], []
    for a, b in pairs:
        lines += [f"add {hx(a, b)}", f"sub {hx(a, b)}", f"mul {hx(a, b)}"]
        want += [(a + b) % L, (a - b) % L, (a * b) % L]
    assert harness(lines, "fr") == want


def test_gf_l_accumulator_sums_of_products(harness):
    rng = random.Random(5)
    edge = [0, 1, L - 1, L, L + 1, TOP]
    lines, want = [], []
    for k in (0, 1, 2, 3, 17, 64):
        for pick in (lambda: rng.randrange(1 << 256), lambda: rng.choice(edge), lambda: rng.randrange(L)):
            ops = [(pick(), pick()) for _ in range(k)]
            lines.append(f"mac {k} " + " ".join(hx(a, b) for a, b in ops))
            want.append(sum(a * b for a, b in ops) % L)
    assert harness(lines, "fr") == want


def test_gf_l_accumulator_beyond_544_bits(harness):
    """as test_accumulator_beyond_544_bits: the row carries pass 2^32 and the sum passes 17 limbs"""
    lines, want = [], []
    for r in (1, 65535, 65536, 65537, 200000):
        lines += [f"macrep {r} {hx(L - 1, L - 1)}", f"macraw {r} {hx(TOP, TOP)}", f"macraw {r} {hx(TOP, 1)}"]
        want += [r * (L - 1) * (L - 1) % L, r * TOP * TOP % L, r * TOP % L]
    assert harness(lines, "fr") == want


@pytest.mark.parametrize("field,m", [("fr", L), ("frbn", N)])
def test_inverse(harness, field, m):
    rng = random.Random(6)
    vals = [0, 1, 2, m - 2, m - 1] + [rng.randrange(m) for _ in range(60)]
    got = harness([f"inv {hx(v)}" for v in vals], field)
    assert got == [pow(v, m - 2, m) for v in vals]
    assert got[0] == 0 and got[1] == 1 and got[4] == m - 1
    assert all(g * v % m == 1 for g, v in zip(got[1:], vals[1:]))
