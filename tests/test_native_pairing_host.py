"""CPU check of csrc/bn256_pairing.h (the BN-256 tower, Miller loop and final exponentiation).

The header is `__host__ __device__`; this test builds it with g++ (AddressSanitizer and UndefinedBehaviorSanitizer)
into tests/native/pairing_host_test.cpp and compares every operation with the Python restatement
(tests/bn256_pairing_ref.py) on random and edge-case operands, so that arithmetic bugs are caught before GPU time
is spent.  Miller-loop values are compared up to a factor in Fp6 (the two use different line scalings, which the
final exponentiation removes); everything else exactly."""
import os
import random
import subprocess

import pytest

from tests import bn256_pairing_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairing_host_test.cpp")
P = R.P


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "pairing_host_test")
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
        return [tuple(int(v, 16) for v in o.split()) for o in out]
    return run


def hx(vals):
    return " ".join(format(v, "x") for v in vals)


# Fp6 in the harness order (x.re, x.im, y.re, y.im, z.re, z.im) of x tau^2 + y tau + z  <->  the restatement's
# w-polynomial (tau = w^2): z w^0, y w^2, x w^4
def f6_to_poly(v):
    x, y, z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    return (z, (0, 0), y, (0, 0), x, (0, 0))


def poly_to_f6(c):
    assert c[1] == c[3] == c[5] == (0, 0)
    return (*c[4], *c[2], *c[0])


EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2]


def rand12(rng, edge=False):
    pick = (lambda: rng.choice(EDGE)) if edge else (lambda: rng.randrange(P))
    return tuple(pick() for _ in range(12))


def test_fp6_ops(harness):
    rng = random.Random(61)
    cases = [tuple(rng.randrange(P) for _ in range(6)) for _ in range(20)] + \
            [tuple(rng.choice(EDGE) for _ in range(6)) for _ in range(10)] + [(0, 0, 0, 0, 1, 0), (1, 0, 0, 0, 0, 0)]
    lines, want = [], []
    for a in cases:
        b = tuple(rng.randrange(P) for _ in range(6))
        pa, pb = f6_to_poly(a), f6_to_poly(b)
        lines += [f"f6mul {hx(a)} {hx(b)}", f"f6sqr {hx(a)}"]
        want += [poly_to_f6(R.f12_mul(pa, pb)), poly_to_f6(R.f12_mul(pa, pa))]
        if any(a):
            lines.append(f"f6inv {hx(a)}")
            want.append(poly_to_f6(R.f12_inv(pa)))
    assert harness(lines) == want


def test_fp12_ops(harness):
    rng = random.Random(121)
    cases = [rand12(rng) for _ in range(12)] + [rand12(rng, edge=True) for _ in range(6)] + [R.GT_ONE]
    lines, want = [], []
    for a in cases:
        b = rand12(rng)
        pa, pb = R.from_gt(a), R.from_gt(b)
        lines += [f"f12mul {hx(a)} {hx(b)}", f"f12sqr {hx(a)}", f"f12conj {hx(a)}", f"f12frob {hx(a)}",
                  f"f12frob2 {hx(a)}", f"f12isone {hx(a)}"]
        want += [R.to_gt(R.f12_mul(pa, pb)), R.to_gt(R.f12_mul(pa, pa)), R.to_gt(R.f12_frob(pa, 6)),
                 R.to_gt(R.f12_frob(pa)), R.to_gt(R.f12_frob(pa, 2)), (1 if a == R.GT_ONE else 0,)]
        if any(a):
            lines.append(f"f12inv {hx(a)}")
            want.append(R.to_gt(R.f12_inv(pa)))
    assert harness(lines) == want


def _pts(rng):
    a, b = rng.randrange(1, R.N), rng.randrange(1, R.N)
    return R.E1.mul(a, R.G1), R.E2.mul(b, R.G2)


def _pt_hex(p, q):
    return hx(p) + " " + hx((*q[0], *q[1]))


def test_miller_loop_matches_up_to_fp6(harness):
    rng = random.Random(5)
    pairs = [(R.G1, R.G2), _pts(rng)]
    got = harness([f"miller {_pt_hex(p, q)}" for p, q in pairs])
    for (p, q), m in zip(pairs, got):
        ref = R.miller(p, q)
        ratio = R.f12_mul(R.from_gt(m), R.f12_inv(ref))
        assert ratio[1] == ratio[3] == ratio[5] == (0, 0), "Miller values differ by more than an Fp6 factor"


def test_final_exponentiation(harness):
    rng = random.Random(9)
    vals = [rand12(rng), R.to_gt(R.miller(R.G1, R.G2))]
    got = harness([f"finalexp {hx(v)}" for v in vals])
    assert got == [R.to_gt(R.final_exp(R.from_gt(v))) for v in vals]


def test_pairing_and_infinity(harness):
    rng = random.Random(11)
    pairs = [(R.G1, R.G2), _pts(rng)]
    lines = [f"pairing {_pt_hex(p, q)}" for p, q in pairs]
    lines += ["pairing 0 0 " + hx((*R.G2[0], *R.G2[1])), "pairing " + hx(R.G1) + " 0 0 0 0"]
    want = [R.pairing(p, q) for p, q in pairs] + [R.GT_ONE, R.GT_ONE]
    assert harness(lines) == want
