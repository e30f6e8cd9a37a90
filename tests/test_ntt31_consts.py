"""csrc/ntt31_consts.h is what scripts/make_ntt31_consts.py writes, byte for byte; the primes follow their rule (the 18
largest c * 2^22 + 1 below 2^31); 18 of them hold every coefficient a product at the cap can have and 17 do not; the
Python-side constants of the NTT are the header's."""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "make_ntt31_consts.py")
HEADER = os.path.join(ROOT, "verifiable_mpc_amd", "csrc", "ntt31_consts.h")

ISSUE_PRIMES = [2130706433, 2113929217, 2088763393, 2025848833, 2013265921, 1866465281, 1811939329, 1790967809,
                1711276033, 1572864001, 1484783617, 1438646273, 1321205761, 1300234241, 1224736769, 1212153857,
                1161822209, 1107296257]


def _script():
    spec = importlib.util.spec_from_file_location("make_ntt31_consts", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_the_committed_header(tmp_path):
    out = tmp_path / "ntt31_consts.h"
    subprocess.check_call([sys.executable, SCRIPT, str(out)])
    assert out.read_bytes() == open(HEADER, "rb").read()


def test_prime_rule():
    gen = _script()
    ps = gen.primes()
    assert ps == ISSUE_PRIMES
    # by trial division, independent of the script's Miller-Rabin: these are ALL the primes c 2^22 + 1 in [p_18, 2^31)
    def is_prime(n):
        return n > 1 and all(n % q for q in range(2, int(n ** 0.5) + 1))
    want = [p for p in range((1 << 31) - (1 << 22) + 1, ps[-1] - 1, -(1 << 22)) if is_prime(p)]
    assert want == ps
    for p in ps:
        w = gen.root_of_unity(p)
        assert pow(w, 1 << 22, p) == 1 and pow(w, 1 << 21, p) == p - 1


def test_eighteen_primes_suffice_and_seventeen_do_not():
    gen = _script()
    assert gen.bound_facts() == (True, False)
    ps = gen.primes()
    bound = (1 << 20) * ((1 << 256) - 1) ** 2
    m = 1
    for p in ps:
        m *= p
    assert m.bit_length() == 551 and bound < (1 << 532) < m
    assert m // ps[-1] < bound            # even dropping the SMALLEST prime leaves too little


def test_python_constants_are_the_headers():
    from verifiable_mpc_amd import _native
    text = open(os.path.join(ROOT, "include", "vmpc.h")).read()

    def macro(name):
        m = re.search(r"#define %s (.+)" % name, text)
        return eval(m.group(1).replace("(size_t)", ""))
    assert _native.BN256_FR_NTT_MIN == macro("VMPC_BN256_FR_NTT_MIN")
    assert _native.BN256_FR_NTT_LDS_LEN == macro("VMPC_BN256_FR_NTT_LDS_LEN")
    assert (_native.POLY_PRODUCT_SCHOOLBOOK, _native.POLY_PRODUCT_AUTO, _native.POLY_PRODUCT_NTT) == \
        (macro("VMPC_POLY_PRODUCT_SCHOOLBOOK"), macro("VMPC_POLY_PRODUCT_AUTO"), macro("VMPC_POLY_PRODUCT_NTT"))
