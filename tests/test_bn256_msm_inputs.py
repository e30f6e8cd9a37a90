"""CPU checks of the BN-256 MSM edge inputs (tests/bn256_msm_inputs.py): the planner's widths, the recoding's
extreme digits and the bucket loads that tests/test_gpu_bn256_edges.py relies on."""
import random

import pytest

from oracle import bn256_ref as bn
from tests import bn256_msm_inputs as mi

N = bn.N


def test_plan_every_width():
    """msm_make_plan with the override c: W = ceil(258 / c), and c = 4 is widened to (5, 52) because W <= 64"""
    want = {4: (5, 52), 5: (5, 52), 6: (6, 43), 7: (7, 37), 8: (8, 33), 9: (9, 29), 10: (10, 26), 11: (11, 24),
            12: (12, 22), 13: (13, 20), 14: (14, 19), 15: (15, 18), 16: (16, 17)}
    for c in range(4, 17):
        assert mi.make_plan(1000, c) == want[c], c


def test_planner_natural_widths():
    """the sizes at which test_gpu_bn256_edges runs each width the planner picks by itself"""
    for n, c in ((1 << 11, 9), (1 << 14, 11), (1 << 15, 12), (1 << 16, 13), (1 << 19, 15)):
        assert mi.make_plan(n)[0] == c, n


def test_recode_reconstructs_and_matches_closed_form():
    rng = random.Random(5)
    cases = [0, 1, N - 1, N - 2, 2**255, (1 << 254) - 1] + [rng.randrange(N) for _ in range(200)]
    for c in range(4, 17):
        cc, W = mi.make_plan(0, c)
        half = 1 << (cc - 1)
        for s in cases:
            d = mi.recode(s, cc, W)
            assert sum(v << (cc * w) for w, v in enumerate(d)) == s
            assert all(-half <= v < half for v in d)
            # the carry into window k is what the digits below it leave over: s mod 2^(ck) - sum_{w<k} d_w 2^(cw)
            for k in range(1, W):
                low = s & ((1 << (cc * k)) - 1)
                left = (low - sum(v << (cc * w) for w, v in enumerate(d[:k]))) >> (cc * k)
                assert mi.carry_into(s, cc, k) == left
        assert mi.recode(N, cc, W) == [0] * W           # non-canonical: counts as zero


@pytest.mark.parametrize("c", range(5, 17))
def test_extreme_scalar_hits_last_bucket_everywhere(c):
    cc, W = mi.make_plan(0, c)
    assert cc == c
    e = mi.extreme(c)
    assert 0 < e < N
    d = mi.recode(e, c, W)
    assert d[:W - 1] == [-(1 << (c - 1))] * (W - 1)      # bucket index nb = 2^(c-1) in every lower window
    assert d[W - 1] == 1


@pytest.mark.parametrize("c", range(5, 17))
def test_n_minus_1_reaches_the_largest_top_digit(c):
    """The top digit is raw_top(s) + carry(s mod 2^(c(W-1))), and the carry is monotone in the lower part (closed
    form above).  A scalar with a smaller raw top window has top digit <= raw_top(N-1) - 1 + 1; one with the same
    raw top window has a lower part <= N-1's.  So N - 1 has the largest top digit of all canonical scalars - and
    that digit never exceeds what the planner allows for (msm_top_max_bucket: bucket index raw + carry - 1 <= raw)."""
    _, W = mi.make_plan(0, c)
    sh = c * (W - 1)
    top = mi.recode(N - 1, c, W)[W - 1]
    raw = (N - 1) >> sh
    carry = mi.carry_into(N - 1, c, W - 1)
    assert top == raw + carry
    assert top - 1 <= mi.top_max_bucket(c, W)
    assert top < 1 << (c - 1)
    # monotone carry: for the lower parts just below and above N-1's, and random ones
    lo = (N - 1) & ((1 << sh) - 1)
    rng = random.Random(c)
    for t in [0, lo, max(lo - 1, 0)] + [rng.randrange(1 << sh) for _ in range(50)]:
        if t <= lo:
            assert mi.carry_into(t, c, W - 1) <= carry
        s = (raw << sh) | t
        if s < N:
            assert mi.recode(s, c, W)[W - 1] <= top
    for s in [rng.randrange(N) for _ in range(300)]:
        assert mi.recode(s, c, W)[W - 1] <= top
    assert (carry == 1) == (c in (6, 7, 8, 9, 10, 12, 14, 16))


def test_heavy_cases_need_the_workgroup_tree():
    """every heavy scalar vector of test_gpu_bn256_edges puts > MSM_FINISH_SERIAL * 1024 entries into one bucket, so
    gk_finish's tree runs whatever segment length (at most 64 << 4 entries) the plan picks"""
    n = 1 << 16
    limit = mi.FINISH_SERIAL * mi.MAX_SEG_LEN
    c, W = mi.make_plan(n)
    for name, sc in mi.skewed_vectors(n, c, 11).items():
        if name in mi.HEAVY:
            assert max(mi.bucket_counts(sc, c, W).values()) > limit, name
    for name, sc in mi.skewed_vectors(n, mi.TABLE_C, 12).items():
        if name in mi.HEAVY:
            assert max(mi.bucket_counts(sc, mi.TABLE_C, mi.TABLE_W, rows=mi.TABLE_W).values()) > limit, name


def test_wire_like_shape():
    sc = mi.wire_like(1 << 14, 3)
    frac = lambda f: sum(1 for s in sc if f(s)) / len(sc)
    assert abs(frac(lambda s: s == 0) - 0.54) < 0.02
    assert abs(frac(lambda s: s in (1, 2)) - 0.09) < 0.01
    assert abs(frac(lambda s: s == N - 1) - 0.05) < 0.01
    assert all(0 <= s < N for s in sc)


def test_reduce_forms():
    """both gk_reduce forms are reachable by the edge tests: the c = 16 table takes SPLIT = 2, small widths and the
    six-key pass SPLIT = 1, and so do c = 10, 11 on the variable-base path"""
    assert mi.reduce_split(mi.TABLE_C, 1) == 2
    assert mi.reduce_split(mi.TABLE_C, 1, K=6) == 1
    assert mi.reduce_split(*mi.make_plan(0, 5)) == 1
    assert mi.reduce_split(*mi.make_plan(0, 8)) == 1
    assert mi.reduce_split(*mi.make_plan(0, 11)) == 2
    assert mi.reduce_split(*mi.make_plan(0, 13)) == 1
