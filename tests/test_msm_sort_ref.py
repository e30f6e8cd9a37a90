"""The restatement of the MSM sort front end (tests/msm_sort_ref.py) against itself, without a GPU: the recodings
reconstruct their scalars at the digit boundaries, a simulated view of every kind of plan passes the checker, and
every mutation of a valid view is rejected AT THE STAGE it belongs to - a checker that cannot fail would make
tests/test_gpu_msm_sort.py worthless."""
import random

import numpy as np
import pytest

from tests import msm_sort_ref as ref

ELL, BN_N = ref.ELL, ref.BN_N


def test_the_orders_are_the_oracles():
    from oracle import bn256_ref, ed25519_ref
    assert ELL == ed25519_ref.ELL and BN_N == bn256_ref.N


def edge_scalars(order, c):
    return [(1 << (c - 1)) - 1, 1 << (c - 1), (1 << 252) - 1, 0, 1, order - 1, (1 << 240) - 1, 1 << 240]


@pytest.mark.parametrize("order", [ELL, BN_N], ids=["ed25519", "bn256"])
@pytest.mark.parametrize("c", [4, 5, 6, 11, 13, 16, 20])
def test_recode_reconstructs_the_scalar(order, c):
    bits = 253 if order == ELL else 256
    W = (bits + 2 + c - 1) // c
    rng = random.Random(c)
    vals = edge_scalars(order, c) + [rng.randrange(order) for _ in range(20)]
    many = ref.recode_many(vals, c, W)
    for k, s in enumerate(vals):
        d = ref.recode(s, c, W, order)
        assert sum(v << (c * w) for w, v in enumerate(d)) == s
        assert all(-(1 << (c - 1)) <= v < (1 << (c - 1)) for v in d) and d[-1] >= 0
        assert list(many[:, k]) == d
    assert ref.recode((1 << (c - 1)) - 1, c, W, order)[:2] == [(1 << (c - 1)) - 1, 0]
    assert ref.recode(1 << (c - 1), c, W, order)[:2] == [-(1 << (c - 1)), 1]          # first negative digit, carry


@pytest.mark.parametrize("order", [ELL, BN_N], ids=["ed25519", "bn256"])
def test_recode_wide_reconstructs_the_scalar_mod_the_order(order):
    rng = random.Random(20)
    vals = edge_scalars(order, 20) + [rng.randrange(order) for _ in range(20)] + [rng.randrange(1 << 240, order)
                                                                                  for _ in range(20)]
    ks = set()
    for s in vals:
        for i in (0, 1, 5, 8191, 8192, (1 << 22) - 8193):
            d = ref.recode_wide(s, i, order)            # (asserts k <= 120, the digit ranges and the congruence itself)
            k = ref.wide_k(s, i, order)
            ks.add(k)
            assert sum(v << (20 * r) for r, v in enumerate(d)) == s + k * order
            if s < (1 << 240) or order != ELL:
                assert k == 0 and d == ref.recode(s, 20, 13, order)
    assert len(ks) > 3 if order == ELL else ks == {0}     # k follows the column, under the Ed25519 order only


# ---- plans of every kind, at reduced size ---------------------------------------------------------------------------
def rand_scalars(rng, n, order, c):
    edge = [0, 1, order - 1, 1 << 252, (1 << 252) - 1, (1 << (c - 1)) - 1, 1 << (c - 1)]
    edge = [v for v in edge if v < order]
    x = [rng.randrange(order) for _ in range(n)]
    for k, v in enumerate(edge[:n]):
        x[(k * 7919) % n] = v
    return x


def case(kind):
    """(plan, expected digits) of one reduced-size plan of the kind"""
    rng = random.Random(sum(kind.encode()))
    if kind in ("msm", "msm_c16", "msm_seg64", "msm_small_cap"):
        c = 16 if kind == "msm_c16" else 11
        p = ref.make_msm_plan(200, 3, ELL, c, 253, seg_shift_min=0 if kind == "msm_seg64" else -3)
        x = rand_scalars(rng, 200, ELL, c)
        x[:70] = [5 + (1 << c)] * 70                   # a heavy bucket in window 0
        if kind == "msm_small_cap":
            p["fine_cap"] = 60
        return p, ref.expected_digits("msm", p, [(x, rand_scalars(rng, 3, ELL, c))])
    if kind.startswith("rows"):
        rows, K = {"rows1": (1, 1), "rows2": (2, 1), "rows4x3": (4, 3), "rows16": (16, 1)}[kind]
        stride, period = 304, 16 // rows
        top = (15, ref.top_max_bucket(ELL, 16, 16)) if rows == 1 else (-1, 0)
        p = ref.plan_geometry(rows * stride, 16, K * period, period, top[0], top[1])
        com = [([77 + 5 * k] * 40 + rand_scalars(rng, 83, ELL, 16), rand_scalars(rng, 3, ELL, 16)) for k in range(K)]
        return p, ref.expected_digits("rows", p, com, table_n=300, rows=rows, windows=16)
    if kind == "wide":
        p = ref.plan_geometry(13 * 8192, 20, 3, 1, wide=1, row_stride=8192)
        com = [(rand_scalars(rng, 50, ELL, 20) + [300001 * (1 + (1 << 20) + (1 << 40))] * 40,
                rand_scalars(rng, 2, ELL, 20)) for _ in range(3)]
        return p, ref.expected_digits("wide", p, com, table_n=90)
    if kind == "bn_msm":
        p = ref.make_msm_plan(300, 0, BN_N, 6, 256, seg_shift_min=0)
        return p, ref.expected_digits("msm", p, [([9] * 70 + rand_scalars(rng, 230, BN_N, 6), [])], BN_N)
    assert kind == "bn_table"
    p = ref.plan_geometry(17 * 40, 16, 1, scalar_bits=256)
    return p, ref.expected_digits("rows", p, [(rand_scalars(rng, 40, BN_N, 16), [])], BN_N, table_n=40, rows=17,
                                  windows=17)


KINDS = ["msm", "msm_c16", "msm_seg64", "msm_small_cap", "rows1", "rows2", "rows4x3", "rows16", "wide", "bn_msm",
         "bn_table"]


@pytest.fixture(scope="module")
def views():
    out = {}
    for kind in KINDS:
        p, D = case(kind)
        out[kind] = (p, D, ref.simulate_view(p, D, np.random.default_rng(len(kind))))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_simulated_view_passes(views, kind):
    p, D, A = views[kind]
    e = ref.check_view(p, A, D)
    assert e.total == np.count_nonzero(D) and len(A["tasks"]) <= p["t_max"]
    if kind == "msm_c16":
        assert p["LB_top"] < p["LB"] and e.unreachable.any()
    if kind == "msm_small_cap":
        assert A["ctrl"][3] >= 1
    if kind in ("msm_seg64", "bn_msm"):
        assert e.seg == 64 and A["ctrl"][0] >= 1          # 70 entries: two segments
    if kind == "bn_msm":
        assert p["balanced"] == 0 and {e.counts[9] - 64, 64} <= set(A["tasks"][A["tasks"][:, 3] == 1][:, 1])
    if kind == "rows1":
        assert p["top_row"] == 15 and p["period"] == 16
    if kind == "rows4x3":
        assert p["W"] == 12 and p["period"] == 4


def mutate(views, kind, fn):
    p, D, A = views[kind]
    A = {k: v.copy() for k, v in A.items()}
    p = dict(p)
    e = ref.Expect(p, D)
    D2 = fn(p, A, e)
    with pytest.raises(ref.StageError) as ei:
        ref.check_view(p, A, D if D2 is None else D2)
    return ei.value


def two_buckets(e):
    """positions in `sorted` of the first entries of two different non-empty buckets"""
    full = np.nonzero(e.counts)[0]
    return int(e.starts[full[0]]), int(e.starts[full[-1]])


def test_a_digit_flipped_in_sign_fails_at_recode(views):
    def fn(p, A, e):
        w, i = np.argwhere(A["digits"] != 0)[3]
        A["digits"][w, i] = -A["digits"][w, i]
    for kind in ("msm", "wide"):
        assert mutate(views, kind, fn).stage == "recode"


def test_entries_swapped_between_buckets_fail_at_the_fine_sort(views):
    def fn(p, A, e):
        a, b = two_buckets(e)
        A["sorted"][[a, b]] = A["sorted"][[b, a]]
    assert mutate(views, "msm", fn).stage == "fine sort"


def test_an_entry_duplicated_over_another_fails_at_the_fine_sort(views):
    def fn(p, A, e):
        heavy = int(np.argmax(e.counts))
        A["sorted"][e.starts[heavy]] = A["sorted"][e.starts[heavy] + 1]
    assert mutate(views, "msm", fn).stage == "fine sort"


def test_starts_off_by_one_fails_at_counts_starts(views):
    def fn(p, A, e):
        A["starts"][np.nonzero(e.counts)[0][5]] += 1
    assert mutate(views, "rows4x3", fn).stage == "counts / starts"


def test_wide_position_left_as_the_bare_column_fails_at_the_fine_sort(views):
    def fn(p, A, e):
        k = int(np.nonzero((A["sorted"] & 0x7fffffff) >= p["row_stride"])[0][0])
        A["sorted"][k] = (A["sorted"][k] & 0x80000000) | ((A["sorted"][k] & 0x7fffffff) % p["row_stride"])
    assert mutate(views, "wide", fn).stage == "fine sort"


def test_count_in_an_unreachable_top_row_bucket_fails_at_counts_starts(views):
    def fn(p, A, e):
        A["counts"][np.nonzero(e.unreachable)[0][0]] = 1
    err = mutate(views, "msm_c16", fn)
    assert err.stage == "counts / starts" and "unreachable" in str(err)


def test_a_task_one_entry_longer_fails_at_plan_pass_2(views):
    def fn(p, A, e):
        A["tasks"][len(A["tasks"]) // 2, 1] += 1
    for kind in ("msm", "bn_msm"):
        assert mutate(views, kind, fn).stage == "plan, pass 2"


def test_tasks_of_different_classes_exchanged_fail_at_plan_pass_2(views):
    def fn(p, A, e):
        t = A["tasks"]
        assert t[0, 1] > t[-1, 1]                       # longest class first
        t[[0, -1]] = t[[-1, 0]]
    for kind in ("msm", "msm_seg64", "bn_msm", "wide"):
        err = mutate(views, kind, fn)
        assert err.stage == "plan, pass 2" and "task order" in str(err)


def test_ctrl3_off_by_one_fails_at_plan_pass_1(views):
    def fn(p, A, e):
        A["ctrl"][3] += 1
    for kind in ("msm", "msm_small_cap"):
        err = mutate(views, kind, fn)
        assert err.stage == "plan, pass 1" and "ctrl[3]" in str(err)


def test_more_tasks_than_t_max_fail_at_plan_pass_2(views):
    def fn(p, A, e):
        A["ctrl"][1] = p["t_max"] + 1
    assert mutate(views, "msm", fn).stage == "plan, pass 2"

    def fn2(p, A, e):                                   # the table is as the segments demand, the buffer is too small
        p["t_max"] = int(A["ctrl"][1]) - 1
    err = mutate(views, "msm", fn2)
    assert err.stage == "plan, pass 2" and "t_max" in str(err)


def test_other_stage_outputs_are_checked_too(views):
    """what no listed mutation touches: the scanned histogram, nseg, heavy_list, seg_starts, split flags"""
    def hist(p, A, e):
        A["hist1"][3] += 1
    assert mutate(views, "rows2", hist).stage == "hist / scan"

    def nseg(p, A, e):
        A["nseg"][np.argmax(e.counts)] += 1
    assert mutate(views, "msm", nseg).stage == "plan, pass 1"

    def heavy(p, A, e):
        A["heavy_list"][0] += 1
    assert mutate(views, "msm", heavy).stage == "plan, pass 1"

    def segs(p, A, e):
        A["seg_starts"][e.split[0]] += 1
    assert mutate(views, "msm", segs).stage == "plan, pass 1"

    def dest(p, A, e):
        A["tasks"][0, 2] += 1
    assert mutate(views, "msm", dest).stage == "plan, pass 2"
