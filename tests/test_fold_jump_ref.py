"""tests/fold_jump_ref.py against plain integers (no GPU, no library): the signed digits of a scalar reconstruct it and
stay in range with no carry out of the top position; the schedule holds every non-zero digit once, by |digit|
descending, with its closing entry; the restated walk - running sum, steps down, S shares, Horner - gives
sum_b s_b e[j + b m_out] mod l for every (rows, digit width) pair, k = 1..6 and every scalar pattern of
tests/test_gpu_fold_jump.py; the geometry rules give the table of shapes that file asserts on the GPU."""
import random

import pytest

from tests import fold_jump_ref as ref

ELL = ref.ELL
PAIRS = [(1, 8), (2, 8), (4, 8), (8, 8), (16, 8), (1, 4), (2, 4), (4, 4), (8, 4)]   # (rows, knob); 16 rows: always 4-bit


def all_pattern_scalars():
    rng = random.Random(1)
    seen = set(ref.EDGE_SCALARS + ref.LEVEL_SCALARS + [0, 1, 2, 127, 128, 129, 255, 256, 7, 8, 9, 15, 16, ELL - 1])
    for bits in (8, 4):
        for k in (1, 6):
            for _, sc in ref.patterns(k, bits, rng):
                seen.update(sc)
    return sorted(seen) + [rng.randrange(ELL) for _ in range(300)]


@pytest.mark.parametrize("bits", [8, 4])
def test_digits_reconstruct_in_range_without_top_carry(bits):
    half = 1 << (bits - 1)
    for s in all_pattern_scalars():
        digits, carry = ref.recode(s, bits)
        assert len(digits) == 256 // bits
        assert sum(d << (bits * p) for p, d in enumerate(digits)) + (carry << 256) == s, hex(s)
        assert all(-half <= d <= half for d in digits), hex(s)
        assert carry == 0, hex(s)


@pytest.mark.parametrize("bits", [8, 4])
def test_recoding_reaches_its_edges(bits):
    """the patterns put digits at -half, half - 1 and -(half - 1), and a carry into every position but the lowest"""
    half, seen, carried = 1 << (bits - 1), set(), set()
    for s in ref.EDGE_SCALARS:
        digits, _ = ref.recode(s, bits)
        seen.update(digits)
        raw = [(s >> (bits * p)) & (2 * half - 1) for p in range(256 // bits)]
        carried.update(p for p in range(256 // bits) if digits[p] % (2 * half) != raw[p])
    assert {-half, half - 1, -(half - 1), -1} <= seen
    assert carried >= set(range(1, 256 // bits))


def test_a_scalar_of_l_or_more_is_refused():
    geo = ref.geometry(4, 64, 2)
    for bad in (ELL, ELL + 1, (1 << 256) - 1):
        assert ref.schedule(geo, 4, [1, bad, 2, 3]) is None
    assert ref.schedule(geo, 4, [1, ELL - 1, 2, 3]) is not None


def check_schedule(geo, rows, scalars, sched):
    O, bits = geo["O"], geo["digit_bits"]
    assert sched.shape == (O, geo["e1"])
    got = {}
    for o in range(O):
        cnt = int(sched[o, 0])
        assert cnt <= geo["e1"] - 2 and not sched[o, 1 + cnt:].any()          # the closing entry and the unused tail
        ents = [int(e) for e in sched[o, 1:1 + cnt]]
        levels = [(e >> 16) & 0xff for e in ents]
        assert levels == sorted(levels, reverse=True) and all(levels)
        for e in ents:
            b, row, d = e & 0xff, (e >> 8) & 0x1f, ((e >> 16) & 0xff) * (-1 if (e >> 15) & 1 else 1)
            assert e >> 24 == 0 and (e >> 13) & 3 == 0 and row < rows and (b, row * O + o) not in got
            got[b, row * O + o] = d
    for b, s in enumerate(scalars):
        digits = [got.get((b, p), 0) for p in range(geo["n_digits"])]
        assert sum(d << (bits * p) for p, d in enumerate(digits)) == s


@pytest.mark.parametrize("rows,knob", PAIRS)
def test_walk_gives_the_fold_for_every_pattern(rows, knob):
    rng = random.Random(rows * 10 + knob)
    for k in range(1, 7):
        m_out = 2 if k < 6 else 1
        geo = ref.geometry(rows, m_out << k, k, knob)
        assert geo["digit_bits"] == (8 if rows <= 8 and knob == 8 else 4) and geo["O"] * rows * geo["digit_bits"] == 256
        exps = [rng.randrange(1, ELL) for _ in range(m_out << k)]
        for name, scalars in ref.patterns(k, geo["digit_bits"], rng):
            sched = ref.schedule(geo, rows, scalars)
            check_schedule(geo, rows, scalars, sched)
            assert ref.walk(geo, rows, sched, exps) == ref.fold_exponents(scalars, exps, m_out), (k, name)
        dup = ref.dup_opposite(exps, m_out, k, [0])
        for scalars in ref.dup_opposite_scalars(k, rng):
            sched = ref.schedule(geo, rows, scalars)
            assert ref.walk(geo, rows, sched, dup) == ref.fold_exponents(scalars, dup, m_out), k


def test_patterns_leave_offsets_and_shares_empty_and_fill_one_level():
    rng = random.Random(3)
    geo = ref.geometry(8, 1024, 4)                    # O = 4, S = 16, 128 entries per offset at most
    by_name = {}
    for name, scalars in ref.patterns(4, 8, rng):
        by_name.setdefault(name, []).append(ref.schedule(geo, 8, scalars))
    assert not by_name["zero"][0].any()
    for sched in by_name["onehot"]:                   # one entry in offset 0 alone: 15 of its 16 shares stay empty
        assert [int(c) for c in sched[:, 0]] == [1, 0, 0, 0] and int(sched[0, 1]) >> 16 == 1
    for sched in by_name["powers"]:                   # 16 positions: every (row, offset) of them once, level 1
        assert int(sched[:, 0].sum()) == 16 and all(int(e) >> 16 == 1 for o in range(4) for e in sched[o, 1:1 + int(sched[o, 0])])
    full = by_name["level"][0]                        # every digit 1: all rows * 2^k entries of an offset on one level
    assert [int(c) for c in full[:, 0]] == [128] * 4 and {int(e) >> 16 for e in full[:, 1:129].ravel()} == {1}
    geo4 = ref.geometry(16, 1024, 2)                  # 4-bit: the same scalar leaves the odd offsets empty
    sched4 = ref.schedule(geo4, 16, [ref.LEVEL_SCALARS[0]] * 4)
    assert [int(c) for c in sched4[:, 0]] == [64, 0, 64, 0]


def test_geometry_of_the_gpu_shapes():
    """the table of the GPU file: digit width, O, S, m_out and n_blocks of every shape it runs"""
    for (rows, k, n_cols, knob), want in ref.SHAPES.items():
        g = ref.geometry(rows, n_cols, k, knob)
        assert (g["digit_bits"], g["O"], g["S"], g["m_out"], g["n_blocks"]) == want, (rows, k, n_cols, knob)
        assert g["grid_x"] % 8 == 0 and 0 <= g["grid_x"] - g["n_blocks"] < 8 and g["grid_y"] == g["S"]
        assert g["m_out"] * g["O"] * g["S"] <= 1 << 17 or g["S"] == 1             # the lane cap
        assert g["S"] == 1 or rows * (1 << k) // g["S"] >= 8                      # at least 8 entries a share


def test_share_count_rules():
    # entries rule alone (one output): S = rows 2^k / 8, capped at 16
    assert [ref.geometry(8, 1 << k, k)["S"] for k in range(1, 7)] == [2, 4, 8, 16, 16, 16]
    assert [ref.geometry(1, 1 << k, k)["S"] for k in range(1, 7)] == [1, 1, 1, 2, 4, 8]
    # lane cap alone (rows 2^k = 1024): m_out O S <= 2^17, O = 4
    assert [ref.geometry(16, m << 6, 6)["S"] for m in (2048, 4096, 8192, 16384, 32768, 65536)] == [16, 8, 4, 2, 1, 1]
