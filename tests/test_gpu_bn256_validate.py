"""gk_validate (csrc/bn256_impl.h, through vmpc_bn256_validate_dev) against a predicate on Python integers: an encoding
is good iff every residue is below P and either all residues are zero or y^2 = x^3 + b holds (tests/bn256_encodings.py,
over oracle/bn256_ref.py).  The expected count of offenders is always the predicate's, never the library's.

The rows are those of bn256_encodings.table: valid points; canonical points off the curve (each residue bent in turn,
the twist's imaginary parts included); residues r + P, which are other bytes for a valid point; P in the place of 0,
which is other bytes for the point at infinity and must not be taken for it; 2^256 - 1 and the values that decide the
comparison with P in each 32-bit word; and a twist point with a zero residue, with P written there - the one encoding
whose curve equation holds and which only the comparison's answer at P itself refuses.  The count is checked exactly: over the whole table, row by row, over batches
around the 256-lane block with offenders at chosen lanes, over a batch in which every lane fails for another reason,
and over the reversed table.

NOT covered: subgroup membership of twist points.  The twist's cofactor is not 1; neither the reference nor this gate
checks membership, and a point of the twist outside G2 counts as good here.

24 tests; with tests/test_gpu_bn256_gates.py 54 tests in 6 s on an MI355X, most of it context and fixture setup.  Each of
these value-only mutations of the library makes tests of this file fail (those of the gates are listed there):
  1. Fp29x2Ops::raw_canonical looks at its first residue only: test_count_over_the_whole_table[2],
     test_each_row_alone[2], test_a_batch_of_offenders_only[2].
  2. gk_validate asks raw_canonical of x only: test_count_over_the_whole_table, test_each_row_alone and
     test_a_batch_of_offenders_only in both groups, test_offenders_at_chosen_lanes[1-513].
  3. gk_validate stores 1 in place of its atomicAdd: test_count_over_the_whole_table, test_a_batch_of_offenders_only and
     test_an_empty_batch in both groups, test_offenders_at_chosen_lanes at every n but 1.
  4. fp_raw_is_canonical answers true on equality: test_count_over_the_whole_table[2], test_each_row_alone[2],
     test_a_batch_of_offenders_only[2] - through the twist point with a zero residue alone; in G1 the curve equation
     refuses every encoding that holds P, so there it is tests/test_native_bn_canonical_host.py (both tests) that fails.
  5. BN256Point.from_bytes reduces mod P, 6. mpc_koe._received_side without its validation: none here."""
import itertools

import numpy as np
import pytest

from tests import bn256_encodings as enc

pytestmark = pytest.mark.gpu
GROUPS = [1, 2]
SIZES = [1, 255, 256, 257, 513]


@pytest.fixture(scope="module")
def ctx():
    import verifiable_mpc_amd as v
    return v.get_context()


def as_array(group, rows):
    vals = [r.vals if isinstance(r, enc.Row) else r for r in rows]
    return np.frombuffer(b"".join(enc.encode(v) for v in vals), np.uint8).reshape(len(vals), enc.WIDTH[group]).copy()


def count(ctx, group, rows):
    arr = as_array(group, rows)
    return ctx.bn256_validate(group, ctx.upload(arr).ptr, len(arr))


@pytest.mark.parametrize("group", GROUPS)
def test_count_over_the_whole_table(ctx, group):
    rows = enc.table(group)
    want = enc.count_bad(group, rows)
    assert want == len(rows) - len(enc.rows_of(group, "good")) and want >= 50
    assert count(ctx, group, rows) == want
    assert count(ctx, group, rows[::-1]) == want
    assert count(ctx, group, enc.rows_of(group, "good")) == 0


@pytest.mark.parametrize("group", GROUPS)
def test_each_row_alone(ctx, group):
    wrong = []
    for row in enc.table(group):
        want = 0 if enc.is_good(group, row.vals) else 1
        got = count(ctx, group, [row])
        if got != want:
            wrong.append((row.cls, row.name, got, want))
    assert not wrong, wrong


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group", GROUPS)
def test_offenders_at_chosen_lanes(ctx, group, n):
    """good points everywhere but at k of the lanes 0, n - 1, 255, 256 (those that exist), for every choice of them: the
    count is k - one atomicAdd per offender, across the edge of the 256-lane block"""
    good, bad = enc.rows_of(group, "good"), enc.bad_rows(group)
    lanes = sorted({p for p in (0, n - 1, 255, 256) if p < n})
    base = [good[i % len(good)].vals for i in range(n)]
    seen, pick = set(), 0
    for k in range(len(lanes) + 1):
        for chosen in itertools.combinations(lanes, k):
            rows = list(base)
            for lane in chosen:
                rows[lane] = bad[pick % len(bad)].vals
                pick += 1
            assert enc.count_bad(group, rows) == k
            assert count(ctx, group, rows) == k, (n, chosen)
            seen.add(k)
    assert seen == set(range(len(lanes) + 1))


@pytest.mark.parametrize("group", GROUPS)
def test_a_batch_of_offenders_only(ctx, group):
    """257 lanes, each bad row in turn: the lanes of a wave disagree about why they fail, and every one is counted"""
    bad = enc.bad_rows(group)
    rows = [bad[i % len(bad)].vals for i in range(257)]
    assert enc.count_bad(group, rows) == 257
    assert count(ctx, group, rows) == 257
    assert count(ctx, group, rows[::-1]) == 257
    for cls in ("off", "alias", "inf-alias", "other"):                  # and every lane for the SAME reason
        same = enc.rows_of(group, cls)
        rows = [same[i % len(same)].vals for i in range(257)]
        assert count(ctx, group, rows) == 257, cls


@pytest.mark.parametrize("group", GROUPS)
def test_an_empty_batch(ctx, group):
    assert ctx.bn256_validate(group, None, 0) == 0
    assert count(ctx, group, enc.bad_rows(group)[:3]) == 3               # and the counter starts from zero again
    assert ctx.bn256_validate(group, None, 0) == 0
