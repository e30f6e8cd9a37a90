"""A plain restatement of the fold jump's host plan (csrc/fold_jump_plan.h) and, in the exponent domain, of the walk
its kernels do over that plan (csrc/fold_jump.hip).

Plan: `geometry` (digit width, n_digits, O, e1, the share count S, n_blocks and the grid), `recode` (signed digits with
carry) and `schedule` (per offset the non-zero digits by |digit| descending, in the library's entry encoding, with the
closing entry).  tests/test_native_fold_jump_plan_host.py compares all three word for word with the header.

Walk: table row r of column i holds 2^(256 r / rows) e_i (as an exponent of the base point); a lane (j, o, share)
walks the schedule of offset o with a running sum `run` and an outer accumulator `acc` - run += +-entry for the
entries dealt to its share (entry e to share e mod S), and at every step down in |digit| (the closing entry's
included) acc += run once per level - and the recombination sums the S shares of an offset and joins the offsets by
Horner with digit_bits doublings a step.  k_fold_jump (4-bit digits, acc parked in memory) and k_fold_jump8 (8-bit digits) are the same walk
with another start level and |digit| mask; `walk` takes both from the geometry.  The result must be
sum_b s_b e[j + b m_out] mod l for every output j (tests/test_fold_jump_ref.py).

`patterns` are the scalar sets the CPU and the GPU tests share."""
import numpy as np

ELL = (1 << 252) + 27742317777372353535851937790883648493
FJ_WAVES = 4


def geometry(rows, n_cols, k, knob=8):
    """knob: 8, or 4 for a context created under VMPC_FOLD_JUMP_DIGITS=4"""
    assert rows in (1, 2, 4, 8, 16) and 1 <= k <= 6 and n_cols >= 1 << k and n_cols & (n_cols - 1) == 0
    m_out = n_cols >> k
    digit_bits = 8 if rows <= 8 and knob != 4 else 4
    n_digits = 256 // digit_bits
    O, B = n_digits // rows, 1 << k
    S = 1
    while S < 16 and m_out * O * S * 2 <= 1 << 17 and rows * B // (S * 2) >= 8:
        S *= 2
    n_blocks = (m_out + 63) // 64 * (O // FJ_WAVES)
    return {"digit_bits": digit_bits, "n_digits": n_digits, "O": O, "e1": rows * B + 2, "S": S, "n_blocks": n_blocks,
            "grid_x": (n_blocks + 7) // 8 * 8, "grid_y": S, "m_out": m_out, "sched_words": O * (rows * B + 2)}


def recode(s, digit_bits):
    """(digits, carry out of the top position): digits in [-half, half), least significant first"""
    assert 0 <= s < 1 << 256
    half, n_digits = 1 << (digit_bits - 1), 256 // digit_bits
    digits, carry = [], 0
    for p in range(n_digits):
        raw = ((s >> (digit_bits * p)) & (2 * half - 1)) + carry
        carry = 1 if raw >= half else 0
        digits.append(raw - 2 * half * carry)
    return digits, carry


def schedule(geo, rows, scalars):
    """uint32 [O, e1]: word 0 the number of entries, then the entries (bits 0..7 = b, 8..12 = row, 15 = negate,
    16..23 = |digit|) by |digit| descending - b ascending, then position ascending, within a level - and a closing 0.
    None when a scalar is not below l."""
    O, half = geo["O"], 1 << (geo["digit_bits"] - 1)
    if any(not 0 <= s < ELL for s in scalars):
        return None
    levels = [[[] for _ in range(half + 1)] for _ in range(O)]
    for b, s in enumerate(scalars):
        digits, carry = recode(s, geo["digit_bits"])
        assert carry == 0
        for p, d in enumerate(digits):
            if d:
                levels[p % O][abs(d)].append(b | (p // O) << 8 | (1 << 15 if d < 0 else 0) | abs(d) << 16)
    sched = np.zeros((O, geo["e1"]), np.uint32)
    for o in range(O):
        ents = [e for v in range(half, 0, -1) for e in levels[o][v]]
        sched[o, 0] = len(ents)
        sched[o, 1:1 + len(ents)] = ents
    return sched


def walk_offset(geo, sched_o, col):
    """what the S lanes (j, o, share) leave in their slots; col(row, b) = the exponent of table entry
    (row, j + b m_out).  All S lanes read the same entries and step down at the same places, so one pass serves them
    all: entry e belongs to share e % S, a step down is taken by every share that has added an entry."""
    S, half = geo["S"], 1 << (geo["digit_bits"] - 1)
    mask = 0xff if geo["digit_bits"] == 8 else 0xffff         # k_fold_jump reads ent >> 16 whole
    cnt = int(sched_o[0])
    run, acc, have, cur = [0] * S, [0] * S, [False] * S, half
    for e in range(cnt + 1):
        ent = int(sched_o[1 + e])
        v = (ent >> 16) & mask
        if cur > v:                      # entries of |digit| >= cur are all in run: it counts once per level
            for sh in range(S):
                if have[sh]:
                    acc[sh] = (acc[sh] + (cur - v) * run[sh]) % ELL
            cur = v
        if e == cnt:                     # the closing entry (|digit| = 0) has brought every level down to 1 in
            break
        sh = e % S
        q = col((ent >> 8) & 0x1f, ent & 0xff)
        run[sh] = (run[sh] + (-q if (ent >> 15) & 1 else q)) % ELL
        have[sh] = True
    return acc


def walk(geo, rows, sched, exps):
    """the m_out outputs (exponents) of the fold over columns with exponents `exps` (n_cols of them)"""
    m_out, O = geo["m_out"], geo["O"]
    shift = 256 // rows
    out = []
    for j in range(m_out):
        def col(row, b):
            return (exps[j + b * m_out] << (shift * row)) % ELL
        acc = 0
        for o in range(O - 1, -1, -1):
            if o != O - 1:
                for _ in range(geo["digit_bits"]):
                    acc = 2 * acc % ELL
            for slot in walk_offset(geo, sched[o], col):
                acc = (acc + slot) % ELL
        out.append(acc)
    return out


def fold_exponents(scalars, exps, m_out):
    """sum_b s_b e[j + b m_out] mod l"""
    return [sum(s * exps[j + b * m_out] for b, s in enumerate(scalars)) % ELL for j in range(m_out)]


def le(bs):
    return int.from_bytes(bytes(bs), "little")


# digit edges: the byte patterns of test_fixed_base_comb_matches_oracle (raw 8-bit digits at +-128 / +-127 and a carry
# through every position), nibble patterns for the 4-bit recoding (raw 8 / 7 and 7 + carry) under a top byte that
# keeps the scalar below l, and the values around l and 2^252
EDGE_SCALARS = [le([0x80] * 31 + [0x0f]), le([0x7f] * 31 + [0x0f]), le([0x81] * 31 + [0x0f]), le([0xff] * 31 + [0x0f]),
                le([0x88] * 31 + [0x08]), le([0x77] * 31 + [0x07]), le([0x78] * 31 + [0x07]),
                ELL - 1, ELL - 2, (ELL - 1) // 2, 1 << 252, (1 << 252) - 1]
# every digit 1 in the 8-bit form (4-bit: every other position - the odd offsets stay empty); every 4-bit digit 1 but
# the top one (8-bit: 17 everywhere but the top)
LEVEL_SCALARS = [le([0x01] * 32), le([0x11] * 31 + [0x01])]


def patterns(k, digit_bits, rng, names=None):
    """[(name, [2^k scalars])]: every call of a pattern (a pattern that needs more scalars than 2^k takes several)"""
    B, n_digits = 1 << k, 256 // digit_bits
    out = [("random", [rng.randrange(ELL) for _ in range(B)]), ("zero", [0] * B)]
    for b in sorted({0, B // 2, B - 1}):
        out.append(("onehot", [1 if i == b else 0 for i in range(B)]))
    for p0 in range(0, n_digits, B):     # one scalar per digit position (2^(digit_bits * 63) = 2^252 < l)
        out.append(("powers", [1 << (digit_bits * ((p0 + i) % n_digits)) for i in range(B)]))
    for i0 in range(0, len(EDGE_SCALARS), B):
        out.append(("edges", [EDGE_SCALARS[(i0 + i) % len(EDGE_SCALARS)] for i in range(B)]))
    for s in LEVEL_SCALARS:
        out.append(("level", [s] * B))
    return [(n, s) for n, s in out if names is None or n in names]


def dup_opposite(exps, m_out, k, js):
    """exps with e[j + m_out] = e[j] and (k >= 2) e[j + 2 m_out] = l - e[j] for j in js: with s_0 = s_1 `run` doubles
    (an addition of a point to itself), with s_0 = s_2 it passes through the neutral element"""
    exps = list(exps)
    for j in js:
        exps[j + m_out] = exps[j]
        if k >= 2:
            exps[j + 2 * m_out] = ELL - exps[j]
    return exps


def dup_opposite_scalars(k, rng):
    B = 1 << k
    return [[1] * B, [1 if b % 2 == 0 else 0 for b in range(B)], [rng.randrange(ELL) for _ in range(B)]]


# (rows, k, n_cols, knob) -> (digit_bits, O, S, m_out, n_blocks): the shapes of tests/test_gpu_fold_jump.py and the
# path each takes, computed from the code as it stood when the file was written
SHAPES = {
    (1, 1, 256, 8): (8, 32, 1, 128, 16),       # remap with per_xcd = 2, 8 offset groups, 2-entry schedules
    (1, 6, 64, 8): (8, 32, 8, 1, 8),           # one output, partial wave
    (2, 3, 512, 8): (8, 16, 2, 64, 4),         # first shared schedule
    (4, 3, 1024, 8): (8, 8, 4, 128, 4),        # two output groups x two offset groups
    (8, 3, 512, 8): (8, 4, 8, 64, 1),
    (8, 4, 1024, 8): (8, 4, 16, 64, 1),        # entries rule at its end
    (8, 4, 1 << 15, 8): (8, 4, 16, 2048, 32),  # lane cap, last size inside it
    (8, 4, 1 << 16, 8): (8, 4, 8, 4096, 64),   # lane cap, first size beyond it
    (16, 1, 256, 8): (4, 4, 4, 128, 2),        # 4-bit kernel, more than one group
    (16, 2, 1024, 8): (4, 4, 8, 256, 4),
    (16, 3, 1 << 14, 8): (4, 4, 16, 2048, 32),  # lane cap, 4-bit
    (16, 3, 1 << 15, 8): (4, 4, 8, 4096, 64),
    (16, 6, 64, 8): (4, 4, 16, 1, 1),          # 1024-entry schedule, one output
    (1, 2, 512, 4): (4, 64, 1, 128, 32),       # k_fold_jump with more than one offset group
    (2, 3, 512, 4): (4, 32, 2, 64, 8),
    (4, 3, 1024, 4): (4, 16, 4, 128, 8),
    (8, 4, 1024, 4): (4, 8, 16, 64, 2),
}
