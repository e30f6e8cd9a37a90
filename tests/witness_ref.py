"""A big-int restatement of the R1CS solve (verifiable_mpc_amd/pynocchio.py SolvePlan, csrc/bn256_r1cs_solve.hip,
DESIGN.md section 22), written by the rounds rule as it is stated - every round scans ALL rows not yet placed - so that it
shares nothing with the product's worklist; and a generator of solvable R1CS with prescribed level widths.  The
independent side of tests/test_witness_plan_host.py and tests/test_gpu_witness.py.

An R1CS here is (V, W, Y, m): three lists of d rows, a row a list of (wire, int coefficient) pairs in any order, with
duplicates, negative values and values >= N allowed."""
import random

import numpy as np

from tests import keygen_ref as K

N = K.N
CHECK, KY, KA, KB = 0, 1, 2, 3


def _merged(row):
    out = {}
    for wire, x in row:
        out[wire] = (out.get(wire, 0) + x) % N
    return {w: x for w, x in out.items() if x}


def plan(r1cs, n_in):
    """-> list of levels; a level is a list of (row, kind, new wire or None, coefficient inverse or 0, [a, b, y] as
    {wire: coefficient} without the new wire) in ascending row order"""
    V, W, Y, m = r1cs
    d = len(V)
    if n_in > m:
        raise ValueError("more inputs than wires")
    rows = [[_merged(M[j]) for M in (V, W, Y)] for j in range(d)]
    known = set(range(n_in + 1))
    todo = list(range(d))
    levels = []
    while todo:
        level, new, rest = [], {}, []
        for j in todo:
            unknown = sorted({w for mat in rows[j] for w in mat} - known)
            if not unknown:
                level.append((j, CHECK, None, 0, rows[j]))
            elif len(unknown) == 1 and unknown[0] not in new:
                s = unknown[0]
                where = [k for k in range(3) if s in rows[j][k]]
                if len(where) > 1:
                    raise ValueError(f"constraint {j + 1}: wire {s} is not linear")
                new[s] = j
                mats = [dict(mat) for mat in rows[j]]
                coef = mats[where[0]].pop(s)
                level.append((j, (KA, KB, KY)[where[0]], s, pow(coef, -1, N), mats))
            else:
                rest.append(j)
        if not level:
            raise ValueError(f"constraint {rest[0] + 1}: two or more unknown wires")
        levels.append(level)
        known |= set(new)
        todo = rest
    missing = sorted(set(range(m + 1)) - known)
    if missing:
        raise ValueError(f"wire {missing[0]} is never defined")
    return levels


class Failed(Exception):
    """a row failed: .row (0-based), .what ("division" or "check")"""

    def __init__(self, row, what):
        super().__init__(f"{what} at row {row}")
        self.row, self.what = row, what


def solve(r1cs, inputs, levels=None):
    """the witness (ints, c[0] = 1) of one input vector; raises Failed at the first failing row in level order"""
    m = r1cs[3]
    levels = plan(r1cs, len(inputs)) if levels is None else levels
    c = [None] * (m + 1)
    c[0] = 1
    for i, x in enumerate(inputs):
        c[1 + i] = int(x) % N
    dot = lambda mat: sum(x * c[w] for w, x in mat.items()) % N
    for level in levels:
        vals = []
        for j, kind, s, inv, mats in level:
            a, b, y = (dot(mat) for mat in mats)
            if kind == CHECK:
                if a * b % N != y:
                    raise Failed(j, "check")
                continue
            if kind == KY:
                v = (a * b - y) * inv % N
            else:
                div, rest = (b, a) if kind == KA else (a, b)
                if div == 0:
                    raise Failed(j, "division")
                v = (y * pow(div, -1, N) - rest) * inv % N
            vals.append((s, v))
        for s, v in vals:                       # a level reads nothing that it writes
            c[s] = v
    return c


def layered_r1cs(widths, seed, n_in=2, kinds=(KY, KA, KB), checks=0):
    """A solvable R1CS whose plan has exactly the level widths `widths`: every row of level l reads at least one wire
    that level l - 1 defines (level 0: an input), the rows are shuffled, the kinds drawn from `kinds`.  Coefficients are
    small, negative or full size; the divisor side of a KA / KB row is 1 + (a wire) so that random inputs do not hit
    zero.  `checks` extra check rows (k x) (k') = (k k') x over the inputs alone hold for every input; the rounds rule
    places them in level 0, whose width grows by `checks`.  -> (V, W, Y, m)"""
    rng = random.Random(seed)
    coef = lambda: rng.choice([rng.randint(1, 3), -rng.randint(1, 3), rng.randrange(1, N), N + rng.randint(1, 5)])
    rows, prev, older, nxt = [], list(range(1, n_in + 1)), [0], n_in + 1
    for li, width in enumerate(widths):
        cur = []
        for _ in range(width):
            s, nxt = nxt, nxt + 1
            cur.append(s)

            def form(must=None):
                f = [(rng.choice(prev + older), coef()) for _ in range(rng.randint(0, 2))]
                if must is not None:
                    f.append((must, coef()))
                rng.shuffle(f)
                return f
            kind = rng.choice(kinds)
            dep = rng.choice(prev)
            if kind == KY:
                row = (form(dep), form() + [(0, coef())], form() + [(s, coef())])
            else:
                lin = form() + [(s, coef())]
                div = [(0, 1), (dep, coef())]
                num = form()
                row = (lin, div, num) if kind == KA else (div, lin, num)
            rows.append(row)
        older, prev = older + prev, cur
    for i in range(checks):
        x, k1, k2 = 1 + i % n_in, coef(), coef()
        rows.append(([(x, k1)], [(0, k2)], [(x, k1 * k2)]))
    rng.shuffle(rows)
    V, W, Y = ([r[k] for r in rows] for k in range(3))
    return V, W, Y, nxt - 1


def from_dense(case):
    """a case of tests/golden/pinocchio_keygen.json (dense rows) -> (V, W, Y, m)"""
    mats = [[[(w, int(x)) for w, x in enumerate(row) if int(x)] for row in case["r1cs"][k]] for k in "VWY"]
    return mats[0], mats[1], mats[2], case["m"]


def from_csr(built):
    """tests/pinocchio_batch_ref.chain_r1cs's (V, W, Y, n_io, m) -> (V, W, Y, m)"""
    out = []
    for ptr, col, vals in built[:3]:
        out.append([[(col[e], vals[e]) for e in range(ptr[j], ptr[j + 1])] for j in range(len(ptr) - 1)])
    return out[0], out[1], out[2], built[4]


def csr(M):
    """rows of (wire, coefficient) pairs -> the CSR tuple R1CSQAP takes, the coefficients as Python ints (duplicates,
    negative values and values >= N stay as they are: R1CSQAP reduces and adds them)"""
    ptr, col, vals = [0], [], []
    for row in M:
        for w, x in row:
            col.append(w)
            vals.append(x)
        ptr.append(len(col))
    return np.asarray(ptr, np.int64), np.asarray(col, np.int64), vals


def level_widths(levels):
    return [len(level) for level in levels]
