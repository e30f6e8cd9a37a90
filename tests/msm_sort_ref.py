"""CPU restatement of the MSM sort front end (csrc/msm_sort.hip) and a checker for what it leaves behind.

The front end is exact integer work: recode -> hist1 -> scan -> part1 -> fine / fine_big -> ranks / classes -> plan2.
`expected_digits` restates the recoding and the digit-row layouts, `check_view` compares a view of the device arrays
(Context.msm_sort_view) with what follows from those digits and raises an AssertionError that NAMES the stage,
`simulate_view` builds a valid view on the CPU (so that the checker itself can be tested without a GPU) and
`plan_geometry` restates msm_plan_geometry / msm_layout's t_max for plans made without a device.

numpy and Python ints only."""
import numpy as np

ELL = 2 ** 252 + 27742317777372353535851937790883648493
BN_N = 65000549695646603732796438742359905742570406053903786389881062969044166799969       # the order of BN-256 (oracle/bn256_ref.py N)
MSM_SEG, MSM_SEG_LOG2, MSM_FINISH_SERIAL, SORT_T = 64, 6, 32, 8192
WIDE_C, WIDE_ROWS = 20, 13
SIGN = 0x80000000
STAGES = ("recode", "hist / scan", "counts / starts", "fine sort", "plan, pass 1", "plan, pass 2")


class StageError(AssertionError):
    def __init__(self, stage, what):
        self.stage = stage
        super().__init__(f"[{stage}] {what}")


def _need(cond, stage, what):
    if not cond:
        raise StageError(stage, what() if callable(what) else what)


# ---- recoding -------------------------------------------------------------------------------------------------------
def recode(s, c, W, order):
    """the library's signed digits (msm_recode_term): W digits in [-2^(c-1), 2^(c-1))"""
    assert order is None or s < order
    half, out, carry = 1 << (c - 1), [], 0
    for _ in range(W):
        raw = (s & ((1 << c) - 1)) + carry
        carry = 1 if raw >= half else 0
        out.append(raw - (carry << c))
        s >>= c
    return out


def wide_k(s, i, order=ELL):
    """k_msm_recode_wide: the multiple of l added to the scalar of column i (Ed25519 scalars from 2^240 up)"""
    if order != ELL or s < (1 << 240):
        return 0
    k = ((((i * 2654435761) & 0xffffffff) >> 16) * 121) >> 16
    assert k <= 120
    return k


def recode_wide(s, i, order=ELL):
    """k_msm_recode_wide: thirteen signed 20-bit digits of s + k l, column i choosing k"""
    assert s < order
    d = recode(s + wide_k(s, i, order) * order, WIDE_C, WIDE_ROWS, None)
    assert all(-(1 << 19) <= v < (1 << 19) for v in d[:12]) and 0 <= d[12] < (1 << 19), d
    assert (sum(v << (20 * r) for r, v in enumerate(d)) - s) % order == 0
    return d


def recode_many(values, c, W):
    """recode() of every value at once: int32 [W, n] (values are non-negative Python ints below 2^(c W))"""
    n = len(values)
    nbytes = (c * W + 7) // 8 + 1
    raw = np.frombuffer(b"".join(int(v).to_bytes(nbytes, "little") for v in values), np.uint8).reshape(n, nbytes)
    bits = np.unpackbits(raw, axis=1, bitorder="little")[:, :c * W].reshape(n, W, c).astype(np.int64)
    rawd = (bits << np.arange(c, dtype=np.int64)).sum(axis=2)           # [n, W] unsigned digits
    out = np.empty((W, n), np.int32)
    carry = np.zeros(n, np.int64)
    for w in range(W):
        v = rawd[:, w] + carry
        carry = (v >= (1 << (c - 1))).astype(np.int64)
        out[w] = v - (carry << c)
    assert not carry.any(), "the top digit carries out"
    return out


# ---- plans ----------------------------------------------------------------------------------------------------------
def top_max_bucket(order, c, W):
    return min((order - 1) >> (c * (W - 1)), 0xffffffff) if c * (W - 1) < 256 else 0


def plan_geometry(n_total, c, W, period=None, top_row=-1, top_max_b=0, scalar_bits=253, wide=0, row_stride=0,
                  seg_shift_min=-3, fine_bits=-1, fill_shift=0):
    """msm_plan_geometry and msm_layout's t_max / hist1_n, restated (the fields a view carries)"""
    p = dict(n_total=n_total, c=c, W=W, period=period if period and 0 < period <= W else W, top_row=top_row,
             top_max_b=top_max_b, wide=wide, row_stride=row_stride, chunks_per_row=row_stride // SORT_T if wide else 0)
    nb = p["nb"] = 1 << (c - 1)
    p["nb1"] = nb + 1
    n_pad = p["n_pad"] = (n_total + 7) & ~7
    idx_bits = 1
    while (1 << idx_bits) < n_pad:
        idx_bits += 1
    nc_target = 256 if n_total >= (1 << 22) else 512
    lb = min(c - 1, 9)
    while lb > 0 and (nb >> lb) < nc_target and (n_total >> (c - 1 - lb)) > 8192:
        lb -= 1
    if 0 <= fine_bits <= 9 and fine_bits <= c - 1 and (nb >> fine_bits) <= 4096:
        lb = fine_bits
    p["fine_cap"] = 12288
    if wide:
        lb = 9
        while lb > 6 and (n_total >> (c - 1 - lb)) > 14336:
            lb -= 1
        idx_bits = 1
        while (1 << idx_bits) < row_stride:
            idx_bits += 1
        p["fine_cap"] = 16384
    p["LB"], p["NC"], p["idx_bits"] = lb, nb >> lb, idx_bits
    p["fine_in_entry"] = int(idx_bits + lb <= 31)
    p["LB_top"] = lb
    if top_row >= 0:
        lt = 0
        while lt < lb and (top_max_b >> lt) > p["NC"] - 1:
            lt += 1
        p["LB_top"] = lt
    p["J"] = (n_pad + SORT_T - 1) // SORT_T
    p["balanced"] = int(scalar_bits == 253)
    work = (W * n_total) >> fill_shift
    ss = 0
    while ss < 4 and ((MSM_SEG << ss) << 18) < work:
        ss += 1
    while ss > seg_shift_min and (seg_len(ss - 1) << 18) >= work:
        ss -= 1
    p["seg_shift"] = ss
    p["hist1_n"] = W * p["NC"] * p["J"]
    p["t_max"] = W * n_total // seg_len(ss) + min(W * n_total, W * nb)
    return p


def seg_len(seg_shift):
    return 1 << (MSM_SEG_LOG2 + seg_shift)


def make_msm_plan(n, n_extra, order, c, scalar_bits, **kw):
    """msm_make_plan for a given window width: W, the top row and the bucket its digits stop at"""
    W = (scalar_bits + 2 + c - 1) // c
    assert W <= 64
    return plan_geometry(n + n_extra, c, W, W, W - 1, top_max_bucket(order, c, W), scalar_bits, **kw)


# ---- expected digit rows --------------------------------------------------------------------------------------------
def expected_digits(kind, plan, commitments, order=ELL, table_n=None, rows=None, windows=None):
    """the full [W][n_pad] digit array, zeros of the padding included.  `commitments`: one (scalars, extras) pair of
    lists per commitment of the pass (a plain MSM has one).
      "msm"   row w = window w; main terms at [0, n), extras at [n, n + n_extra)
      "rows"  a `rows`-row table of `windows` digits per scalar, wpr = windows / rows: digit w of column i of
              commitment k at row k * period + w % wpr, position (w / wpr) * stride + i; extras from column table_n
      "wide"  the 13-row wide-window table: row k, digit r of column i at r * row_stride + i"""
    W, n_pad, c = plan["W"], plan["n_pad"], plan["c"]
    out = np.zeros((W, n_pad), np.int32)
    if kind == "msm":
        (sc, ex), = commitments
        assert all(0 <= s < order for s in list(sc) + list(ex))
        out[:, :len(sc) + len(ex)] = recode_many(list(sc) + list(ex), c, W)
        return out
    if kind == "rows":
        wpr, period = windows // rows, plan["period"]
        stride = n_pad // rows
        assert wpr * rows == windows and period == wpr and stride * rows == n_pad and W == len(commitments) * period
        for k, (sc, ex) in enumerate(commitments):
            assert all(0 <= s < order for s in list(sc) + list(ex)) and len(sc) <= table_n
            cols = np.concatenate([np.arange(len(sc)), table_n + np.arange(len(ex))]).astype(np.int64)
            assert cols.size == 0 or cols.max() < stride
            d = recode_many(list(sc) + list(ex), c, windows)
            for w in range(windows):
                out[k * period + w % wpr, (w // wpr) * stride + cols] = d[w]
        return out
    assert kind == "wide" and c == WIDE_C and W == len(commitments)
    rs = plan["row_stride"]
    assert n_pad == WIDE_ROWS * rs
    for k, (sc, ex) in enumerate(commitments):
        cols = [int(i) for i in range(len(sc))] + [table_n + e for e in range(len(ex))]
        vals = list(sc) + list(ex)
        assert all(0 <= s < order for s in vals)
        d = recode_many([s + wide_k(s, i, order) * order for s, i in zip(vals, cols)], WIDE_C, WIDE_ROWS)
        assert (d[12] >= 0).all()
        cols = np.array(cols, np.int64)
        for r in range(WIDE_ROWS):
            out[k, r * rs + cols] = d[r]
    return out


# ---- what follows from the digits -----------------------------------------------------------------------------------
class Expect:
    """everything the stages must produce, from the digit rows and the plan alone"""

    def __init__(self, plan, digits):
        p = self.plan = plan
        W, nb1, NC, J = p["W"], p["nb1"], p["NC"], p["J"]
        D = np.asarray(digits)
        assert D.shape == (W, p["n_pad"])
        row, pos = np.nonzero(D)
        d = D[row, pos].astype(np.int64)
        mag = np.abs(d)
        assert mag.size == 0 or mag.max() <= p["nb"], "a digit beyond the bucket range"
        self.ci = row * nb1 + mag                                        # bucket slot of every entry
        self.val = (pos.astype(np.int64) | np.where(d < 0, SIGN, 0)).astype(np.uint32)
        self.total = int(mag.size)
        self.top = (np.arange(W) % p["period"]) == p["top_row"]          # rows that are a top window alone
        lb_row = np.where(self.top, p["LB_top"], p["LB"])
        coarse = (mag - 1) >> lb_row[row]
        assert coarse.size == 0 or coarse.max() < NC, "a top-row digit beyond top_max_b"
        # scanned [window][coarse bin][chunk] histogram, the total behind it
        h = np.bincount((row * NC + coarse) * J + pos // SORT_T, minlength=W * NC * J)
        self.bin_fill = h.reshape(W * NC, J).sum(axis=1)
        self.hist1 = np.concatenate([[0], np.cumsum(h)]).astype(np.uint32)
        self.counts = np.bincount(self.ci, minlength=W * nb1).astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.counts)[:-1]])
        # buckets the top row's finer bins do not cover: counts and nseg zeroed, starts never written
        b = np.tile(np.arange(nb1), W)
        self.unreachable = np.repeat(self.top, nb1) & (b - 1 >= (NC << p["LB_top"])) & (b >= 1)
        order = np.lexsort((self.val, self.ci))
        self.sorted_by_bucket = self.val[order]                          # the multiset of every bucket, ascending
        seg = self.seg = seg_len(p["seg_shift"])
        self.nseg = (self.counts + seg - 1) // seg
        self.split = np.nonzero(self.nseg > 1)[0]

    def seg_class(self, rem):
        s = self.plan["seg_shift"]
        return (rem + (1 << s) - 1) >> s if s > 0 else rem

    def task_table(self, seg_starts):
        """msm_make_task over every segment of every bucket: (records uint32 [n, 4], class of each, bucket of each)"""
        p, seg = self.plan, self.seg
        ci = np.repeat(np.arange(self.counts.size), self.nseg)
        first = np.concatenate([[0], np.cumsum(self.nseg)[:-1]])
        sidx = np.arange(ci.size) - first[ci]
        cnt, ns, start = self.counts[ci], self.nseg[ci], self.starts[ci]
        if p["balanced"]:                                                # msm_seg_range, equal segments
            q, r = cnt // ns, cnt % ns
            off, length = sidx * q + np.minimum(sidx, r), q + (sidx < r)
            cls = self.seg_class((cnt + ns - 1) // ns)
        else:                                                            # full segments plus a remainder
            off = sidx * seg
            length = np.minimum(cnt - off, seg)
            cls = np.where((sidx == cnt // seg) & (cnt % seg != 0), self.seg_class(cnt % seg), MSM_SEG)
        one = ns <= 1
        off, length = np.where(one, 0, off), np.where(one, cnt, length)
        dest = np.where(one, ci - ci // p["nb1"] - 1, np.asarray(seg_starts, np.int64)[ci] + sidx)
        rec = np.stack([start + off, length, dest, np.where(one, 0, 1)], axis=1)
        return (rec & 0xffffffff).astype(np.uint32), cls, ci

    def cell(self, cls, ci):
        """order of the task table: longest class first, windows ascending within a class"""
        return (MSM_SEG - cls) * self.plan["W"] + ci // self.plan["nb1"]


def _rows_sorted(a):
    a = np.ascontiguousarray(a)
    return a[np.lexsort(a.T[::-1])]


def check_view(plan, arrays, digits):
    """raises StageError (an AssertionError whose .stage and text name the stage) at the first stage whose output is
    not what the expected digit rows imply; returns the Expect it was checked against"""
    p = plan
    W, nb1 = p["W"], p["nb1"]
    A = {k: np.asarray(v) for k, v in arrays.items()}
    # 1. recode
    st = STAGES[0]
    got = A["digits"]
    _need(got.shape == np.asarray(digits).shape, st, lambda: f"digit rows {got.shape}, expected {np.shape(digits)}")
    bad = np.argwhere(got != digits)
    _need(bad.size == 0, st, lambda: f"{len(bad)} digits differ, first at row {bad[0][0]} position {bad[0][1]}: "
          f"{got[tuple(bad[0])]} != {digits[tuple(bad[0])]}")
    e = Expect(p, digits)
    # 2. hist / scan
    st = STAGES[1]
    _need(A["hist1"].size == p["hist1_n"] + 1, st, "hist1 size")
    _need(int(A["hist1"][p["hist1_n"]]) == e.total, st,
          lambda: f"hist1[hist1_n] = {A['hist1'][p['hist1_n']]}, {e.total} non-zero digits")
    bad = np.nonzero(A["hist1"] != e.hist1)[0]
    _need(bad.size == 0, st, lambda: f"scanned histogram differs at {bad[:4]} (slot = (row * NC + bin) * J + chunk)")
    # 3. counts / starts
    st = STAGES[2]
    counts, starts = A["counts"].astype(np.int64), A["starts"].astype(np.int64)
    bad = np.nonzero(e.unreachable & (counts != 0))[0]
    _need(bad.size == 0, st, lambda: f"unreachable top-row bucket {bad[0] % nb1} of row {bad[0] // nb1} has count "
          f"{counts[bad[0]]}")
    _need(not counts[::nb1].any(), st, "counts[w * nb1] != 0")
    bad = np.nonzero(counts != e.counts)[0]
    _need(bad.size == 0, st, lambda: f"counts differ at row {bad[0] // nb1} bucket {bad[0] % nb1}: {counts[bad[0]]} != "
          f"{e.counts[bad[0]]}")
    # ascending buckets of a row are a running sum, rows tile [0, total) in row order: one exclusive scan over all
    bad = np.nonzero(~e.unreachable & (starts != e.starts))[0]
    _need(bad.size == 0, st, lambda: f"starts differ at row {bad[0] // nb1} bucket {bad[0] % nb1}: {starts[bad[0]]} != "
          f"{e.starts[bad[0]]}")
    # 4. fine sort
    st = STAGES[3]
    srt = A["sorted"]
    _need(srt.size == e.total, st, "size of sorted")
    bucket_of = np.repeat(np.arange(W * nb1), e.counts)
    got_sorted = srt[np.lexsort((srt, bucket_of))]
    bad = np.nonzero(got_sorted != e.sorted_by_bucket)[0]
    _need(bad.size == 0, st, lambda: f"{len(bad)} entries differ; row {bucket_of[bad[0]] // nb1} bucket "
          f"{bucket_of[bad[0]] % nb1}: has {got_sorted[bad[0]]:#x}, expected {e.sorted_by_bucket[bad[0]]:#x}")
    # 5. plan, pass 1
    st = STAGES[4]
    ctrl, nseg = A["ctrl"].astype(np.int64), A["nseg"].astype(np.int64)
    bad = np.nonzero(e.unreachable & (nseg != 0))[0]
    _need(bad.size == 0, st, lambda: f"unreachable top-row bucket {bad[0] % nb1} has nseg {nseg[bad[0]]}")
    bad = np.nonzero(nseg != e.nseg)[0]
    _need(bad.size == 0, st, lambda: f"nseg differs at row {bad[0] // nb1} bucket {bad[0] % nb1}: {nseg[bad[0]]} != "
          f"{e.nseg[bad[0]]} (count {e.counts[bad[0]]}, segments of {e.seg})")
    want = [e.split.size, None, int(e.nseg[e.split].sum()), int((e.bin_fill > p["fine_cap"]).sum()),
            int((e.nseg > MSM_FINISH_SERIAL).sum())]
    for k in (0, 2, 3, 4):
        _need(ctrl[k] == want[k], st, f"ctrl[{k}] = {ctrl[k]}, expected {want[k]}")
    heavy = np.sort(A["heavy_list"][:e.split.size].astype(np.int64))
    _need(np.array_equal(heavy, e.split), st, "heavy_list is not the set of split buckets")
    ss = A["seg_starts"].astype(np.int64)
    by = e.split[np.argsort(ss[e.split], kind="stable")]
    _need(np.array_equal(ss[by], np.concatenate([[0], np.cumsum(e.nseg[by])])[:by.size]), st,
          "the seg_starts ranges of the split buckets do not tile [0, ctrl[2])")
    # 6. plan, pass 2
    st = STAGES[5]
    _need(ctrl[1] == e.nseg.sum(), st, f"ctrl[1] = {ctrl[1]}, {e.nseg.sum()} segments")
    _need(ctrl[1] <= p["t_max"], st, f"ctrl[1] = {ctrl[1]} > t_max = {p['t_max']}")
    tasks = A["tasks"]
    _need(tasks.shape == (ctrl[1], 4), st, f"task table {tasks.shape}")
    want_tasks, _, _ = e.task_table(ss)
    a, b = _rows_sorted(tasks), _rows_sorted(want_tasks)
    bad = np.nonzero((a != b).any(axis=1))[0]
    _need(bad.size == 0, st, lambda: f"{len(bad)} task records differ, first (sorted): {a[bad[0]]} != {b[bad[0]]}")
    cover = np.zeros(e.total + 1, np.int64)
    np.add.at(cover, tasks[:, 0].astype(np.int64), 1)
    np.add.at(cover, tasks[:, 0].astype(np.int64) + tasks[:, 1], -1)
    _need((np.cumsum(cover)[:-1] == 1).all(), st, "a position of sorted is not covered by exactly one task")
    if len(tasks):
        ci = bucket_of[tasks[:, 0].astype(np.int64)]
        cnt, off = e.counts[ci], tasks[:, 0].astype(np.int64) - e.starts[ci]
        if p["balanced"]:
            cls = e.seg_class((cnt + e.nseg[ci] - 1) // e.nseg[ci])
        else:
            cls = np.where((off == (cnt // e.seg) * e.seg) & (cnt % e.seg != 0), e.seg_class(cnt % e.seg), MSM_SEG)
        cell = e.cell(cls, ci)
        bad = np.nonzero(np.diff(cell) < 0)[0]
        _need(bad.size == 0, st, lambda: f"task order: task {bad[0] + 1} (class {cls[bad[0] + 1]}, window "
              f"{ci[bad[0] + 1] // nb1}) follows class {cls[bad[0]]}, window {ci[bad[0]] // nb1}")
    return e


def simulate_view(plan, digits, rng):
    """a valid view of the stage's output for these digit rows: random order inside each bucket, a random legal
    seg_starts assignment, noise wherever the kernels leave memory unwritten.  rng: numpy Generator"""
    p = plan
    e = Expect(p, digits)
    n = e.counts.size
    noise = lambda k: rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32)      # noqa: E731
    order = np.lexsort((rng.random(e.total), e.ci))
    starts = e.starts.astype(np.uint32)
    starts[e.unreachable] = noise(int(e.unreachable.sum()))
    split = rng.permutation(e.split)
    seg_starts = noise(n)
    seg_starts[split] = np.concatenate([[0], np.cumsum(e.nseg[split])[:-1]])[:split.size]
    heavy = noise(n)
    heavy[:split.size] = rng.permutation(e.split)
    tasks, cls, ci = e.task_table(seg_starts)
    shuffle = rng.permutation(len(tasks))
    tasks = tasks[shuffle][np.argsort(e.cell(cls, ci)[shuffle], kind="stable")]
    ctrl = np.array([split.size, len(tasks), e.nseg[e.split].sum(), (e.bin_fill > p["fine_cap"]).sum(),
                     (e.nseg > MSM_FINISH_SERIAL).sum()], np.uint32)
    dt = np.int32 if p["wide"] else np.int16
    return {"digits": np.asarray(digits).astype(dt), "hist1": e.hist1.copy(), "counts": e.counts.astype(np.uint32),
            "starts": starts, "sorted": e.val[order], "nseg": e.nseg.astype(np.uint32), "seg_starts": seg_starts,
            "heavy_list": heavy, "tasks": tasks, "ctrl": ctrl}
