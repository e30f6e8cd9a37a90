"""Sparse matrices over a 256-bit scalar field, host side: what Pinocchio's R1CS (pynocchio.py, BN-256's GF(n)),
Protocol 8's circuits (circuit_sat_gpu.py) and Pi_Nullity's sparse forms (nullity.py, both Ed25519's GF(l)) share.

    values_array     coefficients of any of the accepted kinds -> (nnz, 32) uint8 residues
    csr_entries      a CSR triple checked and expanded to (rows, col, values)
    colsum_plan      the items / long columns that csrc/fr_colsum.h runs
    ColumnPlan       entries in column order in HBM with their plan; run() is the transposed product
    CanonicalCSR     affine forms as canonical CSR with canonical_bytes(), the bytes that digests are made of
    DeviceMatrix     a CanonicalCSR in HBM: rows for the row evaluation, a ColumnPlan for the transposed product

Nothing here knows a modulus: the order is an argument, and `field` names the library's entry point."""
import numpy as np

from . import _native
from .device import ScalarVector

SEG = 64                    # entries per lane of the column sums (csrc/fr_colsum.h); longer columns are cut
PARTIAL = 1 << 31           # an item's dst with this bit set is a partial sum of a long column (FR_COLSUM_PARTIAL)
# field -> the Context method of its entry point ("bn256_cs": Protocol 8's forms over GF(n): out zeroed first, as "ed25519")
_COLSUM = {"bn256": "bn256_qap_colsum", "ed25519": "cs_colsum", "bn256_cs": "bn256_cs_colsum"}


def residue_array(vals, order):
    """ints or field elements of any sign or size -> (n, 32) uint8 canonical residues"""
    return _native.ints_to_array([int(v) % order for v in vals], 32)


def values_array(vals, order, canonical):
    """coefficients -> (nnz, 32) uint8 residues mod `order`: ints of any sign or size, an integer numpy array (reduced
    here; negative entries become order - |v|), or a (nnz, 32) uint8 array of 256-bit little-endian values.  The last
    kind passes through for the device to reduce unless `canonical`: then rows >= order are reduced here (a copy), as
    bytes that go into a digest must be."""
    if isinstance(vals, np.ndarray) and vals.dtype == np.uint8 and vals.ndim == 2:
        a = np.ascontiguousarray(vals)
        if canonical:
            a = a.copy()
            for i in np.nonzero(a[:, 31] >= (order >> 248))[0].tolist():       # only these can be >= order
                a[i] = np.frombuffer((int.from_bytes(a[i].tobytes(), "little") % order).to_bytes(32, "little"), np.uint8)
        return a
    if isinstance(vals, np.ndarray) and vals.dtype.kind in "iu" and vals.ndim == 1 and vals.dtype.itemsize <= 8:
        a = vals.astype(np.int64) if vals.dtype.kind == "i" else vals.astype(np.uint64)
        neg = a < 0 if a.dtype.kind == "i" else np.zeros(len(a), bool)
        mag = np.where(neg, -a, a).astype(np.uint64)
        words = np.zeros((len(a), 8), np.int64)
        words[:, 0] = (mag & np.uint64(0xFFFFFFFF)).astype(np.int64)
        words[:, 1] = (mag >> np.uint64(32)).astype(np.int64)
        if neg.any():
            order_words = [(order >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
            borrow = np.zeros(int(neg.sum()), np.int64)
            sub = words[neg]
            for k in range(8):
                dk = order_words[k] - sub[:, k] - borrow
                borrow = (dk < 0).astype(np.int64)
                sub[:, k] = dk + (borrow << 32)
            words[neg] = sub
        return np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(-1, 32)
    return residue_array(list(vals), order)


def csr_entries(row_ptr, col, vals, order, canonical, who, n_cols=None):
    """(rows, col, values (nnz, 32), n_rows) of a CSR triple; ValueError("{who}: ..") unless row_ptr rises from 0 to
    len(col), there is one value per entry and, where n_cols is given, every column is below it"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_rows = len(row_ptr) - 1
    if n_rows < 0 or row_ptr[0] != 0 or np.any(np.diff(row_ptr) < 0) or row_ptr[-1] != len(col):
        raise ValueError(f"{who}: row_ptr must rise from 0 to the number of entries")
    v = values_array(vals, order, canonical)
    if len(v) != len(col):
        raise ValueError(f"{who}: one value per entry")
    if n_cols is not None and len(col) and (col.min() < 0 or col.max() >= n_cols):
        raise ValueError(f"{who}: column index out of range")
    return np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(row_ptr)), col, v, n_rows


def colsum_plan(col_ptr, dst=None, piece=SEG):
    """items (start, end, dst) and long columns (dst, first partial, count) of csrc/fr_colsum.h for entries in column
    order (col_ptr: n_cols + 1 offsets) -> (items, longs, n_partial).  dst[c]: where column c's sum goes (default c).
    Without dst an empty column is one empty item (it writes 0); with dst it has no item, and its position is the
    caller's to fill."""
    col_ptr = np.asarray(col_ptr, np.int64)
    lens = np.diff(col_ptr)
    pieces = (lens + piece - 1) // piece
    out_of = np.arange(len(lens), dtype=np.int64) if dst is None else np.asarray(dst, np.int64)
    if dst is None:
        pieces = np.maximum(1, pieces)
    n_items = int(pieces.sum())
    col_of = np.repeat(np.arange(len(lens), dtype=np.int64), pieces)
    first_item = np.cumsum(pieces) - pieces
    start = col_ptr[col_of] + (np.arange(n_items, dtype=np.int64) - first_item[col_of]) * piece
    end = np.minimum(start + piece, col_ptr[col_of + 1])
    is_long = pieces > 1
    is_part = is_long[col_of]
    part_idx = np.cumsum(is_part) - 1
    items = np.stack([start, end, np.where(is_part, PARTIAL | part_idx, out_of[col_of])], axis=1).astype(np.uint32)
    long_cols = np.nonzero(is_long)[0]
    longs = np.stack([out_of[long_cols], part_idx[first_item[long_cols]], pieces[long_cols]], axis=1).astype(np.uint32)
    return items, longs, int(is_part.sum())


class ColumnPlan:
    """entries (cols, rows, vals) of n_cols columns in column order on the device, with their colsum plan;
    run(weights, n_rows, out, n_out): out[dst[c]] = sum over column c of vals[e] weights[rows[e]] in `field`.
    place=False: no items yet, the caller calls place(dst) before the first run."""

    def __init__(self, ctx, cols, rows, vals, n_cols, dst=None, field="bn256", place=True):
        order = np.argsort(cols, kind="stable")                 # rows ascending inside a column
        counts = np.bincount(cols, minlength=n_cols) if len(cols) else np.zeros(n_cols, np.int64)
        self.col_ptr = np.concatenate([[0], np.cumsum(counts)])
        self.ctx, self.nnz, self.n_cols, self._run = ctx, len(cols), n_cols, getattr(ctx, _COLSUM[field])
        self.rows = ctx.upload(np.ascontiguousarray(np.asarray(rows, np.uint32)[order])) if len(cols) else ctx.alloc(4)
        self.vals = ctx.upload(np.ascontiguousarray(vals[order])) if len(cols) else ctx.alloc(32)
        self.items = None
        if place:
            self.place(dst)

    def place(self, dst):
        """(re)make the items for the output positions dst (colsum_plan)"""
        items, longs, self.n_partial = colsum_plan(self.col_ptr, dst)
        self.items, self.n_items = self.ctx.upload(items) if len(items) else self.ctx.alloc(4), len(items)
        self.longs, self.n_long = self.ctx.upload(longs) if len(longs) else self.ctx.alloc(4), len(longs)

    def run(self, weights_ptr, n_rows, out_ptr, n_out=None):
        if self.items is None:
            raise RuntimeError("ColumnPlan: place() the items before run()")
        self._run(weights_ptr, n_rows, self.rows.ptr, self.vals.ptr, self.nnz, self.items.ptr, self.n_items,
                  self.longs.ptr, self.n_long, self.n_partial, out_ptr, self.n_cols if n_out is None else n_out)


class CanonicalCSR:
    """affine forms as canonical CSR: entries sorted by (row, col), duplicates added and zeros dropped ON THE HOST, so
    that canonical_bytes() depends on the forms alone.  M: (row_ptr, col, vals[, consts])."""

    def __init__(self, M, n_cols, order, who):
        consts = M[3] if len(M) == 4 else None
        rows, col, v, n_rows = csr_entries(M[0], M[1], M[2], order, True, who, n_cols)
        key = rows * max(n_cols, 1) + col
        by_key = np.argsort(key, kind="stable")
        key, rows, col, v = key[by_key], rows[by_key], col[by_key], v[by_key]
        dup = np.nonzero(key[1:] == key[:-1])[0]
        if len(dup):
            keep = np.ones(len(key), bool)
            for i in dup.tolist():          # entry i + 1 repeats entry i: add it into the first of its run
                first = i
                while not keep[first]:
                    first -= 1
                s = int.from_bytes(v[first].tobytes(), "little") + int.from_bytes(v[i + 1].tobytes(), "little")
                v[first] = np.frombuffer((s % order).to_bytes(32, "little"), np.uint8)
                keep[i + 1] = False
            rows, col, v = rows[keep], col[keep], v[keep]
        nz = v.any(axis=1) if len(v) else np.zeros(0, bool)
        rows, col, v = rows[nz], col[nz], v[nz]
        self.n_rows, self.n_cols = n_rows, n_cols
        self.rows, self.col, self.vals = rows, col, np.ascontiguousarray(v)
        self.row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64) \
            if n_rows else np.zeros(1, np.int64)
        self.consts = values_array(consts, order, True) if consts is not None else np.zeros((n_rows, 32), np.uint8)
        if len(self.consts) != n_rows:
            raise ValueError(f"{who}: one constant per row")

    def canonical_bytes(self):
        return b"".join([self.n_rows.to_bytes(8, "little"), len(self.col).to_bytes(8, "little"),
                         self.row_ptr.astype("<u8").tobytes(), self.col.astype("<u8").tobytes(), self.vals.tobytes(),
                         self.consts.tobytes()])

    def const_ints(self):
        return _native.array_to_ints(self.consts)


class DeviceMatrix:
    """a CanonicalCSR over GF(l) - or, vector=BnScalarVector, over GF(n) - in HBM: CSR for the row evaluation, a
    ColumnPlan over its non-empty columns for the transposed product"""

    def __init__(self, ctx, M, vector=ScalarVector):
        self.ctx, self.n_rows, self.nnz = ctx, M.n_rows, len(M.col)
        self.row_ptr = ctx.upload(M.row_ptr.astype(np.uint32))
        self.col = ctx.upload(M.col.astype(np.uint32)) if self.nnz else ctx.alloc(4)
        self.vals = ctx.upload(M.vals) if self.nnz else ctx.alloc(32)
        self.consts = vector.from_array(M.consts, ctx) if M.n_rows else vector.empty(0, ctx)
        self.listed, compact = np.unique(M.col, return_inverse=True)
        self.plan = ColumnPlan(ctx, compact, M.rows, M.vals, len(self.listed), field="bn256_cs" if vector.BN else "ed25519",
                               place=False)
        self._placed = None             # the (n_x, n_in) of the plan's items: weighted_columns places them

    def csr(self):
        return (self.row_ptr.ptr, self.col.ptr, self.vals.ptr, self.consts.ptr)

    def weighted_columns(self, weights_ptr, n_x, n_in, out_ptr, n_out):
        """out (n_out scalars over z) = sum_i weights[i] row_i, column c at z position c (c < n_x) or n_in + 3 + c - n_x.
        The plan's items are made per (n_x, n_in); only the last pair's are kept."""
        if self._placed != (n_x, n_in):
            self.plan.place(np.where(self.listed < n_x, self.listed, self.listed - n_x + n_in + 3))
            self._placed = (n_x, n_in)
        self.plan.run(weights_ptr, self.n_rows, out_ptr, n_out)
