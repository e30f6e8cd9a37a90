"""Pi_Nullity of AC20 (p. 17-18; verifiable_mpc/ac20/nullity.py:21-40) over Ed25519: prove that s linear forms all
vanish on a committed vector, by opening the one form L = sum_i rho^i L_i with Protocol 5.

    FormMatrix                  s linear forms over n variables in HBM, dense (row-major, strided) or sparse (CSR)
    prove_nullity_compressed    nullity.py:21-28
    verify_nullity_compressed   nullity.py:31-40

(prove_nullity_koe, nullity.py's other flavour, is not built: knowledge_of_exponent.py says why.)

The reference composes L with s Python form products and s sums.  Here (csrc/nullity.hip) a dense matrix is combined
in one pass - a lane per column, Horner over the rows - and all s values L_i(x) come from one launch sequence; sparse
forms go through the transposed product of csrc/fr_colsum.h (sparse.DeviceMatrix) with the weights rho^i.

Transcripts, selected by `transcript=` (default: TRANSCRIPT below): "compact" (DESIGN.md section 16 states the bytes;
tests/nullity_ref.py restates them) - forms, L and x device-resident all the way into the compact Protocol 5 - and
"reference": rho = pivot.fiat_shamir_hash([P, lin_forms], order), and with list-mode forms L by the reference's own
expression on the host, so that Python ints grow unreduced exactly as they do there.

Like the reference, the prover proves whatever y = L(x) is; FormMatrix.first_nonzero tells a caller which form does
not vanish.
"""
import hashlib

import numpy as np

from . import compressed_pivot, pivot, sparse, wire
from .device import ScalarVector, _View, get_context
from .groups import ORDER, as_point

TRANSCRIPT = "compact"
RHO_TAG = b"vmpc-ac20/nullity/v1"
FORMS_TAG = b"vmpc-ac20/nullity/forms/v1"
MISMATCH = "Linear form L does not correspond to reconstructed linear form with rho."    # nullity.py:34-36


def _is_form(f):
    return hasattr(f, "coeffs") and hasattr(f, "constant")


def _device_forms(lin_forms):
    return isinstance(lin_forms, FormMatrix) or isinstance(lin_forms, np.ndarray) or \
        any(isinstance(f.coeffs, ScalarVector) for f in lin_forms)


class FormMatrix:
    """s linear forms over n variables on the device.  FormMatrix(forms): a list of LinearForm / AffineForm (list or
    ScalarVector coefficients; constants are not part of a linear form and are ignored), or an (s, n, 32) uint8 array
    of 256-bit little-endian values (taken mod l); n= gives the width of an empty list.  from_csr / from_device: below.

        combine(rho)      -> ScalarVector, sum_i rho^i L_i
        values(x)         -> [L_i(x)] as ints
        first_nonzero(x)  -> the smallest i with L_i(x) != 0, or None
        digest            SHA-256 over the shape and the canonical element bytes (dense: leaves hashed on the device)
    """

    def __init__(self, forms, n=None, ctx=None):
        self.ctx = ctx = ctx or get_context()
        self.sparse = None
        self._digest = None
        if isinstance(forms, np.ndarray):
            if forms.dtype != np.uint8 or forms.ndim != 3 or forms.shape[2] != 32:
                raise ValueError("FormMatrix: an array of forms is (s, n, 32) uint8")
            self.s, self.n = int(forms.shape[0]), int(forms.shape[1])
            self._set_dense(ctx.upload(np.ascontiguousarray(forms)) if forms.size else ctx.alloc(32), self.n,
                            canonical=not bool((forms[:, :, 31] >= 0x10).any()))
            return
        forms = list(forms)
        if not all(_is_form(f) for f in forms):
            raise ValueError("FormMatrix: a list of linear forms, an (s, n, 32) uint8 array, or from_csr / from_device")
        self.s = len(forms)
        self.n = len(forms[0].coeffs) if forms else int(n or 0)
        if any(len(f.coeffs) != self.n for f in forms):
            raise ValueError("FormMatrix: the forms have different lengths")
        buf = ctx.alloc(max(32, 32 * self.s * self.n))
        for i, f in enumerate(forms):
            if not self.n:
                break
            if isinstance(f.coeffs, ScalarVector):
                ctx.copy(buf.ptr + 32 * i * self.n, f.coeffs.ptr, 32 * self.n)
            else:
                ctx.upload_into(buf.ptr + 32 * i * self.n, sparse.residue_array([pivot._residue(c) for c in f.coeffs], ORDER))
        self._set_dense(buf, self.n, canonical=True)

    def _set_dense(self, buf, stride, canonical):
        self.stride = stride
        total = self.s * self.n
        if not canonical:
            # one row of s n elements under s = 1: vmpc_fr_rows_combine_dev copies it reduced
            if total > 1 << 30:
                raise ValueError("FormMatrix: more than 2^30 elements with values >= l among them")
            reduced = self.ctx.alloc(32 * total)
            self.ctx.fr_rows_combine(buf.ptr, 1, total, total, 1, reduced.ptr)
            buf = reduced
        self.buf = buf

    @classmethod
    def from_device(cls, data, s, n, row_stride=None, ctx=None):
        """rows already in HBM: `data` a ScalarVector (canonical residues, as every ScalarVector holds) whose element
        i row_stride + j is coefficient j of form i; row_stride >= n (default n).  Not copied."""
        self = cls.__new__(cls)
        self.ctx = ctx or data.ctx
        self.sparse, self._digest = None, None
        self.s, self.n = int(s), int(n)
        stride = self.n if row_stride is None else int(row_stride)
        if stride < self.n or (self.s and len(data) < (self.s - 1) * stride + self.n):
            raise ValueError("FormMatrix.from_device: the buffer does not hold s rows of n at this stride")
        self.stride, self.buf = stride, data
        return self

    @classmethod
    def from_csr(cls, row_ptr, col, vals, n, ctx=None):
        """sparse forms: row i holds vals[e] at column col[e] for row_ptr[i] <= e < row_ptr[i + 1]; vals as
        circuit_sat_gpu.SparseCircuit takes them (ints of any sign or size, an integer array, (nnz, 32) uint8);
        duplicates add, zeros are dropped"""
        self = cls.__new__(cls)
        self.ctx = ctx or get_context()
        self._digest = None
        self.n = int(n)
        self.sparse = sparse.CanonicalCSR((row_ptr, col, vals), self.n, ORDER, "SparseCircuit: FormMatrix")
        self.s = self.sparse.n_rows
        self._dev = sparse.DeviceMatrix(self.ctx, self.sparse)
        return self

    def __len__(self):
        return self.s

    @property
    def ptr(self):
        return self.buf.ptr

    # ---- the three products ------------------------------------------------------------------------------------------
    def combine(self, rho):
        rho = int(rho) % ORDER
        out = ScalarVector.empty(self.n, self.ctx)
        if self.sparse is not None:
            pw, p = [], 1
            for _ in range(self.s):
                pw.append(p)
                p = p * rho % ORDER
            wts = ScalarVector.from_ints(pw, self.ctx)
            self._dev.weighted_columns(wts.ptr, self.n, 0, out.ptr, self.n)     # every column is an "input" column
        else:
            self.ctx.fr_rows_combine(self.ptr, self.s, self.n, self.stride, rho, out.ptr)
        return out

    def _values_dev(self, x):
        x = pivot._as_device(x)
        if len(x) != self.n:
            raise ValueError(f"FormMatrix: {self.n} variables, {len(x)} values")
        out = ScalarVector.empty(self.s, self.ctx)
        if self.sparse is not None:
            if self.s:      # the kernel's two row sets are both these rows: one buffer takes both (check = 2)
                self.ctx.cs_triples(self._dev.csr(), self._dev.csr(), None, self.s, self.n, 0, x.ptr, out.ptr, out.ptr, 2)
            return out, False
        return out, self.ctx.fr_rows_dot(self.ptr, self.s, self.n, self.stride, x.ptr, out.ptr)

    def values(self, x):
        return self._values_dev(x)[0].to_ints()

    def first_nonzero(self, x):
        out, first = self._values_dev(x)
        if first is False:      # sparse rows: no index from the kernel
            return next((i for i, v in enumerate(out.to_ints()) if v), None)
        return first

    # ---- what the transcripts read -------------------------------------------------------------------------------
    @property
    def digest(self):
        if self._digest is None:
            head = self.s.to_bytes(8, "little") + self.n.to_bytes(8, "little")
            if self.sparse is not None:
                self._digest = hashlib.sha256(FORMS_TAG + b"S" + head + self.sparse.canonical_bytes()).digest()
            else:
                nbytes = 32 * self.s * self.n
                rows = self
                if self.stride != self.n and self.s > 1:       # the digest is of the rows without the gaps
                    rows = self.ctx.alloc(max(32, nbytes))
                    for i in range(self.s):
                        self.ctx.copy(rows.ptr + 32 * i * self.n, self.ptr + 32 * i * self.stride, 32 * self.n)
                leaves = self.ctx.sha256_chunks(rows.ptr, nbytes, compressed_pivot.CHUNK)
                self._digest = hashlib.sha256(FORMS_TAG + b"D" + head + leaves).digest()
        return self._digest

    def forms(self):
        """the rows as LinearForms over device coefficients (views, nothing is copied): what the reference transcript
        prints"""
        if self.sparse is not None:
            raise ValueError("FormMatrix: the reference transcript prints dense forms; sparse ones have none")
        buf = self.buf.v.buf if isinstance(self.buf, ScalarVector) else self.buf
        off = self.buf.v.off if isinstance(self.buf, ScalarVector) else 0
        return [pivot.LinearForm(ScalarVector(_View(buf, off + i * self.stride, self.n, 32), self.ctx))
                for i in range(self.s)]


def as_form_matrix(lin_forms):
    return lin_forms if isinstance(lin_forms, FormMatrix) else FormMatrix(lin_forms)


def compact_challenge(P, forms_digest, order=ORDER):
    """rho of the compact transcript: SHA-256(tag || compressed P || FormMatrix.digest), little-endian, mod l"""
    return int.from_bytes(hashlib.sha256(RHO_TAG + wire.compress_point(as_point(P)) + forms_digest).digest(),
                          "little") % order


def _host_combination(lin_forms, rho):
    return sum((linform_i) * (rho ** i) for i, linform_i in enumerate(lin_forms))      # nullity.py:25, :32


def _printable(lin_forms):
    return lin_forms.forms() if isinstance(lin_forms, FormMatrix) else \
        FormMatrix(lin_forms).forms() if isinstance(lin_forms, np.ndarray) else lin_forms


def prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf, transcript=None, r=None, mask=None):
    """nullity.py:21-28: (proof, L, y, rho).  `r`, `mask`: Protocol 5's masks (protocol_5_prover's r= and rho=; rho is
    the challenge here), drawn there when None."""
    mode = compressed_pivot.transcript_mode(transcript, TRANSCRIPT)
    order = gf.order
    if mode == "reference":
        shown = _printable(lin_forms)
        rho = pivot.fiat_shamir_hash([P, shown], order)
        if not _device_forms(lin_forms):
            L = _host_combination(lin_forms, rho)
            y = L(x)
        else:
            L = pivot.LinearForm(as_form_matrix(lin_forms).combine(rho))
            y = gf(L.coeffs.dot(pivot._as_device(x)))
    else:
        assert order == ORDER
        fm = as_form_matrix(lin_forms)
        rho = compact_challenge(P, fm.digest, order)
        L = pivot.LinearForm(fm.combine(rho))
        x = pivot._as_device(x)
        y = gf(L.coeffs.dot(x))
        if r is None and len(x) >= compressed_pivot.MASKS_ON_DEVICE_MIN:
            r = compressed_pivot.masks(len(x), fm.ctx)
    proof = compressed_pivot.protocol_5_prover(generators, P, L, y, x, gamma, gf, transcript=mode, r=r, rho=mask)
    return proof, L, y, rho


def verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf, transcript=None):
    """nullity.py:31-40: a bool.  The compact transcript also refuses a rho that is not the hash of (P, lin_forms):
    the reference takes the challenge as it is handed in, and so does the reference transcript here."""
    mode = compressed_pivot.transcript_mode(transcript, TRANSCRIPT)
    if mode == "reference" and not _device_forms(lin_forms) and not isinstance(L.coeffs, ScalarVector):
        L_check = _host_combination(lin_forms, rho)
        if not L_check == L:
            print(MISMATCH)
            return False
        return compressed_pivot.protocol_5_verifier(generators, P, L, y, proof, gf, transcript=mode)
    fm = as_form_matrix(lin_forms)
    rho = int(rho) % gf.order
    if mode == "compact" and rho != compact_challenge(P, fm.digest, gf.order):
        return False
    L_check = fm.combine(rho)
    theirs = pivot._as_device(L.coeffs)
    if len(theirs) != fm.n or fm.ctx.cs_first_diff(L_check.ptr, theirs.ptr, fm.n) is not None:
        print(MISMATCH)
        return False
    return compressed_pivot.protocol_5_verifier(generators, P, pivot.LinearForm(L_check), y, proof, gf, transcript=mode)


def verify_nullity_compressed_batch(generators, items, gf, transcript=None):
    """[verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf, transcript) for (P, L, lin_forms, rho,
    y, proof) in items]: the rho check and the combination of the forms per item as there, then ONE batched pivot
    verification (compressed_pivot.protocol_5_verifier_batch) for the items that passed them"""
    mode = compressed_pivot.transcript_mode(transcript, TRANSCRIPT)
    items = list(items)
    if mode == "reference":
        return [verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf, transcript=mode)
                for P, L, lin_forms, rho, y, proof in items]
    out = [False] * len(items)
    statements, where = [], []
    for i, (P, L, lin_forms, rho, y, proof) in enumerate(items):
        fm = as_form_matrix(lin_forms)
        rho = int(rho) % gf.order
        if rho != compact_challenge(P, fm.digest, gf.order):
            continue
        L_check = fm.combine(rho)
        theirs = pivot._as_device(L.coeffs)
        if len(theirs) != fm.n or fm.ctx.cs_first_diff(L_check.ptr, theirs.ptr, fm.n) is not None:
            print(MISMATCH)
            continue
        statements.append((P, pivot.LinearForm(L_check), y, proof))
        where.append(i)
    for i, ok in zip(where, compressed_pivot.protocol_5_verifier_batch(generators, statements, gf, transcript=mode)):
        out[i] = ok
    return out
