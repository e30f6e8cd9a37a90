"""Protocol 8 of AC20 (circuit satisfiability, verifiable_mpc/ac20/circuit_sat_cb.py:59-318) from a SPARSE circuit, on
the device: the step that turns "a circuit and its inputs" into the triple (z, [z], L) the pivots take.

    SparseCircuit                    what Protocol 8 needs of a circuit_builder.Circuit, as CSR data
    protocol_8_excl_pivot_prover     circuit_sat_cb.py:59-166
    protocol_8_excl_pivot_verifier   circuit_sat_cb.py:169-252
    circuit_sat_prover / _verifier   circuit_sat_cb.py:255-318 (PivotChoice.compressed and .pivot)

The reference evaluates the gates one by one, interpolates f and g as coefficient lists, multiplies them and evaluates h
at 2m + 1 points (quadratic Python with a large constant), and builds a dense form per gate.  Here (csrc/circuit_sat.hip)
the triples are computed level by level, f and g are extended to 0 and m+2..2m in barycentric form (a correlation with
the table 1/k: the one quadratic step, this field has no NTT), the Lagrange vectors at the challenge are prefix / suffix
products, and the forms are transposed sparse mat-vecs.  z and L never leave the device between the triples and the
pivot.

Transcripts, selected by `transcript=` (default: TRANSCRIPT below): "compact" (DESIGN.md section 15 states the bytes;
tests/p8_ref.py restates them) - the path that scales, z and L device-resident - and "reference": the reference's two
str(input_list) hashes with its element types, list mode, O((n_out + 3) N) text, for parity on small circuits.

Two fields and two commitment schemes, ONE statement of the protocol.  A SparseCircuit carries its
order: the Ed25519 order (the default) or the BN-256 order, and with it the device vector class and the kernels' field
(_Field).  The generators select the scheme as in the reference (circuit_sat_cb.py:65-72, :183): {"g", "h", ..} commit
to z by an Ed25519 vector commitment and open L with the compressed or the plain pivot; a pp {"pp_lhs", "pp_rhs"}
(knowledge_of_exponent.trusted_setup) commits by the restriction argument (P, pi) and opens L with the
knowledge-of-exponent pivot - three group elements whatever N is, no power-of-two padding of z, compact transcript
only.  A verifier recognises the variant by a z_commitment that is a dict.

K witnesses of ONE circuit: protocol_8_excl_pivot_prover_batch / circuit_sat_prover_batch run every stage once for all
K, over either field and scheme (DESIGN.md sections 20 and 32), and return what K single calls return.
"""
import hashlib
from random import SystemRandom

import numpy as np

from . import compressed_pivot, pivot, sparse, wire
from . import knowledge_of_exponent as koe
from .device import BN256_ORDER, BnScalarVector, ScalarVector, get_context
from .fields import FiniteFieldElement
from .groups import ORDER

prng = SystemRandom()

TRANSCRIPT = "compact"


class _Field:
    """what Protocol 8 knows of its scalar field: the order, the device vector class (ScalarVector / BnScalarVector;
    its BN is the `bn=` of the Context's cs_* methods) and the tag of a circuit's digest"""

    def __init__(self, order, vector, circuit_tag):
        self.order, self.vector, self.bn, self.circuit_tag = order, vector, vector.BN, circuit_tag

    def residue(self, v):
        """int, own or foreign field element -> canonical residue (pivot._residue, with this field's order)"""
        return int(v.value if pivot._duck_field(v) and not isinstance(v, FiniteFieldElement) else v) % self.order

    def residues(self, vals):
        return sparse.residue_array([self.residue(v) for v in vals], self.order)


_FIELDS = {ORDER: _Field(ORDER, ScalarVector, b"vmpc-ac20/p8/circuit/v1"),
           BN256_ORDER: _Field(BN256_ORDER, BnScalarVector, b"vmpc-ac20/p8/circuit/bn256/v1")}


class SparseCircuit:
    """The circuit as data.  A, B: the affine forms of the left / right wire of each of the m multiplication gates over
    the columns (x_0..x_{n_x-1}, gamma_0..gamma_{m-1}), as CSR (row_ptr, col, vals, consts) - vals / consts: ints of any
    sign or size, an integer array, or (nnz, 32) uint8; duplicates add; consts may be left out (zeros).  Row i may only
    read gamma_j with j < i.  O: the forms of the n_out output gates, same shape (None: no outputs).  text: what stands
    for str(circuit) (default: the hex SHA-256 of the canonical CSR bytes).

    m = 0 is allowed: f and g are then the constants r_a, r_b (the reference's lagrange_interp_ff of a one-point
    vector) and z = x + [r_a, r_b, r_a r_b].

    order: the field the forms are canonicalised in and the device tables and kernels run over - the Ed25519 order
    (default: today's object and digest) or the BN-256 order (the knowledge-of-exponent variant; the digest's tag then
    says so)."""

    def __init__(self, n_x, A, B, O=None, text=None, order=ORDER):
        self.n_x = int(n_x)
        if int(order) not in _FIELDS:
            raise ValueError("SparseCircuit: order is neither the Ed25519 nor the BN-256 group order")
        self.order, self.field = int(order), _FIELDS[int(order)]
        order = self.order
        m = len(A[0]) - 1
        self.A = sparse.CanonicalCSR(A, self.n_x + m, order, "SparseCircuit: A")
        self.B = sparse.CanonicalCSR(B, self.n_x + m, order, "SparseCircuit: B")
        if self.B.n_rows != m:
            raise ValueError("SparseCircuit: A and B must have one row per multiplication gate each")
        self.O = sparse.CanonicalCSR(O if O is not None else ([0], [], [], []), self.n_x + m, order, "SparseCircuit: O")
        self.m, self.n_out = m, self.O.n_rows
        for M, what in ((self.A, "A"), (self.B, "B")):
            bad = np.nonzero(M.col >= self.n_x + M.rows)[0]
            if len(bad):
                e = bad[np.argmin(M.rows[bad])]
                raise ValueError(f"SparseCircuit: row {int(M.rows[e])} of {what} reads gamma_{int(M.col[e]) - self.n_x}, "
                                 f"which is not an earlier gate")
        self.digest = hashlib.sha256(self.field.circuit_tag + b"".join(v.to_bytes(8, "little") for v in
                                                                       (self.n_x, self.m, self.n_out)) +
                                     b"".join(M.canonical_bytes() for M in (self.A, self.B, self.O))).digest()
        self.text = text if text is not None else self.digest.hex()
        # depth of each multiplication gate and the gates grouped by depth: dependencies point backwards, so one pass
        # over the gamma entries of A and B in row order (a gate's depth is final before any later gate reads it)
        depth = [0] * m
        dep_r = np.concatenate([M.rows[M.col >= self.n_x] for M in (self.A, self.B)])
        dep_j = np.concatenate([M.col[M.col >= self.n_x] - self.n_x for M in (self.A, self.B)])
        by_row = np.argsort(dep_r, kind="stable")
        for r, j in zip(dep_r[by_row].tolist(), dep_j[by_row].tolist()):
            if depth[j] >= depth[r]:
                depth[r] = depth[j] + 1
        self.depth = np.asarray(depth, np.int64)
        self.level_order = np.argsort(self.depth, kind="stable").astype(np.uint32)
        self.level_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.depth))]).astype(np.int64) if m else \
            np.zeros(1, np.int64)
        self._dev = None
        self._raw = None

    # the names Protocol 8 reads of a circuit_builder.Circuit
    @property
    def input_ct(self):
        return self.n_x

    @property
    def mul_ct(self):
        return self.m

    @property
    def output_ct(self):
        return self.n_out

    def __str__(self):
        return self.text

    def padding(self, n_x=None):
        """zeros to append to x so that len(z) + 1 is a power of two (circuit_sat_cb.py:46-56)"""
        z_len = (self.n_x if n_x is None else n_x) + 3 + 2 * self.m
        return 0 if bin(z_len + 1).count("1") == 1 else (1 << z_len.bit_length()) - z_len - 1

    def pad(self, x):
        """x with padding(len(x)) zeros appended: inputs no form reads"""
        return list(x) + [0] * self.padding(len(x))

    @classmethod
    def from_circuit(cls, circuit, order=ORDER):
        """From a circuit_builder.Circuit (duck-typed), by the rules of construct_affine_form
        (circuit_builder.py:417-498), each add / scalar-mul gate expanded once."""
        n = circuit.input_ct
        by_name, forms = {}, {}
        for g in circuit.gates:
            by_name.setdefault(g.output.name, g)

        def is_var(v):
            return hasattr(v, "input_index")

        def var_form(v):
            if not is_var(v):
                return {}, 0 + v
            if v.input_index is not None:
                return {v.input_index: 1}, 0
            child = by_name[v.name]
            if child.op.name == "mul":
                return {n + child.mul_index: 1}, 0
            return forms[id(child)]

        def scaled(form, s):
            return {c: v * s for c, v in form[0].items()}, form[1] * s

        # gates are in creation order, so a gate's inputs are expanded before it: no recursion, each gate once.
        # Coefficients stay the Python objects the builder holds (ints of any sign, field elements): the reference
        # transcript prints them as they are.
        for g in circuit.gates:
            name = g.op.name
            if name == "add":
                (e0, k0), (e1, k1) = var_form(g.inputs[0]), var_form(g.inputs[1])
                e = dict(e0)
                for c, v in e1.items():
                    e[c] = e.get(c, 0) + v
                forms[id(g)] = (e, k0 + k1)
            elif name == "scalar_mul":
                if is_var(g.inputs[0]):
                    forms[id(g)] = scaled(var_form(g.inputs[0]), g.inputs[1])
                elif is_var(g.inputs[1]):
                    forms[id(g)] = scaled(var_form(g.inputs[1]), g.inputs[0])
                else:
                    forms[id(g)] = ({}, g.inputs[0] * g.inputs[1])
            elif name == "mul":
                forms[id(g)] = ({n + g.mul_index: 1}, 0)
            else:
                raise ValueError(f"gate operation {name!r}")

        def csr(rows):
            ptr, col, vals, consts = [0], [], [], []
            for e, k in rows:
                for c in sorted(e):
                    col.append(c)
                    vals.append(int(e[c]))
                ptr.append(len(col))
                consts.append(int(k))
            return ptr, col, vals, consts

        muls = circuit.mul_gates()
        raw = {"A": [var_form(g.inputs[0]) for g in muls], "B": [var_form(g.inputs[1]) for g in muls],
               "O": [forms[id(circuit.gates[ix])] for ix in circuit.output_gates]}
        sc = cls(n, csr(raw["A"]), csr(raw["B"]), csr(raw["O"]), text=str(circuit), order=order)
        sc._raw = raw
        return sc

    def raw_forms(self):
        """{"A" | "B" | "O": [({col: coefficient}, constant)]} with the coefficients as Python objects: the builder's own
        (from_circuit), else the canonical residues as ints"""
        if self._raw is None:
            def rows(M):
                ints = [int.from_bytes(M.vals[i].tobytes(), "little") for i in range(len(M.col))]
                out = [({}, k) for k in M.const_ints()]
                for r, c, v in zip(M.rows.tolist(), M.col.tolist(), ints):
                    out[r][0][c] = v
                return out
            self._raw = {"A": rows(self.A), "B": rows(self.B), "O": rows(self.O)}
        return self._raw

    # ---- device state, made once ------------------------------------------------------------------------------------
    def device(self):
        if self._dev is None:
            ctx, V = get_context(), self.field.vector
            d = {"ctx": ctx, "A": sparse.DeviceMatrix(ctx, self.A, V), "B": sparse.DeviceMatrix(ctx, self.B, V),
                 "O": sparse.DeviceMatrix(ctx, self.O, V), "order": ctx.upload(self.level_order) if self.m else ctx.alloc(4)}
            K = 2 * self.m + 1
            d["fact"], d["ifact"] = V.empty(K + 1, ctx), V.empty(K + 1, ctx)
            ctx.cs_tables(K, d["fact"].ptr, d["ifact"].ptr, bn=self.field.bn)
            self._dev = d
        return self._dev


def as_sparse(circuit, order=ORDER):
    return circuit if isinstance(circuit, SparseCircuit) else SparseCircuit.from_circuit(circuit, order)


# ---- transcript ------------------------------------------------------------------------------------------------------------
def _mode(transcript):
    return compressed_pivot.transcript_mode(transcript, TRANSCRIPT)


class _Pedersen:
    """z is committed to by an Ed25519 vector commitment [z] = gamma h + sum_i z_i g_i; L is opened by the compressed
    or the plain pivot"""
    order = ORDER
    first_tag, second_tag = b"vmpc-ac20/p8/first/v1", b"vmpc-ac20/p8/second/v1"

    @staticmethod
    def commit(generators, z, gamma):
        return pivot.vector_commitment(z, gamma, generators["g"], generators["h"])

    @staticmethod
    def commit_batch(generators, Z, N, gammas):
        """([z_commitment], None) for the rows of Z: K queued commitments, read back together"""
        zs = [Z[p * N:(p + 1) * N] for p in range(len(gammas))]
        gv, h = pivot._points_on_device(generators["g"]), pivot._as_point(generators["h"])
        assert len(gv) >= N, "Not enough generators."
        pending = [pivot._commit_launch(z, gamma, gv, h, gv.ctx) for z, gamma in zip(zs, gammas)]
        return [pc.result() for pc in pending], None     # the first waits for all K, the others only copy

    @staticmethod
    def commitment_bytes(z_commitment):
        return wire.compress_point(z_commitment)


class _Koe:
    """z is committed to by the restriction argument over a pp: (P, pi), one G1 and one G2 MSM
    (knowledge_of_exponent.restriction_argument_prover); L is opened by the knowledge-of-exponent pivot.  N = len(z)
    needs 2N points on either side of the pp, the reference's assertion (knowledge_of_exponent.py:109,128).  K
    witnesses of one circuit (commit_batch) are the K rows of ONE staged matrix (gamma_p, z_p) and two row-MSMs
    (knowledge_of_exponent.restriction_argument_prover_batch); the matrix goes on to the batched opening, which
    multiplies the same rows."""
    order = BN256_ORDER
    first_tag, second_tag = b"vmpc-ac20/p8-koe/first/v1", b"vmpc-ac20/p8-koe/second/v1"

    @staticmethod
    def commit(generators, z, gamma):
        N = len(z)
        assert 2 * N - 1 <= len(generators["pp_lhs"]), \
            "Requirement does not hold: 2*len(x)-1 <= number of generators in first group."
        assert len(generators["pp_lhs"]) == 2 * N
        P, pi = koe.restriction_argument_prover(range(N), z, gamma, generators)
        return {"P": P, "pi": pi}

    @staticmethod
    def commit_batch(generators, Z, N, gammas):
        """([{"P", "pi"}], lhs) for the rows of Z; lhs: the staged rows (gamma_p, z_p), for the opening"""
        assert 2 * N - 1 <= len(generators["pp_lhs"]), \
            "Requirement does not hold: 2*len(x)-1 <= number of generators in first group."
        assert len(generators["pp_lhs"]) == 2 * N
        pairs, lhs = koe.restriction_argument_prover_batch(Z, gammas, generators, stride=N, n=N, return_lhs=True)
        return [{"P": P, "pi": pi} for P, pi in pairs], lhs

    @staticmethod
    def commitment_bytes(z_commitment):
        return z_commitment["P"].to_bytes() + z_commitment["pi"].to_bytes()


_KOE_REFERENCE_TRANSCRIPT = (
    "Protocol 8 with a knowledge-of-exponent pp: only the compact transcript is built.  The reference's own prover "
    "hashes the dict z_commitment where its verifier hashes the list [P, pi, ..] (circuit_sat_cb.py:107 against "
    ":189-194), so its two sides do not agree on the first challenge, and MPyC's repr of a BN-256 point - the text both "
    "would hash - is not pinned anywhere in this package")


def _scheme_of_commitment(z_commitment):
    return _Koe if isinstance(z_commitment, dict) else _Pedersen


def _scheme_of_generators(generators, circuit, gf):
    """the reference's dispatch (circuit_sat_cb.py:65-72): a pp selects the knowledge-of-exponent variant.  The field
    of gf and of the circuit must be the scheme's."""
    if "pp_lhs" in generators:
        scheme = _Koe
    elif "g" in generators:
        scheme = _Pedersen
    else:
        raise NotImplementedError("Protocol 8 over a SparseCircuit: generators are neither {'g', 'h', ..} nor a "
                                  "knowledge-of-exponent pp over BN-256")
    _check_field(scheme, circuit, gf)
    return scheme


def _check_field(scheme, circuit, gf):
    what = "the knowledge-of-exponent pp (BN-256)" if scheme is _Koe else "Ed25519 generators"
    if gf.order != scheme.order:
        raise ValueError(f"Protocol 8: gf.order is not the group order of {what}")
    if circuit.order != scheme.order:
        raise ValueError(f"Protocol 8: the circuit's order is not the group order of {what}: build the SparseCircuit "
                         f"with order=")


def _first_digest(z_commitment, circuit, n_in):
    scheme = _scheme_of_commitment(z_commitment)
    return hashlib.sha256(scheme.first_tag + scheme.commitment_bytes(z_commitment) + circuit.digest +
                          n_in.to_bytes(8, "little")).digest()


def first_challenge(digest, order):
    """the challenge c at which f, g, h are opened, from the first digest"""
    return int.from_bytes(digest, "little") % order


def _second_challenge(digest, ys, outputs, order, tag=_Pedersen.second_tag):
    h = hashlib.sha256(tag + digest)
    h.update(b"".join((int(v) % order).to_bytes(32, "little") for v in ys))
    h.update(len(outputs).to_bytes(4, "little") + b"".join((int(v) % order).to_bytes(32, "little") for v in outputs))
    return int.from_bytes(h.digest(), "little") % order


class ChallengeOnNode(ValueError):
    """the first challenge is one of the interpolation nodes 0..2m (probability about 2m / 2^252): the reference's
    _recombination_vectors divides by zero there"""


def _check_not_node(c, m):
    if 0 <= c <= 2 * m:
        raise ChallengeOnNode(f"Protocol 8: the first challenge {c} is an interpolation node (0..{2 * m})")


# ---- forms ---------------------------------------------------------------------------------------------------------------------
class _Forms:
    """the forms of f(c), g(c), h(c) over z, device-resident, and what L needs of them"""

    def __init__(self, circuit, n_in, c, order, k_out=None):
        """k_out: device memory of two scalars that takes the constants of F and G instead of the host, so that nothing
        waits here; the caller sets self.k once it has read them (the batch prover reads all witnesses' at once)"""
        d = circuit.device()
        ctx, m = d["ctx"], circuit.m
        assert order == circuit.order
        self.circuit, self.n_in, self.N, self.order, self.ctx = circuit, n_in, n_in + 3 + 2 * m, order, ctx
        N, Vec, bn = self.N, circuit.field.vector, circuit.field.bn
        self.lam = Vec.empty(m + 1, ctx)                         # nodes 0..m
        ctx.cs_lagrange(c, m, d["ifact"].ptr, self.lam.ptr, bn=bn)
        self.H = Vec.empty(N, ctx)                               # zeros, then the vector of the nodes 0..2m
        ctx.upload_into(self.H.ptr, np.zeros((n_in + 2, 32), np.uint8))
        ctx.cs_lagrange(c, 2 * m, d["ifact"].ptr, self.H.ptr + 32 * (n_in + 2), bn=bn)
        self.F, self.G = Vec.empty(N, ctx), Vec.empty(N, ctx)
        self.k = []
        for wire_ix, (M, V) in enumerate(((d["A"], self.F), (d["B"], self.G))):
            M.weighted_columns(self.lam.ptr + 32, circuit.n_x, n_in, V.ptr, N)
            ctx.copy(V.ptr + 32 * (n_in + wire_ix), self.lam.ptr, 32)
            if k_out is None:
                self.k.append(self.lam[1:].dot(M.consts) if m else 0)
            else:
                self.k.append(None)
                if m:
                    ctx.fr_dot_into(self.lam.ptr + 32, M.consts.ptr, m, k_out + 32 * wire_ix, bn=bn)
        self.k.append(0)

    def values(self, z):
        return [(V.dot(z) + k) % self.order for V, k in zip((self.F, self.G, self.H), self.k)]

    def combine(self, rho, ys, outputs, gf):
        """L = sum_k rho^k (O_k - out_k) + rho^n_out (F - y1) + rho^(n_out+1) (G - y2) + rho^(n_out+2) (H - y3)"""
        circuit, order = self.circuit, self.order
        n_out = circuit.n_out
        pw = [pow(rho, k, order) for k in range(n_out + 3)]
        Vec = circuit.field.vector
        co = Vec.empty(self.N, self.ctx)
        wts = Vec.from_ints(pw[:n_out], self.ctx)
        circuit.device()["O"].weighted_columns(wts.ptr, circuit.n_x, self.n_in, co.ptr, self.N)
        const = sum(p * (k - int(o)) for p, k, o in zip(pw, circuit.O.const_ints(), outputs))
        for V, k, y, p in zip((self.F, self.G, self.H), self.k, ys, pw[n_out:]):
            co = V.axpy(p, co)
            const += p * (k - int(y))
        return pivot.AffineForm(co, gf(const % order))


def _witness_on_device(circuit, x, order, gamma_witness=None):
    """z = (x, f(0), g(0), h(0), h(1..2m)) as a device vector; draws r_a, r_b from `prng`"""
    n_in, m, n_x = len(x), circuit.m, circuit.n_x
    d = circuit.device()
    ctx, F = d["ctx"], circuit.field
    assert order == F.order
    N = n_in + 3 + 2 * m
    z = F.vector.empty(N, ctx)
    ctx.upload_into(z.ptr, F.residues(x))
    r_a = prng.randrange(1, order)
    r_b = prng.randrange(1, order)
    a, b = F.vector.empty(m + 1, ctx), F.vector.empty(m + 1, ctx)
    ctx.upload_into(a.ptr + 32 * m, F.residues([r_a]))
    ctx.upload_into(b.ptr + 32 * m, F.residues([r_b]))
    g_off = n_in + 3
    if gamma_witness is not None:
        if len(gamma_witness) != m:
            raise ValueError(f"gamma_witness: {m} gate outputs expected")
        if m:
            ctx.upload_into(z.ptr + 32 * g_off, F.residues(gamma_witness))
            bad = ctx.alloc(4)
            ctx.cs_triples(d["A"].csr(), d["B"].csr(), None, m, n_x, g_off, z.ptr, a.ptr, b.ptr, 1, bad.ptr, bn=F.bn)
            first = int(ctx.download(bad.ptr, 4).view(np.uint32)[0])
            if first != 0xFFFFFFFF:
                raise ValueError(f"gamma_witness: multiplication gate {first} is not the product of its wires")
    else:
        for lv in range(len(circuit.level_ptr) - 1):
            lo, hi = int(circuit.level_ptr[lv]), int(circuit.level_ptr[lv + 1])
            ctx.cs_triples(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, n_x, g_off, z.ptr, a.ptr, b.ptr,
                           bn=F.bn)
    ctx.cs_extend(a.ptr, b.ptr, m, d["fact"].ptr, d["ifact"].ptr, z.ptr + 32 * n_in, bn=F.bn)
    return z


# ---- reference transcript (list mode) ----------------------------------------------------------------------------------------
# The two hashes are pivot.fiat_shamir_hash over the reference's lists (circuit_sat_cb.py:107-111, :149-162) with the
# reference's element types: the forms' coefficients are Python ints that are never reduced (circuit_builder.py:506-537
# multiplies the builder's ints by the Lagrange vectors, which recombine.py:31 returns as ints), constants turn into
# field elements where a field element is subtracted.  The text is O((n_out + 3) N), so this assembly is host code; the
# device computes z and the Lagrange vectors.  For parity, not for size.
FIRST_TAG = "First hash circuit satisfiability protocol"
SECOND_TAG = "Second hash circuit satisfiability protocol"


def _typed_forms(circuit, n_in, c):
    """(linform_f, linform_g, linform_h, circuit_forms) as list-mode forms, typed as the reference's"""
    d = circuit.device()
    ctx, m, n_x = d["ctx"], circuit.m, circuit.n_x
    N = n_in + 3 + 2 * m
    lam, lam2 = ScalarVector.empty(m + 1, ctx), ScalarVector.empty(2 * m + 1, ctx)
    ctx.cs_lagrange(c, m, d["ifact"].ptr, lam.ptr)
    ctx.cs_lagrange(c, 2 * m, d["ifact"].ptr, lam2.ptr)
    lam, lam2 = lam.to_ints(), lam2.to_ints()
    raw = circuit.raw_forms()

    def pos(col):
        return col if col < n_x else n_in + 3 + (col - n_x)

    fg = []
    for wire_ix, rows in enumerate((raw["A"], raw["B"])):
        co, const = [0] * N, 0
        for (e, k), l_j in zip(rows, lam[1:]):
            for col, v in e.items():
                co[pos(col)] = co[pos(col)] + v * l_j
            const = const + k * l_j
        co[n_in + wire_ix] = 1 * lam[0]
        fg.append(pivot.AffineForm(co, const))
    lh = pivot.LinearForm([0] * n_in + [0] * 2 + lam2)
    circuit_forms = []
    for e, k in raw["O"]:
        co = [0] * N
        for col, v in e.items():
            co[pos(col)] = v
        circuit_forms.append(pivot.AffineForm(co, k))
    return fg[0], fg[1], lh, circuit_forms


def _typed_outputs(circuit, x, z_ints, gf):
    """circuit(x) with the reference's typing: one field element among the inputs makes every gate value a field
    element (circuit_builder.py:133-172 sums c * v over ALL positions); all-int inputs leave exact, unreduced ints"""
    n_x, n_in = circuit.n_x, len(x)
    raw = circuit.raw_forms()
    if any(not isinstance(v, int) for v in x):
        gamma = [gf(v) for v in z_ints[n_in + 3:n_in + 3 + circuit.m]]
        pad = gf(0)
    else:
        gamma, pad = [], 0
        for (ea, ka), (eb, kb) in zip(raw["A"], raw["B"]):
            w = [sum(v * (x[c] if c < n_x else gamma[c - n_x]) for c, v in e.items()) + k for e, k in ((ea, ka), (eb, kb))]
            gamma.append(w[0] * w[1])
    return [sum(v * (x[c] if c < n_x else gamma[c - n_x]) for c, v in e.items()) + k + pad for e, k in raw["O"]]


def _reference_prover(generators, circuit, x, z, gf):
    order, n_in = gf.order, len(x)
    z_ints = z.to_ints()
    z_list = list(x) + [gf(v) for v in z_ints[n_in:]]
    gamma = prng.randrange(1, order)
    z_commitment = pivot.vector_commitment(z_list, gamma, generators["g"], generators["h"])
    proof = {"z_commitment": z_commitment}
    c = pivot.fiat_shamir_hash([z_commitment, circuit.text, FIRST_TAG], order)
    _check_not_node(c, circuit.m)
    lf, lg, lh, circuit_forms = _typed_forms(circuit, n_in, c)
    y1, y2, y3 = lf(z_list), lg(z_list), lh(z_list)
    assert y1 * y2 == y3
    proof["y1"], proof["y2"], proof["y3"] = y1, y2, y3
    outputs = _typed_outputs(circuit, x, z_ints, gf)
    proof["outputs"] = outputs
    lin_forms = [form - y for form, y in zip(circuit_forms, outputs)] + [lf - y1, lg - y2, lh - y3]
    rho = pivot.fiat_shamir_hash([y1, y2, y3, z_commitment, outputs, circuit_forms, lin_forms, SECOND_TAG], order)
    L = sum((linform_i) * (rho ** i) for i, linform_i in enumerate(lin_forms))
    proof["L"] = L
    return proof, z_commitment, L, z_list, gamma


def _reference_verifier(proof, circuit, gf, verification):
    order = gf.order
    N = len(proof["L"].coeffs)
    n_in = N - 3 - 2 * circuit.m
    outputs = proof["outputs"]
    if n_in < circuit.n_x or len(outputs) != circuit.n_out:
        verification["L_wellformed_from_Cfgh_forms"] = False
        return verification, None
    z_commitment = proof["z_commitment"]
    c = pivot.fiat_shamir_hash([z_commitment, circuit.text, FIRST_TAG], order)
    if 0 <= c <= 2 * circuit.m:
        verification["L_wellformed_from_Cfgh_forms"] = False
        return verification, None
    y1, y2, y3 = proof["y1"], proof["y2"], proof["y3"]
    lf, lg, lh, circuit_forms = _typed_forms(circuit, n_in, c)
    lin_forms = [form - y for form, y in zip(circuit_forms, outputs)] + [lf - y1, lg - y2, lh - y3]
    rho = pivot.fiat_shamir_hash([y1, y2, y3, z_commitment, outputs, circuit_forms, lin_forms, SECOND_TAG], order)
    L = sum((linform_i) * (rho ** i) for i, linform_i in enumerate(lin_forms))
    verification["L_wellformed_from_Cfgh_forms"] = bool(L == proof["L"])
    return verification, L


# ---- prover -----------------------------------------------------------------------------------------------------------------
def protocol_8_excl_pivot_prover(generators, circuit, x, gf, use_koe=False, gamma_witness=None, transcript=None):
    """circuit_sat_cb.py:59-166 for a SparseCircuit (anything else is converted): (proof, z_commitment, L, z, gamma) with
    z a device ScalarVector and L an AffineForm over device coefficients.  Random draws from `prng` in the reference's
    order: r_a, r_b, then gamma.  gamma_witness: the gate outputs, if the caller has them - they are checked (one
    launch) instead of computed (one launch per depth level)."""
    mode = _mode(transcript)
    if use_koe and "pp_lhs" not in generators:
        raise NotImplementedError("Protocol 8 over a SparseCircuit: the knowledge-of-exponent variant lives in another "
                                  "field (BN-256) and takes a pp (knowledge_of_exponent.trusted_setup) as generators")
    circuit = as_sparse(circuit, _Koe.order if "pp_lhs" in generators else ORDER)
    scheme = _scheme_of_generators(generators, circuit, gf)
    if scheme is _Koe and mode == "reference":
        raise NotImplementedError(_KOE_REFERENCE_TRANSCRIPT)
    order, F = gf.order, circuit.field
    n_in, m, n_x = len(x), circuit.m, circuit.n_x
    if n_in < n_x:
        raise ValueError(f"the circuit has {n_x} inputs, {n_in} given")
    z = _witness_on_device(circuit, x, order, gamma_witness)
    d = circuit.device()
    ctx, g_off = d["ctx"], n_in + 3
    if mode == "reference":
        return _reference_prover(generators, circuit, x, z, gf)

    gamma = prng.randrange(1, order)
    z_commitment = scheme.commit(generators, z, gamma)
    proof = {"z_commitment": z_commitment}
    digest = _first_digest(z_commitment, circuit, n_in)
    c = first_challenge(digest, order)
    _check_not_node(c, m)

    forms = _Forms(circuit, n_in, c, order)
    y1, y2, y3 = (gf(v) for v in forms.values(z))
    assert y1 * y2 == y3
    proof["y1"], proof["y2"], proof["y3"] = y1, y2, y3
    outputs = []
    if circuit.n_out:
        o1 = F.vector.empty(circuit.n_out, ctx)          # the kernel's two row sets are both O: one buffer takes both
        ctx.cs_triples(d["O"].csr(), d["O"].csr(), None, circuit.n_out, n_x, g_off, z.ptr, o1.ptr, o1.ptr, 2, bn=F.bn)
        outputs = [gf(v) for v in o1.to_ints()]
    proof["outputs"] = outputs
    rho = _second_challenge(digest, (y1, y2, y3), outputs, order, scheme.second_tag)
    L = forms.combine(rho, (y1, y2, y3), outputs, gf)
    proof["L"] = L
    return proof, z_commitment, L, z, gamma


def protocol_8_excl_pivot_verifier(proof, circuit, gf, use_koe=False, transcript=None):
    """circuit_sat_cb.py:169-252: (verification, L); O(nnz + N), nothing quadratic"""
    mode = _mode(transcript)
    scheme = _scheme_of_commitment(proof.get("z_commitment"))
    if use_koe and scheme is not _Koe:
        raise NotImplementedError("Protocol 8 over a SparseCircuit: a knowledge-of-exponent proof carries "
                                  "z_commitment = {'P', 'pi'} over BN-256")
    if scheme is _Koe and mode == "reference":
        raise NotImplementedError(_KOE_REFERENCE_TRANSCRIPT)
    circuit = as_sparse(circuit, scheme.order)
    _check_field(scheme, circuit, gf)
    order = gf.order
    verification = {}
    y1, y2, y3 = (int(proof[k]) % order for k in ("y1", "y2", "y3"))
    verification["y1*y2=y3"] = y1 * y2 % order == y3
    if not verification["y1*y2=y3"]:
        return verification, None
    if mode == "reference":
        return _reference_verifier(proof, circuit, gf, verification)
    N = len(proof["L"].coeffs)
    n_in = N - 3 - 2 * circuit.m
    outputs = proof["outputs"]
    if n_in < circuit.n_x or len(outputs) != circuit.n_out:
        verification["L_wellformed_from_Cfgh_forms"] = False
        return verification, None
    digest = _first_digest(proof["z_commitment"], circuit, n_in)
    c = first_challenge(digest, order)
    if 0 <= c <= 2 * circuit.m:
        # no honest prover sends this (ChallengeOnNode); no kernel is launched
        verification["L_wellformed_from_Cfgh_forms"] = False
        return verification, None
    forms = _Forms(circuit, n_in, c, order)
    rho = _second_challenge(digest, (y1, y2, y3), outputs, order, scheme.second_tag)
    L = forms.combine(rho, (y1, y2, y3), outputs, gf)
    theirs, F = proof["L"], circuit.field
    their_coeffs = theirs.coeffs if isinstance(theirs.coeffs, F.vector) else \
        F.vector.from_ints([F.residue(v) for v in theirs.coeffs], forms.ctx)
    same = int(theirs.constant) % order == int(L.constant) % order and \
        forms.ctx.cs_first_diff(L.coeffs.ptr, their_coeffs.ptr, N, bn=F.bn) is None
    verification["L_wellformed_from_Cfgh_forms"] = bool(same)
    return verification, L


def _choice(pivot_choice):
    return getattr(pivot_choice, "name", pivot_choice)


def _check_choice(choice, has_pp):
    """the pivot and the generators go together: koe with a pp over BN-256, the other two with Ed25519 generators"""
    if choice not in ("compressed", "pivot", "koe"):
        raise NotImplementedError
    if choice == "koe" and not has_pp:
        raise NotImplementedError("PivotChoice.koe over a SparseCircuit: the knowledge-of-exponent pivot lives in "
                                  "another field (BN-256) and takes a pp (knowledge_of_exponent.trusted_setup), a "
                                  "circuit of that order and GF(that order); these generators are Ed25519's")
    if choice != "koe" and has_pp:
        raise ValueError(f"PivotChoice.{choice} with a knowledge-of-exponent pp: a pp goes with PivotChoice.koe")


def circuit_sat_prover(generators, circuit, x, gf, pivot_choice="compressed", gamma_witness=None, transcript=None):
    """circuit_sat_cb.py:255-282 for a SparseCircuit, wholly in this package"""
    choice = _choice(pivot_choice)
    _check_choice(choice, "pp_lhs" in generators)
    mode = _mode(transcript)
    proof, z_commitment, L, z, gamma = protocol_8_excl_pivot_prover(generators, circuit, x, gf,
                                                                    gamma_witness=gamma_witness, transcript=mode)
    if choice == "koe":
        # L(z) = 0 is the opening's own coefficient N: nothing is evaluated here, z and L stay on the device
        proof["pivot_proof"] = koe.opening_linear_form_prover(L, z, gamma, generators, z_commitment["P"],
                                                              z_commitment["pi"])[0]
        return proof
    y = L(z)
    if choice == "compressed":
        r = compressed_pivot.masks(len(z), L.coeffs.ctx) if isinstance(z, ScalarVector) and \
            len(z) >= compressed_pivot.MASKS_ON_DEVICE_MIN else None
        proof["pivot_proof"] = compressed_pivot.protocol_5_prover(generators, z_commitment, L, y, z, gamma, gf,
                                                                  transcript=mode, r=r)
    else:
        # Protocol 2 is the O(N)-proof pivot and has no device prover: its response IS a vector of N scalars
        zs = z if isinstance(z, list) else [gf(v) for v in z.to_ints()]
        proof["pivot_proof"] = pivot.prove_linear_form_eval(generators["g"], generators["h"], z_commitment, L, y, zs,
                                                            gamma, gf)
    return proof


def circuit_sat_verifier(proof, generators, circuit, gf, pivot_choice="compressed", transcript=None):
    """circuit_sat_cb.py:285-318 for a SparseCircuit: the verification dict"""
    choice = _choice(pivot_choice)
    _check_choice(choice, "pp_lhs" in generators)
    mode = _mode(transcript)
    if (choice == "koe") != isinstance(proof.get("z_commitment"), dict):
        raise ValueError("circuit_sat_verifier: a knowledge-of-exponent proof (z_commitment = {'P', 'pi'}) goes with "
                         "PivotChoice.koe and a pp, any other proof with Ed25519 generators")
    verification, L = protocol_8_excl_pivot_verifier(proof, circuit, gf, transcript=mode)
    if L is None:
        return verification
    if choice == "koe":
        # a proof whose L is not the forms' combination is rejected already: the opening (two MSMs, five Miller loops)
        # is not run against the verifier's own L, and every key that is False names what was wrong
        if not verification["L_wellformed_from_Cfgh_forms"]:
            return verification
        # the opening is checked on the (P, pi) that the first challenge was drawn from: a pivot proof that names
        # other points than the commitment fails the restriction check
        zc, pp_proof = proof["z_commitment"], proof["pivot_proof"]
        bound = all(pp_proof[k].to_bytes() == zc[k].to_bytes() for k in ("P", "pi"))
        ok = koe.opening_linear_form_verifier(L, generators, {"P": zc["P"], "pi": zc["pi"], "Q": pp_proof["Q"]}, 0)
        ok["restriction_arg_check"] = bool(ok["restriction_arg_check"] and bound)
        verification["pivot_verification"] = ok
        return verification
    if choice == "compressed":
        ok = compressed_pivot.protocol_5_verifier(generators, proof["z_commitment"], L, gf(0), proof["pivot_proof"], gf,
                                                  transcript=mode)
    else:
        z, phi, c = proof["pivot_proof"]
        ok = pivot.verify_linear_form_proof(generators["g"], generators["h"], proof["z_commitment"], L, gf(0), z, phi, c)
    verification["pivot_verification"] = ok
    return verification


def circuit_sat_verifier_batch(proofs, generators, circuit, gf, transcript=None, pivot_choice=None):
    """[circuit_sat_verifier(proof, generators, circuit, gf, pivot_choice, transcript) for proof in proofs] - many inputs
    of one circuit: Protocol 8's checks per proof, then the proofs that yielded an L in ONE batched pivot verification.
    pivot_choice None: by the generators - a pp selects the knowledge-of-exponent pivot
    (knowledge_of_exponent.opening_linear_form_verifier_batch), Ed25519 generators the compressed
    one (compressed_pivot.protocol_5_verifier_batch); "pivot" has no batch form."""
    has_pp = "pp_lhs" in generators
    choice = ("koe" if has_pp else "compressed") if pivot_choice is None else _choice(pivot_choice)
    _check_choice(choice, has_pp)
    if choice == "koe":
        return _koe_verifier_batch(proofs, generators, circuit, gf, _mode(transcript))
    if choice != "compressed":
        raise NotImplementedError("circuit_sat_verifier_batch: the compressed and the knowledge-of-exponent pivot")
    mode = _mode(transcript)
    circuit = as_sparse(circuit)
    out, statements, where = [], [], []
    for proof in proofs:
        verification, L = protocol_8_excl_pivot_verifier(proof, circuit, gf, transcript=mode)
        if L is not None:
            statements.append((proof["z_commitment"], L, gf(0), proof["pivot_proof"]))
            where.append(len(out))
        out.append(verification)
    for i, ok in zip(where, compressed_pivot.protocol_5_verifier_batch(generators, statements, gf, transcript=mode)):
        out[i]["pivot_verification"] = ok
    return out


# bytes of linear forms L (32 N each) that the knowledge-of-exponent route of circuit_sat_verifier_batch keeps alive at a
# time: the proofs are consumed in chunks of that many, one batched opening per chunk
KOE_VERIFY_BUDGET_BYTES = 1 << 28


def _koe_verifier_batch(proofs, pp, circuit, gf, mode):
    """circuit_sat_verifier(.., PivotChoice.koe) proof for proof, up to L; then one opening batch per chunk of proofs"""
    out, chunk, held = [], [], 0

    def flush():
        # (L, proof points, bound, index) of the chunk's proofs that got as far as the opening; one batch per length of
        # L (an honest batch of one circuit has one)
        by_len = {}
        for item in chunk:
            by_len.setdefault(len(item[0].coeffs), []).append(item)
        for items in by_len.values():
            oks = koe.opening_linear_form_verifier_batch([L for L, _, _, _ in items], pp, [pts for _, pts, _, _ in items],
                                                         [0] * len(items))
            for (_, _, bound, i), ok in zip(items, oks):
                ok["restriction_arg_check"] = bool(ok["restriction_arg_check"] and bound)
                out[i]["pivot_verification"] = ok
        chunk.clear()

    for proof in proofs:
        if not isinstance(proof.get("z_commitment"), dict):
            raise ValueError("circuit_sat_verifier: a knowledge-of-exponent proof (z_commitment = {'P', 'pi'}) goes with "
                             "PivotChoice.koe and a pp, any other proof with Ed25519 generators")
        nbytes = 32 * len(proof["L"].coeffs)
        if held and held + nbytes > KOE_VERIFY_BUDGET_BYTES:
            flush()
            held = 0
        held += nbytes
        verification, L = protocol_8_excl_pivot_verifier(proof, circuit, gf, transcript=mode)
        out.append(verification)
        if L is None or not verification["L_wellformed_from_Cfgh_forms"]:
            continue
        # as in circuit_sat_verifier: the opening is checked on the commitment's (P, pi); a pivot proof that names other
        # points fails the restriction check
        zc, pp_proof = proof["z_commitment"], proof["pivot_proof"]
        bound = all(pp_proof[k].to_bytes() == zc[k].to_bytes() for k in ("P", "pi"))
        chunk.append((L, {"P": zc["P"], "pi": zc["pi"], "Q": pp_proof["Q"]}, bound, len(out) - 1))
    flush()
    return out


# ---- K witnesses of one circuit -------------------------------------------------------------------
# what one chunk of a batch may hold in Z, the row values and the extension's workspace
BATCH_BUDGET_BYTES = 1 << 30
MAX_BATCH = 65535           # VMPC_FR_CS_MAX_WIT of include/vmpc.h


def _batch_inputs(xs, n_in, field=_FIELDS[ORDER]):
    """(K, n_in, rows): rows a (K, n_in, 32) uint8 array of canonical residues of `field`, or the caller's device vector
    (the field's: ScalarVector / BnScalarVector) of K n_in scalars.  Only a sequence of input lists is converted integer
    by integer."""
    if isinstance(xs, ScalarVector):
        if xs.BN != field.bn:
            raise ValueError(f"xs on the device: a {field.vector.__name__} goes with this circuit's order")
        if n_in is None:
            raise ValueError("xs on the device: n_in= says where a witness ends")
        if (n_in == 0 and len(xs)) or (n_in and len(xs) % n_in):
            raise ValueError(f"xs holds {len(xs)} scalars, not a multiple of n_in = {n_in}")
        return (len(xs) // n_in if n_in else 0), n_in, xs
    if isinstance(xs, np.ndarray) and xs.dtype == np.uint8:
        if xs.ndim != 3 or xs.shape[2] != 32:
            raise ValueError("xs as an array: (K, n_in, 32) uint8 little-endian residues")
        rows = np.ascontiguousarray(xs)
        # only values whose top byte reaches the order's may not be canonical (l < 2^253: 0x10)
        big = np.argwhere(rows[:, :, 31] >= field.order >> 248)
        if len(big):
            rows = rows.copy()
            for p, i in big.tolist():
                v = int.from_bytes(rows[p, i].tobytes(), "little") % field.order
                rows[p, i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        return rows.shape[0], rows.shape[1], rows
    xs = [list(x) for x in xs]
    if not xs:
        return 0, 0, np.zeros((0, 0, 32), np.uint8)
    if any(len(x) != len(xs[0]) for x in xs):
        raise ValueError("xs: every witness takes the same number of inputs")
    rows = [field.residues(x).reshape(len(xs[0]), 32) for x in xs]
    return len(xs), len(xs[0]), np.stack(rows)


def _input_lists(xs, n_in):
    """xs as K lists of Python values, for the paths that are host list code"""
    if isinstance(xs, ScalarVector):
        K, n_in, _ = _batch_inputs(xs, n_in)
        flat = xs.to_ints()
        return [flat[p * n_in:(p + 1) * n_in] for p in range(K)]
    if isinstance(xs, np.ndarray) and xs.dtype == np.uint8:
        K, n_in, rows = _batch_inputs(xs, n_in)
        return [[int.from_bytes(rows[p, i].tobytes(), "little") for i in range(n_in)] for p in range(K)]
    return [list(x) for x in xs]


def _batch_bytes(circuit, n_in, k):
    """device bytes of k witnesses' Z, row values and extension workspace"""
    m = circuit.m
    return 32 * k * (n_in + 3 + 2 * m + 2 * (m + 1)) + circuit.device()["ctx"].cs_extend_batch_bytes(m, k, bn=circuit.field.bn)


def _chunk_size(circuit, n_in, K):
    """the most witnesses (<= K) whose _batch_bytes stay within BATCH_BUDGET_BYTES, at least one"""
    lo, hi = 1, min(K, MAX_BATCH)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _batch_bytes(circuit, n_in, mid) <= BATCH_BUDGET_BYTES:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _witnesses_on_device(circuit, rows, n_in, draws, gamma_witnesses=None, first=0):
    """Z: the K = len(draws) vectors z of _witness_on_device as consecutive rows of ONE device vector (stride N) of the
    circuit's field, for the inputs `rows` (host array or device vector from witness 0 on) and draws [(r_a, r_b, ..)].
    Every stage runs once for all K; `first` is only what an error calls witness 0."""
    K, m, n_x = len(draws), circuit.m, circuit.n_x
    d = circuit.device()
    ctx, F = d["ctx"], circuit.field
    Vec, bn = F.vector, F.bn
    M, N, g_off = m + 1, n_in + 3 + 2 * m, n_in + 3
    Z = Vec.empty(K * N, ctx)
    a, b = Vec.empty(K * M, ctx), Vec.empty(K * M, ctx)
    X = rows if isinstance(rows, ScalarVector) else Vec.from_array(rows.reshape(K * n_in, 32), ctx)
    r = ctx.upload(F.residues([dr[0] for dr in draws] + [dr[1] for dr in draws]))
    G = None
    if gamma_witnesses is not None and m:
        G = ctx.upload(F.residues([v for gw in gamma_witnesses for v in gw]))
    for p in range(K):
        ctx.copy(Z.ptr + 32 * p * N, X.ptr + 32 * p * n_in, 32 * n_in)
        ctx.copy(a.ptr + 32 * (p * M + m), r.ptr + 32 * p, 32)
        ctx.copy(b.ptr + 32 * (p * M + m), r.ptr + 32 * (K + p), 32)
        if G is not None:
            ctx.copy(Z.ptr + 32 * (p * N + g_off), G.ptr + 32 * p * m, 32 * m)
    if G is not None:
        bad = ctx.alloc(4 * K)
        ctx.cs_triples_batch(d["A"].csr(), d["B"].csr(), None, m, n_x, g_off, Z.ptr, N, a.ptr, b.ptr, M, K, 1, bad.ptr,
                             bn=bn)
        firsts = ctx.download(bad.ptr, 4 * K).view(np.uint32)
        for p in np.nonzero(firsts != 0xFFFFFFFF)[0][:1].tolist():
            raise ValueError(f"gamma_witnesses[{first + p}]: multiplication gate {int(firsts[p])} is not the product of "
                             f"its wires")
    elif gamma_witnesses is None:
        for lv in range(len(circuit.level_ptr) - 1):
            lo, hi = int(circuit.level_ptr[lv]), int(circuit.level_ptr[lv + 1])
            ctx.cs_triples_batch(d["A"].csr(), d["B"].csr(), d["order"].ptr + 4 * lo, hi - lo, n_x, g_off, Z.ptr, N, a.ptr,
                                 b.ptr, M, K, bn=bn)
    ctx.cs_extend_batch(a.ptr, b.ptr, M, m, d["fact"].ptr, d["ifact"].ptr, Z.ptr + 32 * n_in, N, K, bn=bn)
    return Z


def _prove_chunk(generators, circuit, rows, n_in, draws, gamma_witnesses, gf, first):
    """Protocol 8 without the pivot for the witnesses of one chunk, stage by stage; nothing is read back inside a loop
    over witnesses.  (results, Z, staged): the chunk's matrix Z and what the scheme's commit_batch staged besides the
    commitments (the knowledge-of-exponent rows (gamma_p, z_p); None for Ed25519), for the pivot that follows."""
    order, K, m, n_x, n_out = gf.order, len(draws), circuit.m, circuit.n_x, circuit.n_out
    d = circuit.device()
    ctx, N, g_off = d["ctx"], n_in + 3 + 2 * m, n_in + 3
    Vec, bn = circuit.field.vector, circuit.field.bn
    scheme = _Koe if "pp_lhs" in generators else _Pedersen
    Z = _witnesses_on_device(circuit, rows, n_in, draws, gamma_witnesses, first)
    zs = [Z[p * N:(p + 1) * N] for p in range(K)]           # views: each keeps the allocation alive
    commitments, staged = scheme.commit_batch(generators, Z, N, [dr[2] for dr in draws])
    digests = [_first_digest(zc, circuit, n_in) for zc in commitments]
    cs = [first_challenge(dg, order) for dg in digests]
    for p, c in enumerate(cs):
        if 0 <= c <= 2 * m:
            raise ChallengeOnNode(f"Protocol 8, witness {first + p}: the first challenge {c} is an interpolation node "
                                  f"(0..{2 * m})")
    # per witness F z, G z, H z and the constants of F and G: five scalars, read back together
    Y = Vec.empty(5 * K, ctx)
    forms = []
    for p, (z, c) in enumerate(zip(zs, cs)):
        f = _Forms(circuit, n_in, c, order, Y.ptr + 32 * (5 * p + 3))
        for i, V in enumerate((f.F, f.G, f.H)):
            ctx.fr_dot_into(V.ptr, z.ptr, N, Y.ptr + 32 * (5 * p + i), bn=bn)
        forms.append(f)
    o1 = None
    if n_out:
        o1 = Vec.empty(K * n_out, ctx)
        ctx.cs_triples_batch(d["O"].csr(), d["O"].csr(), None, n_out, n_x, g_off, Z.ptr, N, o1.ptr, o1.ptr, n_out, K, 2,
                             bn=bn)
    ys = Y.to_ints()
    outs = o1.to_ints() if n_out else []
    results = []
    for p, (z, zc, f, dg, dr) in enumerate(zip(zs, commitments, forms, digests, draws)):
        f.k = [ys[5 * p + 3], ys[5 * p + 4], 0] if m else [0, 0, 0]
        y1, y2, y3 = (gf((v + k) % order) for v, k in zip(ys[5 * p:5 * p + 3], f.k))
        assert y1 * y2 == y3
        proof = {"z_commitment": zc, "y1": y1, "y2": y2, "y3": y3}
        outputs = [gf(v) for v in outs[p * n_out:(p + 1) * n_out]]
        proof["outputs"] = outputs
        rho = _second_challenge(dg, (y1, y2, y3), outputs, order, scheme.second_tag)
        L = f.combine(rho, (y1, y2, y3), outputs, gf)
        proof["L"] = L
        results.append((proof, zc, L, z, dr[2]))
    return results, Z, staged


def _prove_chunks(generators, circuit, xs, gf, gamma_witnesses, mode, n_in):
    """protocol_8_excl_pivot_prover_batch's checks and draws, then one _prove_chunk per chunk of witnesses: yields what
    _prove_chunk returns.  The compact transcript only."""
    has_pp = "pp_lhs" in generators
    circuit = as_sparse(circuit, _Koe.order if has_pp else ORDER)
    scheme = _scheme_of_generators(generators, circuit, gf)
    if scheme is _Koe and mode == "reference":
        raise NotImplementedError(_KOE_REFERENCE_TRANSCRIPT)
    assert mode != "reference"
    order = gf.order
    K, n_in, rows = _batch_inputs(xs, n_in, circuit.field)
    if K == 0:
        return
    if n_in < circuit.n_x:
        raise ValueError(f"the circuit has {circuit.n_x} inputs, {n_in} given")
    if gamma_witnesses is not None:
        gamma_witnesses = [list(gw) for gw in gamma_witnesses]
        if len(gamma_witnesses) != K or any(len(gw) != circuit.m for gw in gamma_witnesses):
            raise ValueError(f"gamma_witnesses: {K} lists of {circuit.m} gate outputs expected")
    draws = [(prng.randrange(1, order), prng.randrange(1, order), prng.randrange(1, order)) for _ in range(K)]
    step = _chunk_size(circuit, n_in, K)
    for lo in range(0, K, step):
        hi = min(K, lo + step)
        part = rows[lo * n_in:hi * n_in] if isinstance(rows, ScalarVector) else rows[lo:hi]
        yield _prove_chunk(generators, circuit, part, n_in, draws[lo:hi],
                           gamma_witnesses[lo:hi] if gamma_witnesses is not None else None, gf, lo)


def protocol_8_excl_pivot_prover_batch(generators, circuit, xs, gf, gamma_witnesses=None, transcript=None, n_in=None):
    """[protocol_8_excl_pivot_prover(generators, circuit, x, gf, ...) for x in xs] for K inputs of ONE circuit, with the
    random draws those K calls would make (r_a, r_b, gamma of witness 0, then witness 1, ..: all before the first launch)
    and so the same proofs - but every stage once for all K: one launch per depth level, one batched extension, the K
    commitments together, K queued sets of forms whose values are read back together.

    The generators select the scheme and the field as in the single prover: Ed25519 generators commit by K queued
    vector commitments read back together; a knowledge-of-exponent pp (a circuit and gf of the BN-256 order, the compact
    transcript only) by ONE restriction_argument_prover_batch on the rows of Z - one staged matrix, one row-MSM in G1
    and one on the twist.

    xs: K input lists of one length; a (K, n_in, 32) uint8 array of little-endian residues; or a device vector of the
    circuit's field (ScalarVector, BnScalarVector) of K n_in scalars with n_in=.  gamma_witnesses: K lists of gate
    outputs, checked in one launch.  Each returned z is a slice of one device vector.  K is cut into chunks of at most
    BATCH_BUDGET_BYTES of Z, row values and workspace."""
    mode = _mode(transcript)
    if mode == "reference":             # host list code by construction
        if "pp_lhs" in generators:
            raise NotImplementedError(_KOE_REFERENCE_TRANSCRIPT)
        _scheme_of_generators(generators, as_sparse(circuit), gf)
        lists = _input_lists(xs, n_in)
        gws = gamma_witnesses if gamma_witnesses is not None else [None] * len(lists)
        return [protocol_8_excl_pivot_prover(generators, circuit, x, gf, gamma_witness=gw, transcript=mode)
                for x, gw in zip(lists, gws)]
    return [r for results, _, _ in _prove_chunks(generators, circuit, xs, gf, gamma_witnesses, mode, n_in) for r in results]


def circuit_sat_prover_batch(generators, circuit, xs, gf, pivot_choice="compressed", gamma_witnesses=None, transcript=None,
                             n_in=None):
    """[circuit_sat_prover(generators, circuit, x, gf, pivot_choice, ...) for x in xs]: Protocol 8 for all K witnesses
    together (protocol_8_excl_pivot_prover_batch), then the pivot.  The compressed pivot runs per witness, in order.
    The knowledge-of-exponent pivot (a pp, PivotChoice.koe) is ONE opening_linear_form_prover_batch per chunk of
    witnesses on the commitments' P and pi and on the rows the commitment staged: one product, one split and one
    row-MSM for the chunk, z and L on the device throughout.  The plain pivot and the reference
    transcript are host list code: a loop over circuit_sat_prover."""
    choice = _choice(pivot_choice)
    _check_choice(choice, "pp_lhs" in generators)
    mode = _mode(transcript)
    if choice == "koe":
        if mode == "reference":
            raise NotImplementedError(_KOE_REFERENCE_TRANSCRIPT)
        proofs = []
        for results, _, lhs in _prove_chunks(generators, circuit, xs, gf, gamma_witnesses, mode, n_in):
            # L(z) = 0 is each opening's own coefficient N: nothing is evaluated here
            opened = koe.opening_linear_form_prover_batch([L for _, _, L, _, _ in results], None,
                                                          [gamma for _, _, _, _, gamma in results], generators,
                                                          [zc["P"] for _, zc, _, _, _ in results],
                                                          [zc["pi"] for _, zc, _, _, _ in results], lhs=lhs)
            for (proof, _, _, _, _), (pivot_proof, _) in zip(results, opened):
                proof["pivot_proof"] = pivot_proof
                proofs.append(proof)
        return proofs
    if choice == "pivot" or mode == "reference":
        lists = _input_lists(xs, n_in)
        gws = gamma_witnesses if gamma_witnesses is not None else [None] * len(lists)
        return [circuit_sat_prover(generators, circuit, x, gf, pivot_choice, gamma_witness=gw, transcript=mode)
                for x, gw in zip(lists, gws)]
    proofs = []
    for proof, z_commitment, L, z, gamma in protocol_8_excl_pivot_prover_batch(generators, circuit, xs, gf,
                                                                               gamma_witnesses, mode, n_in):
        y = L(z)
        r = compressed_pivot.masks(len(z), L.coeffs.ctx) if len(z) >= compressed_pivot.MASKS_ON_DEVICE_MIN else None
        proof["pivot_proof"] = compressed_pivot.protocol_5_prover(generators, z_commitment, L, y, z, gamma, gf,
                                                                  transcript=mode, r=r)
        proofs.append(proof)
    return proofs
