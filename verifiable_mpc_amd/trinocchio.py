"""Counterpart of demos/demo_zkp_trinocchio.py (Trinocchio, Schoenmakers, Veeningen and de Vreede, eprint 2015/480): M
parties hold Shamir shares of a QAP witness, each computes a Pinocchio proof SHARE on its MI355X, and the shares are
recombined in the exponent into one proof that the ordinary `pynocchio.verify` accepts.

    c_shares, h_shares            demo_zkp_trinocchio.py:70-79   (h computed in the clear, then shared)
    compute_proof on the shares   demo_zkp_trinocchio.py:80      pynocchio.compute_proof, unchanged
    recombination                 demo_zkp_trinocchio.py:86-93   proof[key] = sum_p lambda_p * share_p[key]
    c_client                      demo_zkp_trinocchio.py:96-98   [1] + opened I/O wires

What differs from the demo: h is never known to anybody.  Each party computes `pynocchio.compute_h_share` on its own
share vector - the polynomial part of V W / t, bilinear in the shares, so a degree-2t sharing of h that M >= 2t + 1
parties recombine - and masks it with a fresh degree-2t sharing of zero before anything that
depends on it leaves the party.  The zero-knowledge deltas the demo leaves as a TODO are degree-t shared randomness and
ride along.  Whether the SHARED witness satisfies the constraints - the remainder of p / qap.t, which the demo drops
unchecked - is a random linear combination of the rows' residuals (vmpc_bn256_qap_residual_dev), masked and opened.

The share arithmetic is GF(n), n the BN-256 group order: `Runtime` is mpc_ac20.PartyRuntime's hub, tags and exchange of
bytes over csrc/mpc_share.hip's GF(n) entries.  A party exchanges (section 19 has the argument):

    check      1. the dealt randomness (deltas, rho) and sharings of zero   2. rho opened   3. the masked residual opened
    always     (1. as above, when there is anything to deal)   then ONE exchange of the eight proof-share points with
               the shares of the I/O wires

so 4 exchanges with the check and 2 without (1 when there is nothing to deal: no deltas and an empty h).

    shares of the inputs only     demo_zkp_trinocchio.py:42,70   calculate_witness_shares, prove_inputs

`prove` starts from shares of the WHOLE witness (as with `gamma_witness=` in mpc_circuit_sat).  `calculate_witness_shares`
makes them from shares of the inputs alone, as the demo's qap.calculate_witness on secure values does: the rows that
need no communication run locally, every multiplicative depth of the circuit costs one more exchange (DESIGN.md
section 23), and `prove_inputs` is the two in a row.  In the clear the witness comes from pynocchio.calculate_witness /
calculate_witness_batch.

    K witnesses of one QAP        prove_batch, prove_inputs_batch

`prove_batch` is `prove` for K witnesses in the SAME exchanges: one deal round, rho opened once, the K masked residuals
opened together, one exchange of the 8 K proof-share points.  There is one prover body, `_prove`: `prove` runs it on a
batch of one, and `prove_inputs` / `prove_inputs_batch` are calculate_witness_shares followed by it.  The recombination in the exponent - of one proof or of K -
is one vmpc_bn256_recombine_dev launch per group (`Runtime.recombine_points`, csrc/bn256_recombine.hip).

Out of scope:
  * a division by a shared value in the witness computation on shares (it needs an inversion protocol with two more
    exchanges; pynocchio.ShareSolvePlan refuses such a circuit), inputs that are partly public, and parties that
    deviate from the protocol;
  * QAP construction from code (stays with the reference, as for pynocchio);
  * multi-client Trinocchio (the paper's Alg. 4);
  * any transport other than the hub: a real runtime moves the same bytes.
"""
import time
import types

import numpy as np

from . import _native
from . import pynocchio as pn
from .device import ScalarVector, get_context
from .mpc_ac20 import LocalHub, PartyRuntime

ORDER = pn.ORDER
_ORDER_BE = np.frombuffer(ORDER.to_bytes(32, "big"), np.uint8).astype(np.int16)


def recombination_vector(xs, x_r=0):
    """Lagrange coefficients for the nodes xs at x_r, mod n (mpyc.thresha._recombination_vector as
    demo_zkp_trinocchio.py:88 calls it)."""
    out = []
    for i, x_i in enumerate(xs):
        num = den = 1
        for j, x_j in enumerate(xs):
            if i != j:
                num = num * (x_r - x_j) % ORDER
                den = den * (x_i - x_j) % ORDER
        out.append(num * pow(den, ORDER - 2, ORDER) % ORDER)
    return out


def random_residues(rng, count):
    """(count, 32) uint8 uniform residues mod n from `rng`: 256-bit draws, those >= n rejected (n is 0.56 x 2^256, so
    reducing instead would make the low residues twice as likely)"""
    out = np.zeros((0, 32), np.uint8)
    while len(out) < count:
        k = 2 * (count - len(out)) + 16
        arr = np.frombuffer(rng.getrandbits(256 * k).to_bytes(32 * k, "little"), np.uint8).reshape(k, 32)
        diff = arr[:, ::-1].astype(np.int16) - _ORDER_BE          # most significant byte first
        first = (diff != 0).argmax(axis=1)
        below = diff[np.arange(k), first] < 0                     # (a row equal to n has diff 0 everywhere: rejected)
        out = np.concatenate([out, arr[below]])
    return np.ascontiguousarray(out[:count])


class Runtime(PartyRuntime):
    """PartyRuntime over GF(n): pid in 0..M-1 holds the share at x = pid + 1.  Share vectors are device vectors of
    32-byte residues (device.ScalarVector used as a container: its arithmetic is GF(l) and is not used here).
    A product of two degree-t sharings - h is one - has degree 2t, which M parties recombine only if 2t < M: anything
    else is refused here, before a context exists."""

    def __init__(self, pid=0, parties=1, threshold=0, rng=None, hub=None, ctx=None):
        if 2 * threshold >= parties:
            raise ValueError(f"trinocchio: h is a degree-{2 * threshold} sharing, which {parties} parties cannot "
                             f"recombine (2 t < M)")
        super().__init__(pid, parties, threshold, rng, hub)
        self.gf = None                                              # opened values are plain ints mod n
        self.weights = recombination_vector(list(range(1, parties + 1)))
        self.lagrange = self.weights[pid]
        self.exchanges = 0
        self.stage_log = None               # a list: prove appends (stage, seconds), each ended by a synchronisation
        self._ctx = ctx

    def _context(self):
        return self._ctx or get_context()

    def _stage(self, name, t0):
        """scripts/trinocchio_probe.py's bracket: the local work since t0 belongs to `name`; -> the new t0"""
        if self.stage_log is not None:
            self._context().sync()
            self.stage_log.append((name, time.perf_counter() - t0))
        return time.perf_counter()

    def _next_tag(self, kind):
        self.exchanges += 1                 # every exchange draws exactly one tag
        return super()._next_tag(kind)

    # what the GF(l) class does with l's arithmetic has no meaning here
    def _random(self, sectype=None):
        raise NotImplementedError("trinocchio.Runtime: use random_shares")

    async def schur_prod(self, a, b, out=None, dst=None):
        raise NotImplementedError("trinocchio.Runtime: no product of shares is needed for a Pinocchio proof")

    def _dealt(self, values, n, degree, ctx):
        """fresh degree-`degree` sharings of the n device scalars `values` (None: of zero) -> (M, n, 32) host table"""
        M = self.parties
        a = values if values is not None else ctx.upload(np.zeros((n, 32), np.uint8))
        coeffs = ctx.upload(random_residues(self.rng, degree * n)) if degree else None
        out = ctx.alloc(32 * M * n)
        ctx.bn256_share_mul_deal(a.ptr, None, n, coeffs.ptr if degree else None, degree, M, out.ptr, n)
        return ctx.download(out.ptr, 32 * M * n, (M, n, 32))

    async def _deal_round(self, n_rand, n_zero):
        """ONE exchange that carries both kinds of dealt randomness: every party deals n_rand random values of its own
        with degree t and n_zero zeros with degree 2t.  -> (the n_rand random shares, combined: a ScalarVector;
        the n_zero zero sharings as RECEIVED, an M x n_zero device matrix still to be added up - the combination that
        adds them takes the value to be masked as its addend, see `masked`)"""
        ctx, M, n = self._context(), self.parties, n_rand + n_zero
        if n == 0:
            return ScalarVector.empty(0, ctx), None
        t0 = time.perf_counter()
        tables = []
        if n_rand:
            tables.append(self._dealt(ctx.upload(random_residues(self.rng, n_rand)), n_rand, self.threshold, ctx))
        if n_zero:
            tables.append(self._dealt(None, n_zero, 2 * self.threshold, ctx))
        table = np.concatenate(tables, axis=1)
        self._stage("masks", t0)
        got = await self.exchange_vectors([table[q] for q in range(M)])
        t0 = time.perf_counter()
        parts = ctx.upload(np.ascontiguousarray(np.stack(got)))            # M x n
        rand = ScalarVector.empty(n_rand, ctx)
        if n_rand:
            ctx.bn256_share_combine(parts.ptr, M, n_rand, n, [1] * M, None, None, rand.ptr)
        self._stage("masks", t0)
        return rand, (_Zeros(parts, n_rand, n_zero, n) if n_zero else None)

    def masked(self, zeros, first, values_ptr, n):
        """the n device scalars at values_ptr + the zero sharings first .. first + n - 1 of a `_deal_round`, in one
        combination: the unmasked values are its addend and go nowhere else (values_ptr None: the zero shares alone)"""
        ctx = self._context()
        out = ScalarVector.empty(n, ctx)
        if n:
            assert first + n <= zeros.n
            ctx.bn256_share_combine(zeros.parts.ptr + 32 * (zeros.offset + first), self.parties, n, zeros.stride,
                                    [1] * self.parties, None, values_ptr, out.ptr)
        return out

    async def random_shares(self, n):
        """n uniformly random secrets nobody knows, shared with degree `threshold`"""
        return (await self._deal_round(n, 0))[0]

    async def zero_shares(self, n):
        """n degree-2t sharings of zero: every party deals zeros with the degree argument 2t, one exchange, the sum of
        what arrived (a combination with weights 1)"""
        zeros = (await self._deal_round(0, n))[1]
        return self.masked(zeros, 0, None, n)

    def _recombined(self, got, n, ctx):
        t0 = time.perf_counter()
        parts = ctx.upload(np.ascontiguousarray(np.stack(got)))
        res = ScalarVector.empty(n, ctx)
        ctx.bn256_share_combine(parts.ptr, self.parties, n, n, self.weights, None, None, res.ptr)
        out = res.to_ints()
        self._stage("exchange", t0)
        return out

    async def output(self, x):
        """open a share vector (of any degree below M) to all parties: every party sends its shares, the M-point
        recombination runs on the device -> list of ints mod n"""
        n, ctx = len(x), x.ctx
        if n == 0:
            return []
        mine = ctx.download(x.ptr, 32 * n, (n, 32))
        return self._recombined(await self.exchange_vectors(mine), n, ctx)

    async def exchange_points(self, points, scalars=None):
        """send this party's BN256Point / BN256TwistPoint elements as bytes, receive everybody's: list over parties of
        lists of points.  scalars: an (n, 32) uint8 array of shares that rides along in the same exchange; then
        -> (points, the n opened values)."""
        raw = [(p.group, p.to_bytes()) for p in points]
        every = await self.hub.exchange(self.pid, self._next_tag("pts"), (raw, scalars))
        cls = {1: pn.BN256Point, 2: pn.BN256TwistPoint}
        pts = [[cls[g].from_bytes(b) for g, b in part[0]] for part in every]
        if scalars is None:
            return pts
        n = len(scalars)
        return pts, (self._recombined([part[1] for part in every], n, self._context()) if n else [])

    def recombine_points(self, every, ctx=None):
        """The M parties' lists of n points each (exchange_points' result: element e of every list in one group) ->
        the n sums  sum_p weights[p] every[p][e]  in the exponent, as points.  The G1 and the twist elements are packed
        into one (M, n_g, width) table each: one upload, one validation (a point off its curve raises VmpcError with
        E_NOTONCURVE, as pynocchio.msm does), one vmpc_bn256_recombine_dev launch per group, ONE synchronisation and
        one download each."""
        ctx, M = ctx or self._context(), self.parties
        if len(every) != M:
            raise ValueError(f"recombine_points: {len(every)} lists of points for {M} parties")
        groups = [p.group for p in every[0]]
        if any([p.group for p in part] != groups for part in every[1:]):
            raise ValueError("recombine_points: the parties' lists differ in length or in their points' groups")
        out, pending = [None] * len(groups), []
        for cls in (pn.BN256Point, pn.BN256TwistPoint):
            ix = [i for i, g in enumerate(groups) if g == cls.group]
            if not ix:
                continue
            table = np.frombuffer(b"".join(part[i].to_bytes() for part in every for i in ix), np.uint8)
            parts, res = ctx.upload(table), ctx.alloc(cls.width * len(ix))
            if ctx.bn256_validate(cls.group, parts.ptr, M * len(ix)):
                raise _native.VmpcError(_native.E_NOTONCURVE, "trinocchio.recombine_points")
            ctx.bn256_recombine(cls.group, parts.ptr, M, len(ix), len(ix), self.weights, res.ptr)
            pending.append((cls, ix, parts, res))
        ctx.sync()
        for cls, ix, _, res in pending:
            raw = ctx.download(res.ptr, cls.width * len(ix)).tobytes()
            for k, i in enumerate(ix):
                out[i] = cls.from_bytes(raw[cls.width * k:cls.width * (k + 1)])
        return out


class _Zeros:
    """the zero sharings a party received in one deal round: M rows of `n` scalars at column `offset` of `parts`"""

    def __init__(self, parts, offset, n, stride):
        self.parts, self.offset, self.n, self.stride = parts, offset, n, stride


def deal_witness(c, threshold, parties, rng):
    """Degree-`threshold` Shamir shares mod n of every wire value for parties 1..M, as M (n_wires, 32) uint8 arrays
    (dealer / test helper: in the demo the shares come from MPyC's input protocol and calculate_witness)."""
    vals = [int(v) % ORDER for v in c]
    coeffs = [[rng.randrange(ORDER) for _ in vals] for _ in range(threshold)]
    out = []
    for p in range(parties):
        x = p + 1
        row = []
        for i, v in enumerate(vals):
            acc = 0
            for k in range(threshold - 1, -1, -1):
                acc = (acc + coeffs[k][i]) * x % ORDER
            row.append((acc + v) % ORDER)
        out.append(_native.ints_to_array(row, 32))
    return out


def _input_share_rows(x_share):
    """this party's input shares -> ((K, n_in, 32) uint8 canonical residues, whether the caller gave K vectors)"""
    if isinstance(x_share, np.ndarray) and x_share.dtype == np.uint8 and x_share.ndim in (2, 3):
        arr = np.ascontiguousarray(x_share if x_share.ndim == 3 else x_share[None])
        if arr.shape[2] != 32:
            raise ValueError(f"calculate_witness_shares: shares of {arr.shape[2]} bytes, scalars have 32")
        diff = arr.reshape(-1, 32)[:, ::-1].astype(np.int16) - _ORDER_BE          # most significant byte first
        first = (diff != 0).argmax(axis=1)
        if len(diff) and (diff[np.arange(len(diff)), first] >= 0).any():
            raise ValueError("calculate_witness_shares: a share is a residue mod n, below n")
        return arr, x_share.ndim == 3
    x = [int(v) for v in x_share]
    return pn.scalars_to_array(x).reshape(1, len(x), 32), False


async def calculate_witness_shares(rt, qap, x_share, ctx=None, wide_rows=0):
    """One party's run of the M-party R1CS solve (demo_zkp_trinocchio.py:70, qap.calculate_witness on secure values):
    from this party's degree-t shares of the INPUTS alone to its degree-t shares of every wire, with no wire ever opened.
    x_share: a list of ints, an (n_in, 32) uint8 array, or a (K, n_in, 32) array for K input vectors of one R1CS (array
    elements are residues below n).  -> (n_wires, 32) or (K, n_wires, 32) uint8, slot 0 = 1: what `prove` takes.

    pynocchio.ShareSolvePlan orders the rows: for r = 0 .. D the linear rows of depth r run locally through
    vmpc_bn256_r1cs_solve_batch_dev on the share vector (`wide_rows` as there), then for r < D the product rows of depth
    r + 1 cost ONE exchange - the party multiplies its shares, deals the degree-2t product afresh with degree t
    (vmpc_bn256_r1cs_share_mul_deal_dev; the product itself is stored nowhere), sends every party its row, and
    recombines what arrives with the M-point weights (vmpc_bn256_r1cs_share_finish_dev).  Exactly plan.n_rounds
    exchanges, whatever K is; a circuit without a product of shared values exchanges nothing.  A division by a shared
    value is ShareSolvePlan's ValueError, raised before any device call or exchange.  Whether the inputs satisfy the
    circuit's check rows is not tested here: prove(check=True) tests every row."""
    arr, many = _input_share_rows(x_share)
    K, n_in = arr.shape[0], arr.shape[1]
    plan = pn.ShareSolvePlan(qap, n_in)
    if K > _native.BN256_R1CS_MAX_WIT:
        raise ValueError(f"calculate_witness_shares: {K} input vectors, one call takes {_native.BN256_R1CS_MAX_WIT}")
    n_wires, M, t, D = qap.m + 1, rt.parties, rt.threshold, plan.n_rounds
    host = np.zeros((K, n_wires, 32), np.uint8)
    host[:, 0, 0] = 1
    host[:, 1:n_in + 1] = arr
    if K == 0:
        return host
    ctx = ctx or rt._context()
    ptrs, _ = plan.device(ctx)
    t0 = time.perf_counter()
    dc, bad = ctx.upload(host), ctx.alloc(4 * K * (D + 1))
    t0 = rt._stage("upload", t0)
    for r in range(D + 1):
        lv0, lv1 = int(plan.phase_ptr[r]), int(plan.phase_ptr[r + 1])
        # L_r: a sub-range of the local level table, its device copy moved along; the call sets its K status words
        ctx.bn256_r1cs_solve_batch(ptrs[:12] + [ptrs[12] + 4 * lv0], plan.local_level_ptr[lv0:lv1 + 1], n_in, qap.m,
                                   dc.ptr, n_wires, K, wide_rows, bad.ptr + 4 * K * r)
        t0 = rt._stage("local", t0)
        if r == D:
            break
        r0, r1 = plan.round_rows(r + 1)
        n_e = K * (r1 - r0)
        coeffs = ctx.upload(random_residues(rt.rng, t * n_e)) if t else None
        t0 = rt._stage("coeffs", t0)
        table = ctx.alloc(32 * M * n_e)
        ctx.bn256_r1cs_share_mul_deal(ptrs, r0, r1, qap.m, dc.ptr, n_wires, K, coeffs.ptr if t else None, t, M,
                                      table.ptr, n_e)
        t0 = rt._stage("mul_deal", t0)
        dealt = ctx.download(table.ptr, 32 * M * n_e, (M, n_e, 32))
        t0 = rt._stage("download", t0)
        got = await rt.exchange_vectors([dealt[q] for q in range(M)])
        t0 = rt._stage("exchange", t0)
        parts = ctx.upload(np.ascontiguousarray(np.stack(got)))
        t0 = rt._stage("upload", t0)
        ctx.bn256_r1cs_share_finish(ptrs, r0, r1, qap.m, parts.ptr, M, n_e, rt.weights, dc.ptr, n_wires, K)
        t0 = rt._stage("finish", t0)
    ctx.sync()
    words = ctx.download(bad.ptr, 4 * K * (D + 1)).view("<u4")
    assert (words == 0xFFFFFFFF).all(), "a linear row failed: ShareSolvePlan leaves no divisor that can be zero"
    out = ctx.download(dc.ptr, host.nbytes, host.shape)
    rt._stage("download", t0)
    return out if many else out[0]


async def prove_inputs(rt, qap, key, x_share, zk=True, check=True):
    """`prove` from shares of the inputs alone (the demo's whole flow): calculate_witness_shares on key.ctx, then prove
    on the shares of the witness -> prove's (proof, c_client).  n_rounds + prove's exchanges in all."""
    if not isinstance(key, pn.PreparedKey):
        raise TypeError("trinocchio.prove_inputs: key must be a pynocchio.PreparedKey")
    if isinstance(x_share, np.ndarray) and x_share.ndim == 3:
        raise ValueError("trinocchio.prove_inputs: one input vector per proof")
    c_share = await calculate_witness_shares(rt, qap, x_share, ctx=key.ctx)
    return await prove(rt, qap, key, c_share, zk=zk, check=check)


async def prove(rt, qap, key, c_share, zk=True, check=True):
    """One party's run of the M-party prover.  rt: this party's Runtime; key: a pynocchio.PreparedKey; c_share: this
    party's degree-t shares of the witness over qap.indices, an (n_wires, 32) uint8 array or a list of ints.
    -> (proof, c_client): the proof has the keys and point types of pynocchio.compute_proof's result, c_client is
    [1] + the opened I/O wires; `pynocchio.verify(qap, verikey, proof, c_client)` takes them unchanged.  Every party
    returns the same pair.

    zk: jointly random degree-t shared deltas make the proof zero-knowledge (the demo's TODO).
    check: the parties open a jointly random rho and the masked sum_j rho^j (a_j b_j - y_j) over the shared rows; if it
    is not zero the shares are not of a satisfying witness (or not consistent sharings at all) and every party raises
    ValueError("inconsistent shares") before a proof share is exchanged.  A wrong witness passes with probability at
    most d / n.  Without the check a wrong witness gives a proof whose H check fails.

    `prove_batch`'s body (_prove) on one witness: its exchanges, its random draws and its stages."""
    if not isinstance(key, pn.PreparedKey):
        raise TypeError("trinocchio.prove: key must be a pynocchio.PreparedKey")
    pn._check_cap(qap, "trinocchio.prove")
    return (await _prove(rt, qap, key, pn._witness_array(qap, c_share)[None], zk, check, "inconsistent shares"))[0]


async def prove_batch(rt, qap, key, c_shares, zk=True, check=True):
    """`prove` for K witnesses of one QAP in the exchanges of ONE: 4 with the check, 2 without, 1 when there is nothing to
    deal, whatever K is.  c_shares: this party's degree-t shares of the K witnesses, a (K, n_wires, 32) uint8 array or K
    vectors as `prove` takes them.  -> a list of K (proof, c_client) pairs, proof w with the keys and point types of
    pynocchio.compute_proof's result; every party returns the same list (K = 0: [] and no exchange).  If a masked
    residual is not zero every party raises ValueError("inconsistent shares: witness w"), w the lowest such witness,
    before a proof share leaves."""
    if not isinstance(key, pn.PreparedKey):
        raise TypeError("trinocchio.prove_batch: key must be a pynocchio.PreparedKey")
    arr, _ = pn._share_batch_args(qap, c_shares, None, "trinocchio.prove_batch")
    if len(arr) == 0:
        return []
    return await _prove(rt, qap, key, arr, zk, check, "inconsistent shares: witness {w}")


async def _prove(rt, qap, key, arr, zk, check, bad):
    """The prover behind `prove` (K = 1) and `prove_batch`: arr holds this party's shares of K >= 1 witnesses,
    (K, n_wires, 32); bad: the ValueError's text for a residual that is not zero, formatted with w = the lowest such witness.

    One deal round carries 3 K deltas (witness w's at the random shares 3 w .. 3 w + 2) and rho with degree t, and
    K residual masks and K n_h masks of h with degree 2t.  rho is opened once, after every share it tests is fixed; the
    K residuals of one vmpc_bn256_qap_residual_batch_dev launch are masked in one combination and opened in ONE
    exchange.  One rho for K witnesses: a batch with a wrong witness passes with probability at most K d / n (each
    witness's residual is a nonzero polynomial of degree below d in rho, the union bound over the witnesses).  Then
    compute_h_share_batch's stages on the row values that the residual read, one combination for the masks where h's rows
    are contiguous (zk: d + 1 of d + 1 scalars), pynocchio.compute_proof_batch, ONE exchange of the 8 K points with the K
    out_ix shares of the I/O wires, and one recombination launch per group (Runtime.recombine_points)."""
    K, d = len(arr), int(qap.d)
    ctx, M = key.ctx, rt.parties
    assert rt._context() is ctx, "the runtime and the prepared key share one context"
    n_h = d + 1 if zk else max(d - 1, 0)
    n_delta, n_check = (3 * K if zk else 0), (1 if check else 0)
    # 1. all dealt randomness in one exchange: deltas and rho with degree t, zeros (K residuals, K h) with degree 2t
    rand, zeros = await rt._deal_round(n_delta + n_check, K * (n_check + n_h))
    t0 = time.perf_counter()
    aby, keep = pn._upload_row_values_batch(ctx, qap, arr)
    t0 = rt._stage("h_share", t0)
    if check:
        # 2. rho is opened only now: the shares it tests were fixed before anybody knew it
        rho = (await rt.output(rand[n_delta:]))[0]
        t0 = time.perf_counter()
        res = ScalarVector.empty(K, ctx)
        for lo in range(0, K, _native.BN256_QAP_MAX_WIT):
            n = min(K - lo, _native.BN256_QAP_MAX_WIT)
            row = aby.ptr + 32 * 3 * d * lo
            ctx.bn256_qap_residual_batch(row, row + 32 * d, row + 64 * d, 3 * d, d, rho, res.ptr + 32 * lo, n)
        # 3. K degree-2t shares of 0 for satisfying witnesses, opened together under K zero sharings
        masked = rt.masked(zeros, 0, res.ptr, K)
        rt._stage("residual", t0)
        opened = await rt.output(masked)
        wrong = [w for w, v in enumerate(opened) if v != 0]
        if wrong:
            raise ValueError(bad.format(w=wrong[0]))
        t0 = time.perf_counter()
    deltas = None
    if zk:
        dv = rand[:n_delta].to_ints()            # this party's own shares: compute_proof_batch takes them from the host
        deltas = [types.SimpleNamespace(v=dv[3 * w], w=dv[3 * w + 1], y=dv[3 * w + 2]) for w in range(K)]
    hs = pn._h_from_row_values_batch(ctx, qap, aby, rand[:n_delta] if zk else None, K)
    del aby, keep        # (the stream has drained)
    t0 = rt._stage("h_share", t0)
    if n_h:
        # h's K rows lie d + 1 scalars apart: with the deltas they are contiguous and one combination masks them all
        stride, ones = d + 1, [1] * M
        first = zeros.parts.ptr + 32 * (zeros.offset + K * n_check)
        hm = ctx.alloc(32 * stride * K)
        if n_h == stride:
            ctx.bn256_share_combine(first, M, K * n_h, zeros.stride, ones, None, hs[0].buf.ptr, hm.ptr)
        else:
            for w in range(K):
                ctx.bn256_share_combine(first + 32 * n_h * w, M, n_h, zeros.stride, ones, None, hs[w].buf.ptr,
                                        hm.ptr + 32 * stride * w)
        hs = [pn.HPoly(ctx, pn._BufferView(hm, 32 * stride * w, 32 * stride), n_h) for w in range(K)]
    t0 = rt._stage("masks", t0)
    shares = pn.compute_proof_batch(qap, arr, hs, key, deltas)
    rt._stage("proof_share", t0)
    # 4. the 8 K points and this party's shares of the K witnesses' I/O wires, one exchange
    names = list(shares[0])
    out_ix = int(qap.out_ix)
    io = np.ascontiguousarray(arr[:, 1:out_ix + 1]).reshape(K * out_ix, 32)
    every, opened = await rt.exchange_points([share[k] for share in shares for k in names], io)
    t0 = time.perf_counter()
    flat = rt.recombine_points(every, ctx)
    rt._stage("recombine", t0)
    e = len(names)
    return [(dict(zip(names, flat[e * w:e * (w + 1)])), [1] + opened[out_ix * w:out_ix * (w + 1)]) for w in range(K)]


async def prove_inputs_batch(rt, qap, key, x_shares, zk=True, check=True):
    """`prove_batch` from shares of the inputs alone: calculate_witness_shares on key.ctx for the K input vectors (a
    (K, n_in, 32) uint8 array, or K vectors of ints), then prove_batch on the shares of the K witnesses -> prove_batch's
    list.  n_rounds + prove_batch's exchanges for all K."""
    if not isinstance(key, pn.PreparedKey):
        raise TypeError("trinocchio.prove_inputs_batch: key must be a pynocchio.PreparedKey")
    if not (isinstance(x_shares, np.ndarray) and x_shares.ndim == 3):
        rows = [pn.scalars_to_array(x if isinstance(x, np.ndarray) else [int(v) for v in x]) for x in x_shares]
        if len({r.shape for r in rows}) > 1:
            raise ValueError("trinocchio.prove_inputs_batch: the input vectors differ in length")
        x_shares = np.stack(rows) if rows else np.zeros((0, 0, 32), np.uint8)
    if len(x_shares) == 0:
        return []
    c_shares = await calculate_witness_shares(rt, qap, x_shares, ctx=key.ctx)
    return await prove_batch(rt, qap, key, c_shares, zk=zk, check=check)

