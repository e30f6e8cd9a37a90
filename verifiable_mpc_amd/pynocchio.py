"""Pinocchio prover's group work on MI355X (BASELINE config 5).

    compute_proof    verifiable_mpc/trinocchio/pynocchio.py:228-273

The reference builds eight proof elements, each
    apply_to_list(point_add, [int(c[i]) * evalkey[<name i>] for i in qap.indices_mid])
(seven over G1, one over the twist, plus h(s) over the powers of s) and, in the
zero-knowledge case, adds `delta * evalkey[<t term>]`.  Here every element is ONE BN-256 MSM
(csrc/bn256.hip) with the zero-knowledge terms appended as extra (scalar, point) pairs.
Keys and proofs hold `BN256Point` / `BN256TwistPoint` objects (affine coordinates); foreign
points (e.g. MPyC's Jacobian elements) are accepted if they expose `.normalize()` and three
indexable coordinates.  QAP construction from code stays with the reference (out of scope);
the witness of a sparse R1CS is computed here (calculate_witness below).

    compute_h        verifiable_mpc/trinocchio/pynocchio.py:203-225 (compute_p_poly, p / qap.t, compute_h_zk_terms)

The prover's h = (V W - Y) / t comes from the R1CS row values at the witness (csrc/bn256_qap_h.hip, DESIGN.md section
14): this field has no NTT of useful length, and V, W are never interpolated - their quotients by t are power series
whose coefficients are the moments sum_j (a_j / t'(j)) j^k of the weighted row values, and h is a correlation of t's
coefficients with the low half of the two series' product.  The result stays on the device for compute_proof.

    compute_h_batch, compute_proof_batch, prove_batch    (no counterpart in the reference)

K witnesses of ONE QAP: exactly the results of K compute_h / compute_proof calls, with every stage of h run once for all
K - the witness on the grid, the launch plans chosen with K counted - and the K proofs' uploads, synchronisations,
downloads and inversions shared.  What verify_batch takes.  There is one implementation per stage:
compute_h, compute_h_share and compute_proof over a PreparedKey are these functions' code on a batch of one.

    calculate_witness, calculate_witness_batch, prove_batch_inputs, SolvePlan    (tools/code_to_qap.py QAP.calculate_witness)

The witness from the inputs, for one input vector or K of them in one call: a host plan orders the rows of an R1CSQAP by
depth level from the matrices alone, and csrc/bn256_r1cs_solve.hip solves level by level on the device - runs of narrow
levels inside one launch, wide levels in launches of their own.

    Trapdoor, SampleDeltas, Generators        verifiable_mpc/trinocchio/pynocchio.py:36-69 (draws from `prng`)
    generate_evalkey, generate_verikey        verifiable_mpc/trinocchio/pynocchio.py:101-200
    PreparedKey.generate                      PreparedKey(qap, generate_evalkey(...)) without a host round trip

Key generation evaluates every QAP polynomial at the secret s on the device (csrc/bn256_keygen.hip): a reference QAP
as a mat-vec of its coefficients against 1, s, .., s^d; an R1CSQAP (the sparse R1CS, constraint j at x = j) as
v_i(s) = sum_j V[j][i] l_j(s) over the Lagrange basis at s, O(nnz + d).  Each key entry is then one fixed-base product
of g1 or g2 (the scaled generators' factors folded into the exponent).

    pairing          verifiable_mpc/trinocchio/pynocchio.py:67-72 (ac20/pairing.py optimal_ate)
    verify           verifiable_mpc/trinocchio/pynocchio.py:276-325
    verify_batch     the same for many proofs over one verification key

The verifier evaluates each of the five checks as "product of pairings == 1" (csrc/bn256_pairing.hip: one lane
per Miller loop, one lane per product for the final exponentiation); pairing values equal the reference's
coefficient for coefficient.  Off-curve points raise ValueError; G2 subgroup membership is not checked.
"""
import random

import numpy as np

from . import _native
from .device import get_context
from .sparse import ColumnPlan, csr_entries

P = 65000549695646603732796438742359905742825358107623003571877145026864184071783
ORDER = 65000549695646603732796438742359905742570406053903786389881062969044166799969


class BN256Point:
    """Affine point of G1 (y^2 = x^3 + 3 over F_p); `coords is None` is the point at infinity."""
    group = 1
    width = 64

    def __init__(self, coords=None):
        self.coords = None if coords is None else tuple(int(v) % P for v in self._flat(coords))

    @staticmethod
    def _flat(coords):
        return coords

    def to_bytes(self):
        if self.coords is None:
            return bytes(self.width)
        return b"".join(v.to_bytes(32, "little") for v in self.coords)

    @classmethod
    def from_bytes(cls, b):
        vals = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(cls.width // 32)]
        obj = cls.__new__(cls)
        obj.coords = None if not any(vals) else tuple(vals)
        return obj

    def normalize(self):
        return self

    def __eq__(self, other):
        return type(other) is type(self) and self.coords == other.coords

    def __hash__(self):
        return hash((self.group, self.coords))

    def __repr__(self):
        return "O" if self.coords is None else repr(list(self.coords))


class BN256TwistPoint(BN256Point):
    """Affine point of the twist over F_p[i]/(i^2+1): coords = (x.re, x.im, y.re, y.im)."""
    group = 2
    width = 128

    @staticmethod
    def _flat(coords):
        if len(coords) == 2:            # ((x.re, x.im), (y.re, y.im))
            return (coords[0][0], coords[0][1], coords[1][0], coords[1][1])
        return coords


def _as_bytes(pt):
    if isinstance(pt, BN256Point):
        return pt.group, pt.to_bytes()
    # foreign Jacobian / affine element: normalise and read x, y (each an int or a pair)
    q = pt.normalize() if hasattr(pt, "normalize") else pt
    x, y = q[0], q[1]
    if hasattr(x, "__len__") or (hasattr(x, "value") and hasattr(x.value, "__len__")):
        xs = list(x.value) if hasattr(x, "value") else list(x)
        ys = list(y.value) if hasattr(y, "value") else list(y)
        vals = [int(xs[0]), int(xs[1]), int(ys[0]), int(ys[1])]
        return 2, b"".join((v % P).to_bytes(32, "little") for v in vals)
    return 1, (int(x) % P).to_bytes(32, "little") + (int(y) % P).to_bytes(32, "little")


def msm(scalars, points, ctx=None):
    """sum_i scalars[i] * points[i] on the GPU; all points from the same group (G1 or twist)."""
    assert len(scalars) == len(points)
    ctx = ctx or get_context()
    if not points:
        raise ValueError("empty sum has no group")
    enc = [_as_bytes(p) for p in points]
    group = enc[0][0]
    assert all(g == group for g, _ in enc), "mixed groups in one sum"
    width = 64 if group == 1 else 128
    pts = np.frombuffer(b"".join(b for _, b in enc), dtype=np.uint8).reshape(-1, width)
    sc = _native.ints_to_array([int(s) % ORDER for s in scalars], 32)
    dp, ds, out = ctx.upload(pts), ctx.upload(sc), ctx.alloc(width)
    if ctx.bn256_validate(group, dp.ptr, len(points)):
        raise _native.VmpcError(_native.E_NOTONCURVE, "pynocchio.msm")
    ctx.bn256_msm(group, ds.ptr, dp.ptr, len(points), out.ptr)
    ctx.sync()
    cls = BN256Point if group == 1 else BN256TwistPoint
    return cls.from_bytes(ctx.download(out.ptr, width).tobytes())


# the eight proof elements of pynocchio.py:228-273: name -> (evalkey name of term i, zero-knowledge terms
# as (delta attribute, evalkey name))
_ELEMENTS = {
    "r_v*v_mid*g1": (lambda i: "r_v*v" + str(i) + "*g1", (("v", "r_v*t*g1"),)),
    "r_w*w_mid*g2": (lambda i: "r_w*w" + str(i) + "*g2", (("w", "r_w*t*g2"),)),
    "r_y*y_mid*g1": (lambda i: "r_y*y" + str(i) + "*g1", (("y", "r_y*t*g1"),)),
    "r_v*alpha_v*v_mid*g1": (lambda i: f"r_v*alpha_v*v{i}*g1", (("v", "r_v*alpha_v*t*g1"),)),
    "r_w*alpha_w*w_mid*g1": (lambda i: f"r_w*alpha_w*w{i}*g1", (("w", "r_w*alpha_w*t*g1"),)),
    "r_y*alpha_y*y_mid*g1": (lambda i: f"r_y*alpha_y*y{i}*g1", (("y", "r_y*alpha_y*t*g1"),)),
    "r_v*beta*v_mid+r_w*beta*w_mid+r_y*beta*y_mid*g1": (
        lambda i: f"r_v*beta*v+r_w*beta*w+r_y*beta*y{i}_g1",
        (("v", "r_v*beta*t*g1"), ("w", "r_w*beta*t*g1"), ("y", "r_y*beta*t*g1"))),
}


def _from_jacobian(group, raw):
    """(X : Y : Z) canonical residues -> affine BN256Point / BN256TwistPoint (x = X/Z^2, y = Y/Z^3)"""
    v = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]
    if group == 1:
        X, Y, Z = v
        if Z == 0:
            return BN256Point(None)
        zi = pow(Z, P - 2, P)
        return BN256Point((X * zi * zi % P, Y * zi * zi % P * zi % P))
    mul = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
    X, Y, Z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    if Z == (0, 0):
        return BN256TwistPoint(None)
    d = pow(Z[0] * Z[0] + Z[1] * Z[1], P - 2, P)
    zi = (Z[0] * d % P, (-Z[1] * d) % P)
    zi2 = mul(zi, zi)
    x, y = mul(X, zi2), mul(mul(Y, zi2), zi)
    return BN256TwistPoint((x[0], x[1], y[0], y[1]))


def _from_jacobian_many_g1(raws):
    """several G1 sums (X : Y : Z) -> affine, ONE modular inversion for all of them (Montgomery's trick)"""
    vals = [[int.from_bytes(r[32 * i:32 * i + 32], "little") for i in range(3)] for r in raws]
    zs = [v[2] for v in vals if v[2]]
    prefix, run = [], 1
    for z in zs:
        prefix.append(run)
        run = run * z % P
    inv = pow(run, P - 2, P) if zs else 0
    zinv = [0] * len(zs)
    for i in range(len(zs) - 1, -1, -1):
        zinv[i] = inv * prefix[i] % P
        inv = inv * zs[i] % P
    out, j = [], 0
    for X, Y, Z in vals:
        if Z == 0:
            out.append(BN256Point(None))
            continue
        zi = zinv[j]
        j += 1
        zi2 = zi * zi % P
        out.append(BN256Point((X * zi2 % P, Y * zi2 % P * zi % P)))
    return out


def _from_jacobian_many_g2(raws):
    """several twist sums (X : Y : Z) over F_p[i] -> affine, ONE modular inversion for all of them: 1 / Z = conj(Z) / N(Z)
    with the norms N(Z) = Z.re^2 + Z.im^2 in F_p inverted together (Montgomery's trick)"""
    vals = [[int.from_bytes(r[32 * i:32 * i + 32], "little") for i in range(6)] for r in raws]
    norms = [(v[4] * v[4] + v[5] * v[5]) % P for v in vals if v[4] or v[5]]
    prefix, run = [], 1
    for n in norms:
        prefix.append(run)
        run = run * n % P
    inv = pow(run, P - 2, P) if norms else 0
    ninv = [0] * len(norms)
    for i in range(len(norms) - 1, -1, -1):
        ninv[i] = inv * prefix[i] % P
        inv = inv * norms[i] % P
    mul = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
    out, j = [], 0
    for v in vals:
        if not (v[4] or v[5]):
            out.append(BN256TwistPoint(None))
            continue
        zi = (v[4] * ninv[j] % P, (-v[5] * ninv[j]) % P)
        j += 1
        zi2 = mul(zi, zi)
        x, y = mul((v[0], v[1]), zi2), mul(mul((v[2], v[3]), zi2), zi)
        out.append(BN256TwistPoint((x[0], x[1], y[0], y[1])))
    return out


class _KeyVector:
    """One evaluation-key vector on the device: points uploaded, validated and tabulated once."""

    def __init__(self, ctx, points):
        enc = [_as_bytes(p) for p in points]
        group = enc[0][0]
        assert all(g == group for g, _ in enc), "mixed groups in one key vector"
        width = 64 if group == 1 else 128
        pts = np.frombuffer(b"".join(b for _, b in enc), dtype=np.uint8).reshape(-1, width)
        self._init_device(ctx, group, ctx.upload(pts), len(points))

    @classmethod
    def from_device(cls, ctx, group, points_buf, n):
        """from n affine points already in device memory (64 / 128 bytes each)"""
        self = cls.__new__(cls)
        self._init_device(ctx, group, points_buf, n)
        return self

    def _init_device(self, ctx, group, dp, n):
        self.group, self.n = group, n
        self.width = 64 if group == 1 else 128
        if ctx.bn256_validate(group, dp.ptr, n):
            raise _native.VmpcError(_native.E_NOTONCURVE, "pynocchio.PreparedKey")
        self.table = ctx.bn256_table_build(group, dp.ptr, n)
        ctx.sync()


class PreparedKey:
    """The evaluation key of one circuit, prepared for many proofs: the eight point vectors that
    compute_proof reads (pynocchio.py:228-246) are converted, uploaded, checked and expanded into
    fixed-base tables ONCE; each proof then only ships its scalars.  Pass it to compute_proof in place
    of the evalkey dict."""

    def __init__(self, qap, evalkey, ctx=None):
        self.ctx = ctx or get_context()
        self.mid = list(qap.indices_mid)
        self.mid_index = np.asarray(self.mid, dtype=np.int64)
        self.vectors = {}
        self.zk_missing = {}      # element -> names of zero-knowledge key points the evalkey lacks
        for name, (key_fmt, zk) in _ELEMENTS.items():
            points = [evalkey[key_fmt(i)] for i in self.mid]
            missing = [zname for _, zname in zk if zname not in evalkey]
            if missing:
                self.zk_missing[name] = missing
            points += _tail_points(name, zk, evalkey, bool(missing))
            self.vectors[name] = _KeyVector(self.ctx, points)
        powers = []
        while "s^" + str(len(powers)) + "*g1" in evalkey:
            powers.append(evalkey["s^" + str(len(powers)) + "*g1"])
        self.vectors["h*g1"] = _KeyVector(self.ctx, powers)

    @classmethod
    def synthetic(cls, ctx, n, seed=3, mid=None, exponents=False):
        """A key of n `mid` wires whose every entry is a distinct multiple of its group's generator, built on the
        device: the shape of a real prepared key without a circuit (bench.py, scripts/pinocchio_probe.py).
        mid: the key's wire indices (default 0 .. n-1).  exponents=True: return (key, {element: (n + tail, 32) uint8
        discrete logs of its key vector}), zero where a column holds the point at infinity - what a test needs to
        know every sum's value (tests/test_gpu_bn256_edges.py)."""
        g1 = (1).to_bytes(32, "little") + (P - 2).to_bytes(32, "little")
        g2 = b"".join(v.to_bytes(32, "little") for v in (
            64746500191241794695844075326670126197795977525365406531717464316923369116492,
            21167961636542580255011770066570541300993051739349375019639421053990175267184,
            17778617556404439934652658462602675281523610326338642107814333856843981424549,
            20666913350058776956210519119118544732556678129809273996262322366050359951122))
        rng = np.random.default_rng(seed)
        key = cls.__new__(cls)
        key.ctx, key.mid, key.vectors = ctx, list(range(n)) if mid is None else [int(i) for i in mid], {}
        key.mid_index, key.zk_missing = np.asarray(key.mid, dtype=np.int64), {}
        assert len(key.mid) == n
        logs = {}
        for name in list(_ELEMENTS) + ["h*g1"]:
            grp, gen, width = (2, g2, 128) if name.endswith("g2") else (1, g1, 64)
            zk = _ELEMENTS[name][1] if name in _ELEMENTS else ()
            tail = _tail_slots(name, zk)
            ex = rng.integers(0, 256, size=(n + len(tail), 32), dtype=np.uint8)
            ex[:, 31] &= 0x7F
            dg, de = ctx.upload(np.frombuffer(gen, np.uint8)), ctx.upload(ex)
            pts = ctx.alloc(width * (n + len(tail)))
            ctx.bn256_fixed_base(grp, dg.ptr, de.ptr, n + len(tail), pts.ptr)
            for j, used in enumerate(tail):          # columns of deltas this element does not use: infinity
                if not used:
                    ctx.upload_into(pts.ptr + width * (n + j), np.zeros(width, np.uint8))
            ctx.sync()
            key.vectors[name] = _KeyVector.from_device(ctx, grp, pts, n + len(tail))
            if exponents:
                logs[name] = ex.copy()
                for j, used in enumerate(tail):
                    if not used:
                        logs[name][n + j] = 0
        return (key, logs) if exponents else key


# The six G1 sums over c_mid (pynocchio.py:229-246) go through ONE multi-key pass (vmpc_bn256_table_msm_multi_dev):
# they share the scalar vector c_mid || (delta_v, delta_w, delta_y), so each of their key vectors carries three
# trailing columns in that order - the element's zero-knowledge point where it uses the delta, the point at infinity
# where it does not (an infinity entry adds nothing, csrc/bn256_curve.h).
_DELTAS = ("v", "w", "y")
_SHARED_G1 = tuple(name for name in _ELEMENTS if name.endswith("g1"))


def _tail_slots(name, zk):
    """for each trailing column of the element's key vector: does the element use that delta?"""
    if name in _SHARED_G1:
        used = {attr for attr, _ in zk}
        return [d in used for d in _DELTAS]
    return [True] * len(zk)


def _tail_points(name, zk, evalkey, missing):
    if name in _SHARED_G1:
        by_delta = {attr: zname for attr, zname in zk}
        return [evalkey[by_delta[d]] if (d in by_delta and not missing) else BN256Point(None) for d in _DELTAS]
    return [] if missing else [evalkey[zname] for _, zname in zk]


def scalars_to_array(values):
    """Python ints / field elements -> (n, 32) uint8 canonical residues mod the group order, as fast as the
    interpreter allows (one to_bytes per element; the reduction only for values that need it).  (n, 32) uint8
    arrays pass through untouched: a caller that keeps its witness in numpy pays nothing here - at 2^18 terms
    this conversion (2 x 17 ms for c and h) is otherwise longer than the eight sums on the GPU."""
    if isinstance(values, np.ndarray):
        return _native.as_bytes_array(values, 32)
    vals = values if isinstance(values, list) else list(values)
    if not vals:
        return np.zeros((0, 32), np.uint8)
    if type(vals[0]) is not int:
        vals = [int(v) for v in vals]
    try:
        raw = b"".join([v.to_bytes(32, "little") for v in vals])       # (negatives and values >= 2^256 raise)
    except AttributeError:                                             # field elements after a leading int
        vals = [int(v) for v in vals]
        return scalars_to_array(vals)
    except OverflowError:
        raw = b"".join([(v % ORDER).to_bytes(32, "little") for v in vals])
        return np.frombuffer(raw, np.uint8).reshape(-1, 32)
    arr = np.frombuffer(raw, np.uint8).reshape(-1, 32)
    big = np.nonzero(arr[:, 31] >= 0x8f)[0]          # order = 0x8fb5...: only these rows can be >= order
    if len(big):
        arr = arr.copy()
        for i in big:
            arr[i] = np.frombuffer((vals[i] % ORDER).to_bytes(32, "little"), np.uint8)
    return arr


def _mid_is_identity(key, n_wires):
    flag = getattr(key, "_mid_identity", None)
    if flag is None:
        flag = key._mid_identity = bool(len(key.mid) and key.mid[0] == 0 and key.mid[-1] == len(key.mid) - 1
                                        and np.array_equal(key.mid_index, np.arange(len(key.mid))))
    return flag and n_wires == len(key.mid)


def compute_proof(qap, c, h, evalkey, deltas=None):
    """Pinocchio proof elements (pynocchio.py:228-273), one MSM per element.  `evalkey` is the
    reference's dict of points, or a PreparedKey made from it (device-resident, tabulated): then this is
    _compute_proof_batch_prepared's batch of one, which also says what c and h may be."""
    if isinstance(evalkey, PreparedKey):
        return _compute_proof_batch_prepared(evalkey, [c], [h], None if deltas is None else [deltas])[0]
    mid = list(qap.indices_mid)
    cm = [int(c[i]) for i in mid]

    def element(key_fmt, zk=()):
        scalars = list(cm) + [int(d) for d, _ in zk]
        points = [evalkey[key_fmt(i)] for i in mid] + [evalkey[name] for _, name in zk]
        return msm(scalars, points)

    zk = (lambda *pairs: pairs) if deltas is not None else (lambda *pairs: ())
    dv, dw, dy = (deltas.v, deltas.w, deltas.y) if deltas is not None else (0, 0, 0)
    h_scalars = [int(h.coeffs[i]) for i in range(0, len(h))]
    h_points = [evalkey["s^" + str(i) + "*g1"] for i in range(0, len(h))]
    return {
        "r_v*v_mid*g1": element(lambda i: "r_v*v" + str(i) + "*g1", zk((dv, "r_v*t*g1"))),
        "r_w*w_mid*g2": element(lambda i: "r_w*w" + str(i) + "*g2", zk((dw, "r_w*t*g2"))),
        "r_y*y_mid*g1": element(lambda i: "r_y*y" + str(i) + "*g1", zk((dy, "r_y*t*g1"))),
        "r_v*alpha_v*v_mid*g1": element(lambda i: f"r_v*alpha_v*v{i}*g1", zk((dv, "r_v*alpha_v*t*g1"))),
        "r_w*alpha_w*w_mid*g1": element(lambda i: f"r_w*alpha_w*w{i}*g1", zk((dw, "r_w*alpha_w*t*g1"))),
        "r_y*alpha_y*y_mid*g1": element(lambda i: f"r_y*alpha_y*y{i}*g1", zk((dy, "r_y*alpha_y*t*g1"))),
        "r_v*beta*v_mid+r_w*beta*w_mid+r_y*beta*y_mid*g1": element(
            lambda i: f"r_v*beta*v+r_w*beta*w+r_y*beta*y{i}_g1",
            zk((dv, "r_v*beta*t*g1"), (dw, "r_w*beta*t*g1"), (dy, "r_y*beta*t*g1"))),
        "h*g1": msm(h_scalars, h_points),
    }


def _compute_proof_batch_prepared(key, cs, hs, deltas):
    """The eight sums of K proofs over a prepared key, stage-major; compute_proof is the K = 1 call.  ONE upload of the K
    scalar vectors c_mid || (delta_v, delta_w, delta_y) (K = 1: c_mid straight from the caller's array, the deltas behind
    it), then on three streams: K twist sums on aux 20 (the longest single sum, first; without deltas read from the shared
    vector in place, with deltas each over c_mid || delta_w, put together by two device copies on that stream), K
    six-key passes on the main stream (the SIX G1 sums over c_mid are one multi-key pass: one recoding, sort and plan,
    six bucket launches over the one sorted index list, one reduction and one finishing launch) and K h sums on aux 21 -
    the bucket kernels take turns on the chip, the reductions and recombinations (latency chains) overlap them.  All
    are queued without a host wait in between (the table sums do not synchronise); ONLY THEN are host-side h
    coefficients converted, while the GPU works through the sums over c.  One synchronisation per stream, one download
    of all 8 K Jacobian results and two shared inversions (7 K G1 results, K twist results).
    cs[w]: indexable by qap.indices_mid (the reference's list of ints / field elements), or an (n_wires, 32) uint8 array
    of canonical residues (rows taken by index); hs[w]: the reference's polynomial (.coeffs), a list, an (len, 32) uint8
    array, or an HPoly - K HPoly are read where they lie on the device."""
    from .device import get_aux_context
    ctx, K = key.ctx, len(cs)
    if deltas is not None and key.zk_missing:
        raise KeyError("zero-knowledge deltas given but the prepared key lacks "
                       + ", ".join(sorted(n for names in key.zk_missing.values() for n in names)))
    n_mid = len(key.mid)
    zk = deltas is not None
    n_shared = n_mid + (3 if zk else 0)
    n_twist = n_mid + (1 if zk else 0)
    rows = max(n_shared, 1)

    def scalars(w):
        """witness w's c_mid as an (n_mid, 32) array - the caller's own memory where no gather is needed - and its deltas"""
        c = cs[w]
        if isinstance(c, np.ndarray):
            c_all = _native.as_bytes_array(c, 32)
            # (a key whose mid wires are ALL the wires, in order, needs no gather: 8 MB less to copy at 2^18 terms)
            c_mid = c_all if _mid_is_identity(key, len(c_all)) else c_all[key.mid_index]
        else:
            c_mid = scalars_to_array([c[i] for i in key.mid])
        return c_mid, _native.ints_to_array([int(getattr(deltas[w], d)) % ORDER for d in _DELTAS], 32) if zk else None

    if K == 1:
        # one proof: c_mid goes up from where it lies and the deltas in a second small upload behind it - staging the
        # row on the host first would copy 8 MB more at 2^18 terms, of the order of the whole proof
        head = ctx.alloc(32 * rows)
        c_mid, dv = scalars(0)
        ctx.upload_into(head.ptr, c_mid)
        if zk:
            ctx.upload_into(head.ptr + 32 * n_mid, dv)
    else:
        host = np.zeros((K * rows, 32), np.uint8)
        for w in range(K):
            host[w * rows:w * rows + n_mid], dv = scalars(w)
            if zk:
                host[w * rows + n_mid:w * rows + n_shared] = dv
        head = ctx.upload(host)
    twist_sc = ctx.alloc(32 * K * n_twist) if zk else head
    twist_stride = 32 * (n_twist if zk else rows)
    g1 = [key.vectors[name] for name in _SHARED_G1]
    tables = [v.table.ptr for v in g1]
    twist_name = next(name for name in _ELEMENTS if name not in _SHARED_G1)
    tv, hv = key.vectors[twist_name], key.vectors["h*g1"]
    # one result buffer for the three streams: per witness six G1 sums, the h sum (96 bytes each), the twist sum (192)
    n_g1, per = len(g1), 96 * (len(g1) + 1) + 192
    out = ctx.alloc(per * K)
    twist_ctx, h_ctx = get_aux_context(20), get_aux_context(21)
    twist_ctx.wait_for(ctx)               # `head` and `out` come from the main stream
    h_ctx.wait_for(ctx)
    for w in range(K):
        if zk:      # c_mid || delta_w out of the witness's row c_mid || (delta_v, delta_w, delta_y)
            if n_mid:
                twist_ctx.copy(twist_sc.ptr + twist_stride * w, head.ptr + 32 * rows * w, 32 * n_mid)
            twist_ctx.copy(twist_sc.ptr + twist_stride * w + 32 * n_mid, head.ptr + 32 * (rows * w + n_mid + 1), 32)
        twist_ctx.bn256_table_msm(2, tv.table.ptr, tv.n, twist_sc.ptr + twist_stride * w, n_twist, None,
                                  out.ptr + per * w + 96 * (n_g1 + 1))
    for w in range(K):
        ctx.bn256_table_msm_multi(1, tables, g1[0].n, head.ptr + 32 * rows * w, n_shared, out.ptr + per * w)
    # h: a compute_h_batch result is read where it lies; anything else is converted and uploaded once, on h's stream
    keep = []
    if K and all(isinstance(h, HPoly) for h in hs):
        for src in {id(h.ctx): h.ctx for h in hs}.values():
            h_ctx.wait_for(src)
        h_ptrs = [(h.buf.ptr if len(h) else head.ptr, len(h)) for h in hs]
    else:
        arrs = []
        for h in hs:
            if isinstance(h, HPoly):
                arrs.append(scalars_to_array(h.coeffs))
            else:
                hc = h if isinstance(h, (np.ndarray, list)) else h.coeffs
                arrs.append(scalars_to_array(hc if isinstance(hc, np.ndarray) else [hc[i] for i in range(len(h))]))
        offs = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
        hb = h_ctx.upload((arrs[0] if K == 1 else np.concatenate(arrs)) if offs[-1] else np.zeros((1, 32), np.uint8))
        keep.append(hb)
        h_ptrs = [(hb.ptr + 32 * int(offs[w]), len(arrs[w])) for w in range(K)]
    for w, (ptr, n) in enumerate(h_ptrs):
        assert n <= hv.n
        h_ctx.bn256_table_msm(1, hv.table.ptr, hv.n, ptr, n, None, out.ptr + per * w + 96 * n_g1)
    ctx.sync()
    twist_ctx.sync()
    h_ctx.sync()
    raw = ctx.download(out.ptr, per * K).tobytes()
    del keep
    pts1 = _from_jacobian_many_g1([raw[per * w + 96 * i:per * w + 96 * i + 96] for w in range(K) for i in range(n_g1 + 1)])
    pts2 = _from_jacobian_many_g2([raw[per * w + 96 * (n_g1 + 1):per * (w + 1)] for w in range(K)])
    proofs = []
    for w in range(K):
        el = dict(zip(_SHARED_G1 + ("h*g1",), pts1[(n_g1 + 1) * w:(n_g1 + 1) * (w + 1)]))
        el[twist_name] = pts2[w]
        proofs.append({name: el[name] for name in list(_ELEMENTS) + ["h*g1"]})
    return proofs


def compute_proof_batch(qap, cs, hs, key, deltas=None):
    """[compute_proof(qap, cs[w], hs[w], key, deltas[w]) for w in range(K)], point for point.  Over a PreparedKey the K
    proofs share one upload, one synchronisation per stream, one download and the host inversions
    (_compute_proof_batch_prepared); over an evalkey dict this loops over compute_proof.  cs: K witnesses as compute_proof
    takes them, or one (K, n_wires, 32) uint8 array; hs: compute_h_batch's result (read in place on the device) or K of
    anything compute_proof accepts; deltas: None, or K objects with .v .w .y."""
    cs = list(cs)
    hs = list(hs)
    deltas = None if deltas is None else list(deltas)
    K = len(cs)
    if len(hs) != K or (deltas is not None and len(deltas) != K):
        raise ValueError("compute_proof_batch: one h (and one set of deltas) per witness")
    if K == 0:
        return []
    if isinstance(key, PreparedKey):
        return _compute_proof_batch_prepared(key, cs, hs, deltas)
    return [compute_proof(qap, cs[w], hs[w], key, None if deltas is None else deltas[w]) for w in range(K)]


def prove_batch(qap, cs, key, deltas=None):
    """K proofs of one circuit: compute_h_batch, then compute_proof_batch on its device-resident result -> a list of K
    proof dicts, the counterpart of verify_batch.  key: a PreparedKey (or an evalkey dict: the proofs are then made one
    by one).  A witness that violates a constraint raises ValueError before any proof work starts."""
    ctx = key.ctx if isinstance(key, PreparedKey) else None
    cs = cs if isinstance(cs, np.ndarray) else list(cs)
    deltas = None if deltas is None else list(deltas)
    hs = compute_h_batch(qap, cs, deltas, ctx=ctx)
    return compute_proof_batch(qap, cs, hs, key, deltas)


# ---- the pairing and the verifier (trinocchio/pynocchio.py:67-72, 276-325; csrc/bn256_pairing.hip) ----------------

class GT:
    """An element of the pairing's target group: the 12 coefficients of the reference's tower element, in the order
    of include/vmpc.h (x.x.re, x.x.im, x.y.re, ..., y.z.im of f = x w + y).  Immutable; 1 is (0, ..., 0, 1, 0)."""
    __slots__ = ("coeffs",)

    def __init__(self, coeffs):
        coeffs = tuple(int(v) % P for v in coeffs)
        if len(coeffs) != 12:
            raise ValueError("a GT element has 12 coefficients")
        object.__setattr__(self, "coeffs", coeffs)

    def __setattr__(self, name, value):
        raise AttributeError("GT is immutable")

    @classmethod
    def from_bytes(cls, raw):
        return cls(int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(12))

    def is_one(self):
        return self.coeffs == _GT_ONE

    def __eq__(self, other):
        return isinstance(other, GT) and self.coeffs == other.coeffs

    def __hash__(self):
        return hash(("GT", self.coeffs))

    def __repr__(self):
        return "GT(" + ", ".join(hex(v) for v in self.coeffs) + ")"


_GT_ONE = (0,) * 10 + (1, 0)


def _validate(ctx, group, buf, n, what):
    if n and ctx.bn256_validate(group, buf.ptr, n):
        raise ValueError(f"{what}: point not on the {'BN-256 curve' if group == 1 else 'BN-256 twist'}")


def pairing(a, b, ctx=None):
    """e(a, b) for a in G1 and b on the twist, the reference's pynocchio.pairing(a, b) = optimal_ate(b, a), as a GT.
    Accepts BN256Point / BN256TwistPoint and foreign MPyC-style points; the point at infinity gives 1."""
    ctx = ctx or get_context()
    (ga, ra), (gb, rb) = _as_bytes(a), _as_bytes(b)
    if ga != 1 or gb != 2:
        raise ValueError("pairing(a, b): a must be a G1 point and b a twist point")
    da, db, out = ctx.upload(np.frombuffer(ra, np.uint8)), ctx.upload(np.frombuffer(rb, np.uint8)), ctx.alloc(384)
    _validate(ctx, 1, da, 1, "pairing: first argument")
    _validate(ctx, 2, db, 1, "pairing: second argument")
    ctx.bn256_pairing(da.ptr, db.ptr, 1, out.ptr)
    ctx.sync()
    return GT.from_bytes(ctx.download(out.ptr, 384).tobytes())


def pairing_product(g1_points, g2_points, offsets, ctx=None):
    """products prod_{offsets[k] <= j < offsets[k+1]} e(g1_points[j], g2_points[j]) -> (list of GT, list of bool
    is_one); one final exponentiation per product"""
    ctx = ctx or get_context()
    assert len(g1_points) == len(g2_points)
    g1 = _points_array(g1_points, 1, "pairing_product: G1 points")
    g2 = _points_array(g2_points, 2, "pairing_product: twist points")
    gt, ones = _pairing_product_arrays(ctx, g1, g2, offsets, want_gt=True)
    return [GT.from_bytes(gt[384 * k:384 * k + 384]) for k in range(len(offsets) - 1)], ones


def _points_array(points, group, what):
    enc = [_as_bytes(p) for p in points]
    if any(g != group for g, _ in enc):
        raise ValueError(f"{what}: wrong group")
    width = 64 if group == 1 else 128
    return np.frombuffer(b"".join(r for _, r in enc), np.uint8).reshape(-1, width)


def _pairing_product_arrays(ctx, g1, g2, offsets, want_gt=False, validate=True):
    n, n_products = len(g1), len(offsets) - 1
    off = np.asarray(offsets, dtype=np.uint32)
    if n_products < 1 or off[0] != 0 or off[-1] != n or np.any(np.diff(off.astype(np.int64)) < 0):
        raise ValueError("offsets must rise from 0 to the number of pairs")
    d1, d2 = ctx.upload(g1) if n else ctx.alloc(64), ctx.upload(g2) if n else ctx.alloc(128)
    if validate:
        _validate(ctx, 1, d1, n, "pairing_product: G1 points")
        _validate(ctx, 2, d2, n, "pairing_product: twist points")
    doff, dones = ctx.upload(off), ctx.alloc(max(n_products, 1))
    dgt = ctx.alloc(384 * n_products) if want_gt else None
    ctx.bn256_pairing_product(d1.ptr, d2.ptr, n, doff.ptr, n_products, dones.ptr, dgt.ptr if dgt else None)
    ctx.sync()
    ones = [bool(v) for v in ctx.download(dones.ptr, n_products)]
    gt = ctx.download(dgt.ptr, 384 * n_products).tobytes() if want_gt else None
    return gt, ones


_P_WORDS = np.array([(P >> (32 * k)) & 0xFFFFFFFF for k in range(8)], dtype=np.int64)


def _neg_g1_rows(rows):
    """(n, 64) uint8 affine G1 points -> their negatives (y -> p - y; infinity stays all zero)"""
    out = np.array(rows, dtype=np.uint8, copy=True)
    if not len(out):
        return out
    y = out[:, 32:].copy().view("<u4").astype(np.int64)
    res = np.zeros_like(y)
    borrow = np.zeros(len(y), np.int64)
    for k in range(8):
        d = _P_WORDS[k] - y[:, k] - borrow
        borrow = (d < 0).astype(np.int64)
        res[:, k] = d + (borrow << 32)
    inf = ~out.any(axis=1)
    res[inf] = 0
    out[:, 32:] = res.astype("<u4").view(np.uint8).reshape(-1, 32)
    return out


# proof elements in the order the verifier reads them (group 1 except the one twist element)
_PROOF_G1 = ("r_v*v_mid*g1", "r_y*y_mid*g1", "r_v*alpha_v*v_mid*g1", "r_w*alpha_w*w_mid*g1", "r_y*alpha_y*y_mid*g1",
             "r_v*beta*v_mid+r_w*beta*w_mid+r_y*beta*y_mid*g1", "h*g1")
_PROOF_G2 = "r_w*w_mid*g2"
_CHECKS = ("H", "V", "W", "Y", "Z")
# pairs per check, in order: H 3, V 2, W 2, Y 2, Z 3 (12 per proof)
_CHECK_OFFSETS = (0, 3, 5, 7, 9, 12)


class _VerifyingKey:
    """The verification key on the device: the bases of the three IO sums and the fixed pairing arguments,
    converted and validated once."""

    def __init__(self, ctx, qap, verikey):
        self.io = list(qap.indices_io)

        def pts(names, group):
            for name in names:
                if name not in verikey:
                    raise KeyError(name)
            arr = _points_array([verikey[n] for n in names], group, "verikey")
            buf = ctx.upload(arr)
            if ctx.bn256_validate(group, buf.ptr, len(names)):
                for j, name in enumerate(names):
                    one = ctx.upload(arr[j:j + 1])
                    _validate(ctx, group, one, 1, f"verikey[{name!r}]")
            return arr, buf

        self.v_bases = pts(["r_v*v0*g1"] + [f"r_v*v{i}*g1" for i in self.io], 1)[1]
        self.w_bases = pts(["r_w*w0*g2"] + [f"r_w*w{i}*g2" for i in self.io], 2)[1]
        self.y_bases = pts([f"r_y*y{i}*g1" for i in self.io], 1)[1]
        g1_fixed, _ = pts(["alpha_w*g1", "beta*gamma*g1"], 1)
        g2_fixed, _ = pts(["g2", "r_y*t*g2", "alpha_v*g2", "alpha_y*g2", "gamma*g2", "beta*gamma*g2"], 2)
        self.alpha_w_g1 = g1_fixed[0]
        self.neg_beta_gamma_g1 = _neg_g1_rows(g1_fixed[1:2])[0]
        (self.g2, self.r_y_t_g2, self.alpha_v_g2, self.alpha_y_g2, self.gamma_g2,
         self.beta_gamma_g2) = g2_fixed


def _proof_arrays(proofs):
    """(7, B, 64) G1 elements in _PROOF_G1 order and (B, 128) twist elements"""
    g1 = np.empty((len(_PROOF_G1), len(proofs), 64), np.uint8)
    g2 = np.empty((len(proofs), 128), np.uint8)
    for b, proof in enumerate(proofs):
        for k, name in enumerate(_PROOF_G1):
            grp, raw = _as_bytes(proof[name])
            if grp != 1:
                raise ValueError(f"proof {b}: {name!r} is not a G1 point")
            g1[k, b] = np.frombuffer(raw, np.uint8)
        grp, raw = _as_bytes(proof[_PROOF_G2])
        if grp != 2:
            raise ValueError(f"proof {b}: {_PROOF_G2!r} is not a twist point")
        g2[b] = np.frombuffer(raw, np.uint8)
    return g1, g2


def _first_bad(ctx, group, arr):
    """index of the first point of arr (n, width) that is not on its curve (arr holds at least one)"""
    lo, hi = 0, len(arr)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        buf = ctx.upload(arr[lo:mid])
        if ctx.bn256_validate(group, buf.ptr, mid - lo):
            hi = mid
        else:
            lo = mid
    return lo


def _verify_many(ctx, vk, proofs, cs):
    B = len(proofs)
    if B == 0:
        return []
    if len(cs) != B:
        raise ValueError("one witness per proof")
    pg1, pg2 = _proof_arrays(proofs)
    dg1, dg2 = ctx.upload(pg1), ctx.upload(pg2)
    for k, name in enumerate(_PROOF_G1):
        if ctx.bn256_validate(1, dg1.ptr + 64 * B * k, B):
            b = _first_bad(ctx, 1, pg1[k])
            raise ValueError(f"proof {b}: {name!r} is not on the BN-256 curve")
    if ctx.bn256_validate(2, dg2.ptr, B):
        b = _first_bad(ctx, 2, pg2)
        raise ValueError(f"proof {b}: {_PROOF_G2!r} is not on the BN-256 twist")
    # IO sums: A = v0 + sum c_i v_i + pi_v, Bt = w0 + sum c_i w_i + pi_w, C = -(sum c_i y_i + pi_y), Z = -(pi_v + pi_y)
    n_io = len(vk.io)
    one = (1).to_bytes(32, "little")
    c_io = scalars_to_array([int(c[i]) % ORDER for c in cs for i in vk.io]).reshape(B, n_io, 32)
    sc_vw = np.concatenate([np.tile(np.frombuffer(one, np.uint8), (B, 1, 1)), c_io], axis=1)
    d_vw, d_y = ctx.upload(np.ascontiguousarray(sc_vw)), ctx.upload(np.ascontiguousarray(c_io)) if n_io else None
    d_vy = ctx.upload(np.ascontiguousarray(np.stack([pg1[0], pg1[1]], axis=1)))
    outA, outB, outC, outZ = ctx.alloc(64 * B), ctx.alloc(128 * B), ctx.alloc(64 * B), ctx.alloc(64 * B)
    ctx.bn256_lincomb_batch(1, vk.v_bases.ptr, n_io + 1, d_vw.ptr, dg1.ptr, 1, B, False, outA.ptr)
    ctx.bn256_lincomb_batch(2, vk.w_bases.ptr, n_io + 1, d_vw.ptr, dg2.ptr, 1, B, False, outB.ptr)
    ctx.bn256_lincomb_batch(1, vk.y_bases.ptr if n_io else None, n_io, d_y.ptr if n_io else None,
                            dg1.ptr + 64 * B, 1, B, True, outC.ptr)
    ctx.bn256_lincomb_batch(1, None, 0, None, d_vy.ptr, 2, B, True, outZ.ptr)
    ctx.sync()
    A = ctx.download(outA.ptr, 64 * B).reshape(B, 64)
    Bt = ctx.download(outB.ptr, 128 * B).reshape(B, 128)
    C = ctx.download(outC.ptr, 64 * B).reshape(B, 64)
    Z = ctx.download(outZ.ptr, 64 * B).reshape(B, 64)
    v, y, av, aw, ay, beta, h = pg1
    g1 = np.empty((B, 12, 64), np.uint8)
    g2 = np.empty((B, 12, 128), np.uint8)
    # H: e(A, Bt) e(-(yio + pi_y), g2) e(-pi_h, r_y t g2) == 1
    g1[:, 0], g2[:, 0] = A, Bt
    g1[:, 1], g2[:, 1] = C, vk.g2
    g1[:, 2], g2[:, 2] = _neg_g1_rows(h), vk.r_y_t_g2
    # V: e(pi_v, alpha_v g2) e(-pi_av, g2) == 1
    g1[:, 3], g2[:, 3] = v, vk.alpha_v_g2
    g1[:, 4], g2[:, 4] = _neg_g1_rows(av), vk.g2
    # W: e(alpha_w g1, pi_w) e(-pi_aw, g2) == 1
    g1[:, 5], g2[:, 5] = vk.alpha_w_g1, pg2
    g1[:, 6], g2[:, 6] = _neg_g1_rows(aw), vk.g2
    # Y: e(pi_ay, g2) e(-pi_y, alpha_y g2) == 1
    g1[:, 7], g2[:, 7] = ay, vk.g2
    g1[:, 8], g2[:, 8] = _neg_g1_rows(y), vk.alpha_y_g2
    # Z: e(pi_beta, gamma g2) e(-(pi_v + pi_y), beta gamma g2) e(-beta gamma g1, pi_w) == 1
    g1[:, 9], g2[:, 9] = beta, vk.gamma_g2
    g1[:, 10], g2[:, 10] = Z, vk.beta_gamma_g2
    g1[:, 11], g2[:, 11] = vk.neg_beta_gamma_g1, pg2
    offsets = (np.arange(B, dtype=np.int64)[:, None] * 12 + np.array(_CHECK_OFFSETS[:-1])).reshape(-1)
    offsets = np.append(offsets, 12 * B)
    _, ones = _pairing_product_arrays(ctx, g1.reshape(-1, 64), g2.reshape(-1, 128), offsets, validate=False)
    return [dict(zip(_CHECKS, ones[5 * b:5 * b + 5])) for b in range(B)]


def verify(qap, verikey, proof, c, ctx=None):
    """The reference's verify (trinocchio/pynocchio.py:276-325): {"H", "V", "W", "Y", "Z"} -> bool.  Each check
    lhs == rhs is evaluated as the equivalent product of pairings == 1 (the right-hand side's G1 argument negated,
    the point sums folded into the IO linear combinations as terms of coefficient 1); the five products run in ONE
    launch.  Reads only qap.indices_io.  Points not on their curve raise ValueError (the reference would compute on
    them); G2 subgroup membership is not checked."""
    ctx = ctx or get_context()
    return _verify_many(ctx, _VerifyingKey(ctx, qap, verikey), [proof], [c])[0]


def verify_batch(qap, verikey, proofs, cs, ctx=None):
    """[verify(qap, verikey, p, c) for p, c in zip(proofs, cs)] with the key uploaded once, each IO sum of all proofs
    in one launch and all 12 B pairings in one product launch"""
    ctx = ctx or get_context()
    return _verify_many(ctx, _VerifyingKey(ctx, qap, verikey), list(proofs), list(cs))


# ---- key generation (trinocchio/pynocchio.py:36-200; csrc/bn256_keygen.hip) -----------------------------------------

prng = random.SystemRandom()


class Trapdoor:
    """The reference's trapdoor: r_v, r_w, s, alpha_v, alpha_w, alpha_y, beta, gamma drawn from this module's `prng` in
    that order, r_y = r_v r_w mod modulus (pynocchio.py:36-49)."""

    def __init__(self, modulus):
        _td = list(prng.randrange(modulus) for i in range(8))
        r_v, r_w, s, alpha_v, alpha_w, alpha_y, beta, gamma = _td
        self.r_v = r_v
        self.r_w = r_w
        self.r_y = r_v * r_w % modulus
        self.s = s
        self.alpha_v = alpha_v
        self.alpha_w = alpha_w
        self.alpha_y = alpha_y
        self.beta = beta
        self.gamma = gamma


class SampleDeltas:
    """delta_v, delta_w, delta_y from `prng` (pynocchio.py:52-58)"""

    def __init__(self, modulus):
        self.v, self.w, self.y = (prng.randrange(modulus) for i in range(3))


def _generator(ctx, pt, group, what):
    """(device buffer, host bytes) of a generator, checked to be on its curve"""
    grp, raw = _as_bytes(pt)
    name = "BN-256 curve" if group == 1 else "BN-256 twist"
    if grp != group:
        raise ValueError(f"{what}: not a point of the {name}")
    buf = ctx.upload(np.frombuffer(raw, np.uint8))
    if ctx.bn256_validate(group, buf.ptr, 1):
        raise ValueError(f"{what}: generator not on the {name}")
    return buf, raw


def _fixed_base_points(ctx, group, base_buf, exps_ptr, n):
    """n device scalars -> list of points exps[i] * base"""
    if not n:
        return []
    width = 64 * group
    out = ctx.alloc(width * n)
    ctx.bn256_fixed_base(group, base_buf.ptr, exps_ptr, n, out.ptr)
    ctx.sync()
    raw = ctx.download(out.ptr, width * n).tobytes()
    cls = BN256Point if group == 1 else BN256TwistPoint
    return [cls.from_bytes(raw[width * i:width * i + width]) for i in range(n)]


class Generators:
    """g1, g2 and the scaled generators r_v g1, r_w g1, r_w g2, r_y g1, r_y g2 (pynocchio.py:61-69), made by one
    fixed-base launch per group.  g1 / g2 may be foreign (MPyC-style) points; off-curve generators raise ValueError."""

    def __init__(self, td, g1, g2, ctx=None):
        ctx = ctx or get_context()
        b1, raw1 = _generator(ctx, g1, 1, "Generators: g1")
        b2, raw2 = _generator(ctx, g2, 2, "Generators: g2")
        self.g1, self.g2 = BN256Point.from_bytes(raw1), BN256TwistPoint.from_bytes(raw2)
        e1 = ctx.upload(_native.ints_to_array([int(td.r_v) % ORDER, int(td.r_w) % ORDER, int(td.r_y) % ORDER], 32))
        e2 = ctx.upload(_native.ints_to_array([int(td.r_w) % ORDER, int(td.r_y) % ORDER], 32))
        self.g1_v, self.g1_w, self.g1_y = _fixed_base_points(ctx, 1, b1, e1.ptr, 3)
        self.g2_w, self.g2_y = _fixed_base_points(ctx, 2, b2, e2.ptr, 2)


def _matrix_entries(M, n_cols=None):
    """(rows, cols, values (nnz, 32), n_rows, n_cols) of one constraint matrix: a tuple (row_ptr, col, vals) is CSR,
    a list of rows (code_to_r1cs.flatcode_to_r1cs) or a 2-D array is dense"""
    if isinstance(M, tuple):
        rows, col, v, n_rows = csr_entries(*M, ORDER, False, "R1CSQAP")      # values >= ORDER: the device reduces them
        return rows, col, v, n_rows, n_cols
    dense = [[int(x) for x in row] for row in M]
    n_rows = len(dense)
    width = len(dense[0]) if dense else 0
    if any(len(r) != width for r in dense):
        raise ValueError("R1CSQAP: dense rows of different lengths")
    rows, cols, ints = [], [], []
    for r, row in enumerate(dense):
        for c, x in enumerate(row):
            if x % ORDER:
                rows.append(r)
                cols.append(c)
                ints.append(x % ORDER)
    return (np.asarray(rows, np.int64), np.asarray(cols, np.int64), scalars_to_array(ints).reshape(-1, 32), n_rows,
            width)


class R1CSQAP:
    """A QAP given by its sparse R1CS: constraint j (row j - 1) is interpolated at x = j, t(x) = prod_{j=1..d} (x - j),
    the convention of the reference's code_to_qap.QAP (qap_creator.r1cs_to_qap_ff) - but the v/w/y/t coefficients are
    never formed: key generation evaluates v_i(s) = sum_j V[j][i] l_j(s) on the device in O(nnz + d).

    V, W, Y: each a tuple (row_ptr, col, vals) in CSR form (vals: (nnz, 32) uint8, or ints - negative ones and ones
    >= the group order included - reduced mod the order; duplicate (row, col) entries add), or the reference's dense
    row lists (code_to_r1cs.flatcode_to_r1cs).  Column 0 is the constant wire "one", 1..out_ix the io wires, the rest
    mid wires.  m: the number of wires without "one" (default: from the matrices)."""

    def __init__(self, V, W, Y, out_ix, m=None):
        mats = [_matrix_entries(M) for M in (V, W, Y)]
        ds = {e[3] for e in mats}
        if len(ds) != 1:
            raise ValueError("R1CSQAP: V, W and Y must have the same number of rows")
        self.d = ds.pop()
        if self.d < 1:
            raise ValueError("R1CSQAP: at least one constraint")
        widths = [e[4] for e in mats if e[4] is not None]
        top = max([int(e[1].max()) + 1 for e in mats if len(e[1])] + widths + [out_ix + 1])
        self.m = top - 1 if m is None else int(m)
        n_wires = self.m + 1
        for e in mats:
            if len(e[1]) and (e[1].min() < 0 or e[1].max() >= n_wires):
                raise ValueError("R1CSQAP: a column index outside 0..m")
        if not 0 <= out_ix <= self.m:
            raise ValueError("R1CSQAP: out_ix outside 0..m")
        self.out_ix = int(out_ix)
        self.indices = range(self.m + 1)
        self.indices_io_and_0 = range(0, self.out_ix + 1)
        self.indices_io = range(1, self.out_ix + 1)
        self.indices_mid = range(self.out_ix + 1, self.m + 1)
        self._rows = np.concatenate([e[0] for e in mats])
        self._cols = np.concatenate([e[1] + k * n_wires for k, e in enumerate(mats)])
        self._vals = np.concatenate([e[2] for e in mats]) if len(self._cols) else np.zeros((0, 32), np.uint8)
        self._plans = {}

    def _plan(self, ctx):
        key = id(ctx)
        if key not in self._plans:
            self._plans[key] = (ctx, ColumnPlan(ctx, self._cols, self._rows, self._vals, 3 * (self.m + 1)))
        return self._plans[key][1]


def _dense_plan(ctx, qap):
    """a reference QAP's coefficient polynomials as columns (v_0..v_m, w_0..w_m, y_0..y_m, t), rows = degrees"""
    polys = list(qap.v) + list(qap.w) + list(qap.y) + [qap.t]
    rows, cols, ints = [], [], []
    top = 0
    for c, poly in enumerate(polys):
        coeffs = poly.coeffs if hasattr(poly, "coeffs") else poly
        top = max(top, len(coeffs))
        for k, x in enumerate(coeffs):
            x = int(x) % ORDER
            if x:
                rows.append(k)
                cols.append(c)
                ints.append(x)
    vals = scalars_to_array(ints).reshape(-1, 32)
    return ColumnPlan(ctx, np.asarray(cols, np.int64), np.asarray(rows, np.int64), vals, len(polys)), top


def _scalar_buf(ctx, values):
    return ctx.upload(_native.ints_to_array([int(v) % ORDER for v in values], 32))


class _QAPAtS:
    """v_i(s), w_i(s), y_i(s), t(s) (vwyt: 3 (m + 1) + 1 device scalars) and 1, s, .., s^d (powers) of one QAP"""

    def __init__(self, ctx, qap, s):
        self.n_wires = len(qap.indices)
        d = int(qap.d)
        self.d = d
        nw = self.n_wires
        self.vwyt = ctx.alloc(32 * (3 * nw + 1))
        self.t_ptr = self.vwyt.ptr + 32 * 3 * nw
        sb = _scalar_buf(ctx, [s, 1])
        self._keep = [sb]
        if isinstance(qap, R1CSQAP):
            plan, n_pow = qap._plan(ctx), d + 1
        else:
            plan, top = _dense_plan(ctx, qap)
            n_pow = max(d + 1, top)
            self._keep.append(plan)
        self.powers = ctx.alloc(32 * n_pow)
        ctx.upload_into(self.powers.ptr, _native.ints_to_array([1], 32))
        ctx.bn256_fr_powers(sb.ptr, sb.ptr + 32, n_pow - 1, self.powers.ptr + 32)
        if isinstance(qap, R1CSQAP):
            self.ell = ctx.alloc(32 * d)
            ctx.bn256_qap_lagrange(sb.ptr, d, self.ell.ptr, self.t_ptr)
            plan.run(self.ell.ptr, d, self.vwyt.ptr)
        else:
            plan.run(self.powers.ptr, n_pow, self.vwyt.ptr)

    def exps(self, ctx, td, wires):
        """device buffer of the seven exponent vectors (len(wires) + 3 rows each, csrc/bn256_keygen.hip) for `wires`"""
        n = len(wires)
        coef = _scalar_buf(ctx, [td.r_v, td.r_w, td.r_y, td.alpha_v * td.r_v, td.alpha_w * td.r_w,
                                 td.alpha_y * td.r_y, td.beta * td.r_v, td.beta * td.r_w, td.beta * td.r_y])
        idx = ctx.upload(np.asarray(list(wires), np.uint32)) if n else ctx.alloc(4)
        out = ctx.alloc(32 * 7 * (n + 3))
        ctx.bn256_keygen_exps(coef.ptr, self.vwyt.ptr, self.n_wires, self.t_ptr, idx.ptr, n, out.ptr)
        self._keep += [coef, idx]
        return out


# evalkey names per exponent vector of csrc/bn256_keygen.hip, in the reference's order (pynocchio.py:106-140)
_EVAL_NAMES = (lambda i: f"r_v*v{i}*g1", lambda i: f"r_w*w{i}*g2", lambda i: f"r_y*y{i}*g1",
               lambda i: f"r_v*alpha_v*v{i}*g1", lambda i: f"r_w*alpha_w*w{i}*g1", lambda i: f"r_y*alpha_y*y{i}*g1",
               lambda i: f"r_v*beta*v+r_w*beta*w+r_y*beta*y{i}_g1")
# zero-knowledge entries (pynocchio.py:143-154): (name, exponent vector, tail row); "t*g1" is t(s) itself
_ZK_ENTRIES = (("r_v*t*g1", 0, 0), ("r_w*t*g2", 1, 0), ("r_y*t*g1", 2, 2), ("r_v*alpha_v*t*g1", 3, 0),
               ("r_w*alpha_w*t*g1", 4, 1), ("r_y*alpha_y*t*g1", 5, 2), ("r_v*beta*t*g1", 6, 0),
               ("r_w*beta*t*g1", 6, 1), ("r_y*beta*t*g1", 6, 2))


def evalkey_vectors(td, qap, gen, ctx=None):
    """The evaluation key's point vectors on the device, as PreparedKey.generate tabulates them: {element of
    compute_proof (or "h*g1"): (group, device buffer of affine points, count)}; each element's vector holds its
    per-wire points over qap.indices_mid, then its zero-knowledge tail (_tail_slots: infinity where unused)."""
    return _evalkey_device(td, qap, gen, ctx or get_context())[0]


def _evalkey_device(td, qap, gen, ctx):
    b1, _ = _generator(ctx, gen.g1, 1, "generate: gen.g1")
    b2, _ = _generator(ctx, gen.g2, 2, "generate: gen.g2")
    at = _QAPAtS(ctx, qap, td.s)
    mid = list(qap.indices_mid)
    n = len(mid)
    exps = at.exps(ctx, td, mid)
    out = {}
    for k, (name, (_, zk)) in enumerate(_ELEMENTS.items()):
        group, base = (2, b2) if name.endswith("g2") else (1, b1)
        count = n + len(_tail_slots(name, zk))
        pts = ctx.alloc(64 * group * count)
        ctx.bn256_fixed_base(group, base.ptr, exps.ptr + 32 * k * (n + 3), count, pts.ptr)
        out[name] = (group, pts, count)
    pts = ctx.alloc(64 * (at.d + 1))
    ctx.bn256_fixed_base(1, b1.ptr, at.powers.ptr, at.d + 1, pts.ptr)
    out["h*g1"] = (1, pts, at.d + 1)
    ctx.sync()
    return out, at, b1


def _points_of(ctx, group, buf, count):
    width = 64 * group
    raw = ctx.download(buf.ptr, width * count).tobytes()
    cls = BN256Point if group == 1 else BN256TwistPoint
    return [cls.from_bytes(raw[width * i:width * i + width]) for i in range(count)]


def generate_evalkey(td, qap, gen, ctx=None):
    """The reference's generate_evalkey (pynocchio.py:101-167): the same names in the same order, every point equal to
    the reference's for the same td.  Each entry is one fixed-base product of g1 or g2 by an exponent made on the device
    (v_i(s), w_i(s), y_i(s), t(s) by csrc/bn256_keygen.hip).  qap: a reference QAP or an R1CSQAP."""
    ctx = ctx or get_context()
    vecs, at, b1 = _evalkey_device(td, qap, gen, ctx)
    mid = list(qap.indices_mid)
    n = len(mid)
    pts = {name: _points_of(ctx, *vecs[name]) for name in vecs}
    names = list(_ELEMENTS)
    key = {}
    for k in range(6):
        key.update((_EVAL_NAMES[k](i), pts[names[k]][j]) for j, i in enumerate(mid))
    key.update(("s^" + str(i) + "*g1", p) for i, p in enumerate(pts["h*g1"]))
    key.update((_EVAL_NAMES[6](i), pts[names[6]][j]) for j, i in enumerate(mid))
    for zname, k, row in _ZK_ENTRIES:
        key[zname] = pts[names[k]][n + row]
    key["t*g1"] = _fixed_base_points(ctx, 1, b1, at.t_ptr, 1)[0]
    return key


def generate_verikey(td, qap, gen, ctx=None):
    """The reference's generate_verikey (pynocchio.py:170-200): same names, order and points."""
    ctx = ctx or get_context()
    b1, raw1 = _generator(ctx, gen.g1, 1, "generate_verikey: gen.g1")
    b2, raw2 = _generator(ctx, gen.g2, 2, "generate_verikey: gen.g2")
    at = _QAPAtS(ctx, qap, td.s)
    io0 = list(qap.indices_io_and_0)
    n = len(io0)
    exps = at.exps(ctx, td, io0)
    s1 = _scalar_buf(ctx, [td.alpha_w, td.beta * td.gamma])
    s2 = _scalar_buf(ctx, [td.alpha_v, td.alpha_y, td.gamma, td.beta * td.gamma])
    aw_g1, bg_g1 = _fixed_base_points(ctx, 1, b1, s1.ptr, 2)
    av_g2, ay_g2, g_g2, bg_g2 = _fixed_base_points(ctx, 2, b2, s2.ptr, 4)
    ryt_g2 = _fixed_base_points(ctx, 2, b2, exps.ptr + 32 * (2 * (n + 3) + n + 2), 1)[0]
    v = _fixed_base_points(ctx, 1, b1, exps.ptr, n)
    w = _fixed_base_points(ctx, 2, b2, exps.ptr + 32 * (n + 3), n)
    y = _fixed_base_points(ctx, 1, b1, exps.ptr + 32 * 2 * (n + 3), n)
    key = {"g1": BN256Point.from_bytes(raw1), "g2": BN256TwistPoint.from_bytes(raw2), "alpha_v*g2": av_g2,
           "alpha_w*g1": aw_g1, "alpha_y*g2": ay_g2, "gamma*g2": g_g2, "beta*gamma*g1": bg_g1,
           "beta*gamma*g2": bg_g2, "r_y*t*g2": ryt_g2}
    key.update((f"r_v*v{i}*g1", v[j]) for j, i in enumerate(io0))
    key.update((f"r_w*w{i}*g2", w[j]) for j, i in enumerate(io0))
    key.update((f"r_y*y{i}*g1", y[j]) for j, i in enumerate(io0))
    return key


def _prepared_generate(cls, td, qap, gen, ctx=None):
    """PreparedKey(qap, generate_evalkey(td, qap, gen)) without the host round trip: the exponent vectors stay on the
    device, go to bn256_fixed_base, and the points to _KeyVector.from_device (validated and tabulated there)"""
    ctx = ctx or get_context()
    vecs = evalkey_vectors(td, qap, gen, ctx)
    key = cls.__new__(cls)
    key.ctx = ctx
    key.mid = list(qap.indices_mid)
    key.mid_index = np.asarray(key.mid, dtype=np.int64)
    key.vectors, key.zk_missing = {}, {}
    for name, (group, pts, count) in vecs.items():
        key.vectors[name] = _KeyVector.from_device(ctx, group, pts, count)
    return key


PreparedKey.generate = classmethod(_prepared_generate)


# ---- the prover's h (trinocchio/pynocchio.py:203-225; csrc/bn256_qap_h.hip) ------------------------------------------

class HPoly:
    """compute_h's result: h's coefficients in device memory (`buf`, 32 bytes each, lowest first, `len()` of them, made
    on `ctx`'s stream).  `.coeffs` downloads them once, as Python ints - what the reference's Poly offers.  `buf` is
    anything with a `.ptr` that keeps the memory alive: a whole buffer, or compute_h_batch's view into its K rows."""

    def __init__(self, ctx, buf, n):
        self.ctx, self.buf, self._n, self._coeffs = ctx, buf, n, None

    def __len__(self):
        return self._n

    @property
    def coeffs(self):
        if self._coeffs is None:
            self.ctx.sync()
            raw = self.ctx.download(self.buf.ptr, 32 * self._n).tobytes() if self._n else b""
            self._coeffs = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(self._n)]
        return self._coeffs


def _witness_array(qap, c):
    """the witness over qap.indices as (n_wires, 32) uint8 (any 32-byte values: the device reduces them)"""
    n_wires = len(qap.indices)
    if isinstance(c, np.ndarray):
        arr = _native.as_bytes_array(c, 32)
        if len(arr) != n_wires:
            raise ValueError(f"compute_h: the witness has {len(arr)} rows, the QAP {n_wires} wires")
        return arr
    return scalars_to_array([c[i] for i in qap.indices])


def _per_ctx(qap, name, ctx, make):
    """a device object of `qap` made once per context (kept on the QAP object)"""
    cache = qap.__dict__.setdefault("_h_cache", {})
    key = (name, id(ctx))
    if key not in cache:
        cache[key] = (ctx, make())
    return cache[key][1]


def _row_plan(ctx, qap):
    """an R1CSQAP's entries in ROW order (a, b, y stacked: 3 d sums), for vmpc_bn256_qap_colsum_dev with basis = c"""
    n_wires = qap.m + 1
    kind, wire = qap._cols // n_wires, qap._cols % n_wires
    return ColumnPlan(ctx, qap._rows + kind * qap.d, wire, qap._vals, 3 * qap.d)


def _coeff_plan(ctx, qap):
    """a reference QAP's coefficients with the roles exchanged: "column" = (polynomial kind, degree), "row" = wire, so
    that the column sums against c are the coefficients of V, W and Y -> (plan, coefficients per polynomial)"""
    top = max([len(p.coeffs if hasattr(p, "coeffs") else p) for polys in (qap.v, qap.w, qap.y) for p in polys] + [1])
    rows, cols, ints = [], [], []
    for kind, polys in enumerate((qap.v, qap.w, qap.y)):
        for i, poly in zip(qap.indices, polys):
            for k, x in enumerate(poly.coeffs if hasattr(poly, "coeffs") else poly):
                x = int(x) % ORDER
                if x:
                    rows.append(i)
                    cols.append(kind * top + k)
                    ints.append(x)
    vals = scalars_to_array(ints).reshape(-1, 32)
    return ColumnPlan(ctx, np.asarray(cols, np.int64), np.asarray(rows, np.int64), vals, 3 * top), top


def _t_coeffs(ctx, qap):
    """device buffer of t's d + 1 coefficients, made once per (context, QAP)"""
    d = int(qap.d)

    def make():
        out = ctx.alloc(32 * (d + 1))
        if isinstance(qap, R1CSQAP):
            scratch = ctx.alloc(64 * (d + (d + 127) // 128))
            ctx.bn256_qap_t_coeffs(d, scratch.ptr, out.ptr)
            ctx.sync()
        else:
            t = [int(x) % ORDER for x in qap.t.coeffs]
            if len(t) != d + 1:
                raise ValueError("compute_h: qap.t must have d + 1 coefficients")
            ctx.upload_into(out.ptr, _native.ints_to_array(t, 32))
        return out
    return _per_ctx(qap, "t", ctx, make)


def _check_cap(qap, who):
    d = int(qap.d)
    if d + 1 > _native.BN256_FR_POLY_MAX:
        raise ValueError(f"{who}: d + 1 = {d + 1} exceeds the polynomial product's cap {_native.BN256_FR_POLY_MAX}")


def compute_h(qap, c, deltas=None, ctx=None):
    """The reference's h, coefficient for coefficient and length included (pynocchio.py:203-225): with `deltas`
    h + compute_h_zk_terms(qap, c, deltas), d + 1 coefficients; without, p / qap.t, max(d - 1, 0) coefficients (top
    zeros kept).  qap: an R1CSQAP or a reference QAP; c: as compute_proof takes it (ints / field elements indexable by
    qap.indices, negative or >= the order reduced, or an (n_wires, 32) uint8 array).  All O(d^2) work runs on the
    device; the result (an HPoly) stays there and compute_proof over a PreparedKey reads it in place.  A witness that
    violates a constraint raises ValueError naming the first violated constraint (1-based, the point x = j).
    compute_h_batch's pipeline (_h_batch) on one row."""
    _check_cap(qap, "compute_h")
    return _h_batch(ctx or get_context(), qap, _witness_array(qap, c)[None], None if deltas is None else [deltas],
                    "compute_h: the witness")[0]


def _moments_by_tree(ctx, d):
    """whether the context's mode (device.moment_transform) sends d constraints to the subproduct tree"""
    mode = getattr(ctx, "moment_transform", "direct")
    return mode == "tree" or (mode == "auto" and d >= _native.BN256_QAP_MTREE_MIN)


def _mtree_plan(ctx, qap, d):
    """device buffer of the moment transform's plan for d points and n_max = d (csrc/bn256_qap_mtree.hip), made once
    per (context, QAP): (L + 1) d' + 2^(L+1) - 1 + 3 d scalars, 126 MB at d = 2^18 and 570 MB at 2^20"""
    def make():
        plan = ctx.alloc(_native.bn256_qap_mtree_bytes(d, d))
        ctx.bn256_qap_mtree_build(d, d, plan.ptr)
        return plan
    return _per_ctx(qap, "mtree", ctx, make)


def _h_rows(ctx, d, t, aby_ptr, n, dd, out_ptr, out_stride, qap=None):
    """weights -> moments -> combination for n rows a || b || y, 3 d scalars apart, at aby_ptr ->
    n rows of h at out_ptr; dd: device buffer of the rows' three deltas each, or None.  The moments come from the
    subproduct tree where the context's device.moment_transform mode says so and `qap`, which
    keeps the plan, is given; the bits are the same.  Ends with the stream drained, so the caller may release what the
    rows were made from."""
    u = ctx.alloc(32 * 2 * d * n)                # rows ua || ub, stride 2 d; the moments alike
    ctx.bn256_qap_h_weights_batch(aby_ptr, aby_ptr + 32 * d, 3 * d, d, u.ptr, u.ptr + 32 * d, 2 * d, n)
    mom = ctx.alloc(32 * 2 * d * n)
    if qap is not None and _moments_by_tree(ctx, d):
        plan = _mtree_plan(ctx, qap, d)
        tree_scratch = ctx.alloc(_native.bn256_qap_moments_tree_scratch_bytes(d, n))
        ctx.bn256_qap_moments_tree_batch(plan.ptr, d, d, u.ptr, u.ptr + 32 * d, 2 * d, d, mom.ptr, mom.ptr + 32 * d,
                                         2 * d, tree_scratch.ptr, n)
    else:
        ctx.bn256_qap_moments_batch(u.ptr, u.ptr + 32 * d, 2 * d, d, d, mom.ptr, mom.ptr + 32 * d, 2 * d, n)
    scratch = ctx.alloc(32 * 3 * d * n)
    ctx.bn256_qap_h_combine_batch(mom.ptr, mom.ptr + 32 * d, 2 * d, t.ptr, d, None if dd is None else dd.ptr, scratch.ptr,
                                  out_ptr, out_stride, n)
    ctx.sync()      # the temporaries above may be released once the stream has drained


def compute_h_share(qap, c_share, delta_shares=None, ctx=None):
    """compute_h for ONE PARTY's Shamir share of the witness (demos/demo_zkp_trinocchio.py:70-79 computes h in the clear
    and shares its coefficients): the same row values -> weights -> moments -> combination on the party's share vector,
    WITHOUT the constraint check - a share vector never satisfies a_j b_j = y_j - and without a host read-back before
    the result.  deg Y < d, so what comes out is the polynomial part of V W / t, which is bilinear in the shares (plus
    linear in delta_y): from degree-t sharings of c and of the deltas the M parties' results are a degree-2t SHARING of
    the h that compute_h(qap, c, deltas) gives, coefficient for coefficient - M >= 2t + 1 parties recombine it with the
    Lagrange weights at 0, no exchange needed.  delta_shares: this party's shares as .v, .w, .y, or a device buffer of
    those three scalars.  Lengths as compute_h: d + 1 with deltas, max(d - 1, 0) without.  (Whether the shared witness
    satisfies the constraints is trinocchio.prove's residual check, vmpc_bn256_qap_residual_batch_dev.)
    compute_h_share_batch's pipeline (_h_batch without the check) on one row."""
    _check_cap(qap, "compute_h_share")
    if delta_shares is not None and not hasattr(delta_shares, "ptr"):
        delta_shares = [delta_shares]
    return _h_batch(ctx or get_context(), qap, _witness_array(qap, c_share)[None], delta_shares, None)[0]


# ---- h for K witnesses of one QAP -------------------------------------------------------------

BATCH_BUDGET_BYTES = 1 << 30     # device bytes one chunk of a batch may hold at a time (compute_h_batch)


class _BufferView:
    """`nbytes` of a device buffer from byte `offset` on; holds the buffer"""
    __slots__ = ("base", "ptr", "nbytes")

    def __init__(self, base, offset, nbytes):
        self.base, self.ptr, self.nbytes = base, base.ptr + offset, nbytes


def witness_batch_array(n_wires, cs, indices=None):
    """K witnesses -> (K, n_wires, 32) uint8: `cs` is that array already (any 32-byte values), or K witnesses as
    compute_h takes them (each indexable by `indices`, default range(n_wires), or an (n_wires, 32) array).  A witness
    with another number of rows raises ValueError.  Pure: needs no device."""
    if isinstance(cs, np.ndarray) and cs.ndim == 3:
        arr = np.ascontiguousarray(cs, dtype=np.uint8)
        if arr.shape[1:] != (n_wires, 32):
            raise ValueError(f"compute_h_batch: the witnesses have {arr.shape[1]} rows of {arr.shape[2]} bytes, the QAP "
                             f"{n_wires} wires of 32")
        return arr
    cs = list(cs)
    out = np.empty((len(cs), n_wires, 32), np.uint8)
    idx = range(n_wires) if indices is None else indices
    for w, c in enumerate(cs):
        if isinstance(c, np.ndarray):
            a = _native.as_bytes_array(c, 32)
            if len(a) != n_wires:
                raise ValueError(f"compute_h_batch: witness {w} has {len(a)} rows, the QAP {n_wires} wires")
        else:
            if isinstance(c, (list, tuple)) and len(c) != n_wires:
                raise ValueError(f"compute_h_batch: witness {w} has {len(c)} rows, the QAP {n_wires} wires")
            a = scalars_to_array([c[i] for i in idx])
        out[w] = a
    return out


def plan_chunks(k, budget, cost):
    """[(start, stop), ..]: 0..k cut into consecutive chunks, each the longest whose cost(n) (device bytes of n witnesses,
    non-decreasing in n) stays within `budget` - but never empty: a budget below one witness gives one witness per
    chunk.  Pure."""
    chunks, start = [], 0
    while start < k:
        lo, hi = 1, k - start               # the largest n in [1, hi] with cost(n) <= budget, 1 if there is none
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if cost(mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        chunks.append((start, start + lo))
        start += lo
    return chunks


def h_batch_bytes(d, n_wires, n_coef, n, tree=False):
    """device bytes compute_h_batch holds for a chunk of n witnesses: per witness the witness itself, the row values
    (3 d), the weighted rows (2 d), the moments (2 d), the combination's scratch (3 d) and, for a dense QAP, 3 n_coef
    coefficients; plus the arenas of the moments and of the two half products.  tree: the moments by the subproduct
    tree (device.moment_transform) - its scratch (4 d' scalars a witness) and its arena in place of the direct
    kernel's; the plan, which is the QAP's and not the chunk's, is not counted."""
    if n == 0:
        return 0
    per = 32 * (n_wires + 10 * d + 3 * n_coef)
    if tree:
        moments = _native.bn256_qap_moments_tree_batch_bytes(d, d, n)
        scratch = _native.bn256_qap_moments_tree_scratch_bytes(d, n)
    else:
        moments, scratch = _native.bn256_qap_moments_batch_bytes(d, d, n), 0
    arena = max(moments,
                _native.bn256_fr_poly_mul_batch_bytes(d, d, 0, d - 1, n),
                _native.bn256_fr_poly_mul_batch_bytes(d, d, d - 1, d, n))
    return per * n + scratch + arena


def compute_h_batch(qap, cs, deltas=None, ctx=None):
    """[compute_h(qap, cs[w], deltas[w]) for w in range(K)], coefficient for coefficient and length included, with every
    stage run once for all K (csrc/bn256_qap_h.hip's *_batch_dev entries).  cs: K witnesses as compute_h takes them, or
    one (K, n_wires, 32) uint8 array (uploaded as it is); deltas: None, or K objects with .v .w .y.  -> a list of K HPoly,
    each a view into ONE device buffer of K rows of d + 1 scalars, which it keeps alive; compute_proof and
    compute_proof_batch read them in place.
    Stage-major: upload, K queued runs of the row-value plan, ONE check launch and one read of K words - a violated
    witness raises ValueError naming the lowest bad witness (0-based) and its first violated constraint (1-based) before
    weights, moments or products are launched - then weights, moments, combination and one synchronisation.  K is cut
    into consecutive chunks that hold at most BATCH_BUDGET_BYTES of device memory each (plan_chunks, h_batch_bytes); a
    chunk boundary changes no value."""
    _check_cap(qap, "compute_h_batch")
    arr = witness_batch_array(len(qap.indices), cs, qap.indices)
    deltas = None if deltas is None else list(deltas)
    if deltas is not None and len(deltas) != len(arr):
        raise ValueError("compute_h_batch: one set of deltas per witness")
    if len(arr) == 0:
        return []
    return _h_batch(ctx or get_context(), qap, arr, deltas, "compute_h_batch: witness {w}")


def _h_batch(ctx, qap, arr, deltas, check):
    """The h pipeline behind compute_h, compute_h_share and their batch forms: K >= 1 witnesses (or share vectors) of one
    QAP, a (K, n_wires, 32) array -> K HPoly views into one device buffer.  One range of batch_ranges at a time: upload
    and row values (_upload_row_values_batch), the constraint check, then weights, moments and combination
    (_h_from_rows).  deltas: None, a device buffer of 3 K scalars, or K objects with .v .w .y.  check: None for share
    vectors, which never satisfy a_j b_j = y_j; else how the ValueError for the lowest bad witness begins, formatted with
    w = that witness's index - it is raised before the range's weights, moments or products are launched."""
    d = int(qap.d)
    if deltas is not None and not hasattr(deltas, "ptr"):
        deltas = _scalar_buf(ctx, [getattr(dl, name) for dl in deltas for name in _DELTAS])

    def rows(lo, hi):
        aby, keep = _upload_row_values_batch(ctx, qap, arr[lo:hi])
        if check is not None:
            n = hi - lo
            bad = ctx.alloc(4 * n)
            ctx.bn256_qap_check_batch(aby.ptr, aby.ptr + 32 * d, aby.ptr + 64 * d, 3 * d, d, bad.ptr, n)
            ctx.sync()
            words = ctx.download(bad.ptr, 4 * n).view("<u4")
            viol = np.nonzero(words != 0xFFFFFFFF)[0]
            if len(viol):
                j = int(words[viol[0]]) + 1
                raise ValueError(f"{check.format(w=lo + int(viol[0]))} violates constraint {j} "
                                 f"(V(j) W(j) != Y(j) at j = {j})")
        return aby.ptr, (aby, keep)
    return _h_from_rows(ctx, qap, len(arr), deltas, rows)


# ---- h for K SHARE vectors of one QAP (trinocchio.prove_batch) ---------------------------------

def _share_batch_args(qap, c_shares, delta_shares, who):
    """the host half of compute_h_share_batch, which needs no device: -> ((K, n_wires, 32) array, deltas) with deltas
    None, a device buffer of 3 K scalars, or a list of K objects; ValueError for a wrong width or a wrong count"""
    _check_cap(qap, who)
    arr = witness_batch_array(len(qap.indices), c_shares, qap.indices)
    K = len(arr)
    if delta_shares is not None:
        if hasattr(delta_shares, "ptr"):       # a device buffer (its bytes) or a device vector (its scalars)
            have = delta_shares.nbytes // 32 if hasattr(delta_shares, "nbytes") else len(delta_shares)
        else:
            delta_shares = list(delta_shares)
            have = 3 * len(delta_shares)
        if have != 3 * K:
            raise ValueError(f"{who}: one set of three deltas per witness ({have} scalars for {K} witnesses)")
    return arr, delta_shares


def _upload_row_values_batch(ctx, qap, arr):
    """K witnesses or share vectors (a (K, n_wires, 32) array, K >= 1) on the device in ONE upload and their row values
    V(j), W(j), Y(j), K rows a || b || y of 3 d scalars, by K queued runs of the QAP's plan with no host wait between them
    -> (buffer, what must outlive the stream's work on it).  The only code that turns a witness into row values: _h_batch
    runs it range by range, trinocchio.prove_batch once, and reads the rows for the residual and for h."""
    K, n_wires, d = len(arr), arr.shape[1], int(qap.d)
    dc = ctx.upload(arr) if n_wires else ctx.alloc(32)
    aby = ctx.alloc(32 * 3 * d * K)
    if isinstance(qap, R1CSQAP):
        plan = _per_ctx(qap, "rows", ctx, lambda: _row_plan(ctx, qap))
        for w in range(K):
            plan.run(dc.ptr + 32 * n_wires * w, n_wires, aby.ptr + 32 * 3 * d * w)
        return aby, (dc,)
    plan, top = _per_ctx(qap, "coeffs", ctx, lambda: _coeff_plan(ctx, qap))
    coef = ctx.alloc(32 * 3 * top * K)
    for w in range(K):
        plan.run(dc.ptr + 32 * n_wires * w, n_wires, coef.ptr + 32 * 3 * top * w)
        ctx.bn256_qap_horner(coef.ptr + 32 * 3 * top * w, top, 3, d, aby.ptr + 32 * 3 * d * w)
    return aby, (dc, coef)


def batch_ranges(qap, K, tree=False):
    """[(start, stop), ..]: the K witnesses of a batch as compute_h_batch cuts them - plan_chunks under
    BATCH_BUDGET_BYTES, each chunk in pieces of at most BN256_QAP_MAX_WIT (the witness is a grid dimension); tree: as
    h_batch_bytes takes it.  Pure."""
    d, n_wires = int(qap.d), len(qap.indices)
    top = 0
    if not isinstance(qap, R1CSQAP):
        top = max([len(p.coeffs if hasattr(p, "coeffs") else p) for polys in (qap.v, qap.w, qap.y) for p in polys] + [1])
    out = []
    for lo, hi in plan_chunks(K, BATCH_BUDGET_BYTES, lambda n: h_batch_bytes(d, n_wires, top, n, tree)):
        n = min(hi - lo, _native.BN256_QAP_MAX_WIT)
        out += [(a, min(a + n, hi)) for a in range(lo, hi, n)]
    return out


def _h_from_rows(ctx, qap, K, dd, rows):
    """K rows of row values -> K HPoly views into one buffer of K rows of d + 1 scalars; dd: device buffer of the rows'
    three deltas each, or None.  rows(lo, hi) -> (device pointer to rows lo .. hi - 1, what must stay alive while the
    stream works on them), asked for once per range of batch_ranges, in order; the weights, moments and combination run
    once per range and a boundary changes no value.  Nothing here asks whether the rows satisfy a_j b_j = y_j: the
    result is the polynomial part of V W / t."""
    d = int(qap.d)
    t = _t_coeffs(ctx, qap)
    stride = d + 1
    out = ctx.alloc(32 * stride * K)
    for lo, hi in batch_ranges(qap, K, _moments_by_tree(ctx, d)):
        ptr, keep = rows(lo, hi)
        _h_rows(ctx, d, t, ptr, hi - lo, _BufferView(dd, 96 * lo, 96 * (hi - lo)) if dd is not None else None,
                out.ptr + 32 * stride * lo, stride, qap)
        del keep        # (_h_rows has drained the stream)
    n_h = d + 1 if dd is not None else max(d - 1, 0)
    return [HPoly(ctx, _BufferView(out, 32 * stride * w, 32 * stride), n_h) for w in range(K)]


def _h_from_row_values_batch(ctx, qap, aby, dd, K):
    """_h_from_rows on K rows that are on the device already (_upload_row_values_batch's buffer, which the caller holds):
    trinocchio.prove_batch's second step, after the residual has read the same rows"""
    return _h_from_rows(ctx, qap, K, dd, lambda lo, hi: (aby.ptr + 32 * 3 * int(qap.d) * lo, None))


def compute_h_share_batch(qap, c_shares, delta_shares=None, ctx=None):
    """[compute_h_share(qap, c_shares[w], delta_shares[w]) for w in range(K)], coefficient for coefficient and length
    included: compute_h_batch's pipeline (_h_batch: per range of batch_ranges one upload, the queued runs of the row-value
    plan, then weights, moments and combination) without the constraint check (a share vector never satisfies
    a_j b_j = y_j) and so without a host read-back before the result.  c_shares: one party's K share vectors as a
    (K, n_wires, 32) uint8 array, or K vectors as compute_h_share takes them; delta_shares: None, a device buffer of 3 K
    scalars (witness w's delta_v, delta_w, delta_y at 3 w .. 3 w + 2), or K objects with .v .w .y.  -> a list of K HPoly,
    each a view into ONE device buffer of K rows of d + 1 scalars."""
    arr, deltas = _share_batch_args(qap, c_shares, delta_shares, "compute_h_share_batch")
    if len(arr) == 0:
        return []
    return _h_batch(ctx or get_context(), qap, arr, deltas, None)


# ---- the witness from the inputs (code_to_qap.QAP.calculate_witness; csrc/bn256_r1cs_solve.hip) ----

KIND_CHECK, KIND_Y, KIND_A, KIND_B = 0, 1, 2, 3
_NO_WIRE = 0xFFFFFFFF


class SolvePlan:
    """How to compute every wire of a "program-shaped" R1CS from wire 0 (the constant 1) and the inputs, wires
    1 .. n_in: SolvePlan(qap, n_in), made once per (R1CSQAP, n_in) and kept on the QAP.  Pure host work on the constraint
    matrices alone - no device, no flat code.

    Rounds: a round visits the rows not yet placed in ascending row index.  A row whose support (V, W and Y together,
    duplicate entries added first, entries that are 0 mod the order ignored) has no unknown wire is a CHECK row of the
    round; a row with exactly one unknown wire s that no earlier row of the round defines DEFINES s; any other row waits.
    The wires a round defines are known after it.  A round is one LEVEL: the depth is minimal and the order
    deterministic.  The new wire must stand in exactly one of V, W, Y of its defining row, which gives the row's kind,
    with a, b, y the row's dot products over the known wires:
        KIND_Y   c_s = (a b - y) / gamma      every +, - and * row of the reference's flattener
        KIND_A   c_s = (y / b - a) / alpha    its `set` rows (b = wire 0, Y empty) and `/` rows (b the divisor)
        KIND_B   c_s = (y / a - b) / beta
    ValueError (1-based constraint numbers): a new wire in two of V, W, Y of its defining row; rows left with two or
    more unknown wires (the lowest is named); a wire that no row defines and that is no input (the lowest); n_in > m.

    level_ptr (n_levels + 1), and per row in level order: row (the original 0-based row), kind, wire (the new wire,
    0xffffffff for a check row), inv (ints: the inverse of the new wire's coefficient, 0 for a check row); csr: per
    matrix "V", "W", "Y" (row_ptr, col, vals as ints) in that order with the new wire's own entry removed."""

    def __new__(cls, qap, n_in):
        if not isinstance(qap, R1CSQAP):
            raise TypeError("SolvePlan needs the sparse R1CS, not interpolated polynomials: build the QAP as "
                            "R1CSQAP(V, W, Y, out_ix)")
        n_in = int(n_in)
        cache = qap.__dict__.setdefault("_solve_plans", {})
        if n_in not in cache:
            plan = object.__new__(cls)
            plan._build(qap, n_in)
            cache[n_in] = plan
        return cache[n_in]

    def _build(self, qap, n_in):
        m, d, n_wires = qap.m, qap.d, qap.m + 1
        if not 0 <= n_in <= m:
            raise ValueError(f"SolvePlan: n_in = {n_in} inputs, the QAP has m = {m} wires beside the constant")
        # rows[j] = [{wire: coefficient} for V, W, Y], duplicates added, zeros dropped
        raw = qap._vals.tobytes()
        rows = [[{}, {}, {}] for _ in range(d)]
        for e, (j, col) in enumerate(zip(qap._rows.tolist(), qap._cols.tolist())):
            mat = rows[j][col // n_wires]
            wire = col % n_wires
            mat[wire] = mat.get(wire, 0) + int.from_bytes(raw[32 * e:32 * e + 32], "little")
        users = [[] for _ in range(n_wires)]
        unknown = [0] * d
        for j, mats in enumerate(rows):
            for mat in mats:
                for wire in [w for w, x in mat.items() if x % ORDER == 0]:
                    del mat[wire]
                for wire in mat:
                    mat[wire] %= ORDER
            for wire in set().union(*mats):
                users[wire].append(j)
                unknown[j] += wire > n_in
        known = [i <= n_in for i in range(n_wires)]
        level_ptr, order, kinds, wires, invs = [0], [], [], [], []
        ready = [j for j in range(d) if unknown[j] <= 1]
        while ready:
            defined, waiting = {}, []
            for j in ready:                                   # ascending row index
                if unknown[j] == 0:
                    order.append(j), kinds.append(KIND_CHECK), wires.append(_NO_WIRE), invs.append(0)
                    continue
                s = next(w for w in set().union(*rows[j]) if not known[w])
                if s in defined:
                    waiting.append(j)                        # a check row of a later round
                    continue
                where = [k for k in range(3) if s in rows[j][k]]
                if len(where) != 1:
                    raise ValueError(f"SolvePlan: constraint {j + 1} is not linear in wire {s}, the wire it would define "
                                     f"(it stands in {' and '.join('VWY'[k] for k in where)})")
                defined[s] = j
                order.append(j), kinds.append((KIND_A, KIND_B, KIND_Y)[where[0]]), wires.append(s)
                invs.append(pow(rows[j][where[0]].pop(s), -1, ORDER))
            level_ptr.append(len(order))
            nxt = set(waiting)
            for s in defined:
                known[s] = True
            for s in defined:
                for j in users[s]:
                    if j != defined[s]:
                        unknown[j] -= 1
                        if unknown[j] <= 1:
                            nxt.add(j)
            for j in defined.values():
                unknown[j] = -1
            placed = set(order[level_ptr[-2]:])
            ready = sorted(j for j in nxt if j not in placed and unknown[j] >= 0)
        if len(order) < d:
            placed = set(order)
            j = min(j for j in range(d) if j not in placed)
            raise ValueError(f"SolvePlan: constraint {j + 1} keeps {unknown[j]} unknown wires: the R1CS is not "
                             f"program-shaped (every row must define at most one new wire)")
        if not all(known):
            raise ValueError(f"SolvePlan: no constraint defines wire {known.index(False)} and it is not an input")
        self.n_in, self.m, self.d = n_in, m, d
        self.n_levels = len(level_ptr) - 1
        self.level_ptr = np.asarray(level_ptr, np.uint32)
        self.row = np.asarray(order, np.uint32)
        self.kind = np.asarray(kinds, np.uint32)
        self.wire = np.asarray(wires, np.uint32)
        self.inv = invs
        self.csr = {}
        for k, name in enumerate("VWY"):
            ptr, col, vals = [0], [], []
            for j in order:
                for wire in sorted(rows[j][k]):
                    col.append(wire)
                    vals.append(rows[j][k][wire])
                ptr.append(len(col))
            self.csr[name] = (ptr, col, vals)

    def device(self, ctx):
        """the plan's arrays on `ctx`, uploaded once per context -> (13 device addresses as
        Context.bn256_r1cs_solve_batch takes them, the buffers that hold them)"""
        def make():
            bufs = []
            for name in "VWY":
                ptr, col, vals = self.csr[name]
                bufs += [ctx.upload(np.asarray(ptr, np.uint32)), ctx.upload(np.asarray(col + [0], np.uint32)),
                         ctx.upload(scalars_to_array(vals + [0]))]
            bufs += [ctx.upload(self.kind), ctx.upload(self.wire), ctx.upload(scalars_to_array(self.inv)),
                     ctx.upload(self.level_ptr)]
            ctx.sync()
            return [b.ptr for b in bufs], bufs
        cache = self.__dict__.setdefault("_device", {})
        if id(ctx) not in cache:
            cache[id(ctx)] = (ctx, make())
        return cache[id(ctx)][1]


class ShareSolvePlan:
    """SolvePlan's rows in the order of a solve on Shamir SHARES of the wires, where only a product of two shared
    values costs an exchange (trinocchio.calculate_witness_shares): ShareSolvePlan(qap, n_in), made
    once per (R1CSQAP, n_in) from SolvePlan(qap, n_in) and kept on the QAP.  Which row defines which wire, its kind, its
    inverse coefficient and its stored entries are SolvePlan's; only the order differs.  Pure host work.

    Wire 0 is public (every party's share of the constant 1 is 1), so a dot whose stored entries all sit on wire 0, or
    an empty dot, is a public constant.  A defining row is
        LINEAR    a KIND_Y row whose V entries or W entries are a subset of {wire 0}, or a KIND_A / KIND_B row whose
                  divisor side is: the row's own formula on a party's share vector gives its share of the new wire;
        PRODUCT   a KIND_Y row with a shared wire in both V and W: one multiplication of shares, one exchange.
    ValueError (1-based constraint numbers): a KIND_A / KIND_B row whose divisor has a shared wire ("division by a
    shared value": it needs an inversion protocol with two more exchanges and is out of scope); a constant divisor that
    is 0 mod the order.  SolvePlan's check rows are left out (n_checks counts them): trinocchio.prove tests every row
    through the masked residual.

    Depth mu: 0 for wire 0 and the inputs; a linear row gives its wire the largest mu among its stored entries (0 where
    it has none), a product row 1 + that.  n_rounds = the largest mu.  The solve runs the phases
    L_0, P_1, L_1, .., P_D, L_D: P_r the product rows of depth r in ascending row index, ONE exchange; L_r the linear
    rows of depth r in sub-levels (a row's sub-level is 1 + the largest sub-level of a linear wire of the same depth that
    it reads, 0 where it reads none), ascending row index within a sub-level; L_r may be empty.

    The arrays hold the linear rows first, phase by phase, then the product rows, round by round - so the local phases
    are sub-ranges of ONE level table, as vmpc_bn256_r1cs_solve_batch_dev takes them:
        local_level_ptr   (n_local_levels + 1) positions: sub-level k is rows local_level_ptr[k] .. local_level_ptr[k+1]-1
        phase_ptr         (n_rounds + 2): L_r is the sub-levels phase_ptr[r] .. phase_ptr[r+1]-1
        round_ptr         (n_rounds + 1): P_r is rows n_linear + round_ptr[r-1] .. n_linear + round_ptr[r]-1
        row, kind, wire, inv, csr   per row in that order, as SolvePlan's."""

    def __new__(cls, qap, n_in):
        base = SolvePlan(qap, n_in)                     # the TypeError for a reference QAP is SolvePlan's
        cache = qap.__dict__.setdefault("_share_solve_plans", {})
        if base.n_in not in cache:
            plan = object.__new__(cls)
            plan._build(base)
            cache[base.n_in] = plan
        return cache[base.n_in]

    def _build(self, base):
        rows = len(base.row)
        entries = []                                    # per SolvePlan position: the stored columns of V, W, Y
        for name in "VWY":
            ptr, col, _ = base.csr[name]
            entries.append([col[ptr[i]:ptr[i + 1]] for i in range(rows)])
        shared = lambda cols: any(w != 0 for w in cols)
        mu = {w: 0 for w in range(base.n_in + 1)}
        sub = {}                                        # linear-defined wire -> its sub-level
        linear, product = {}, {}                        # (mu, sub-level) / mu -> positions
        for i in range(rows):                           # level order: every entry read was defined before
            kind, j = int(base.kind[i]), int(base.row[i]) + 1
            if kind == KIND_CHECK:
                continue
            v, w, y = entries[0][i], entries[1][i], entries[2][i]
            read = v + w + y
            depth = max((mu[s] for s in read), default=0)
            if kind == KIND_Y:
                is_product = shared(v) and shared(w)
            else:
                is_product = False
                k = 1 if kind == KIND_A else 0
                if shared(entries[k][i]):
                    raise ValueError(f"ShareSolvePlan: division by a shared value in constraint {j} (the solve on shares "
                                     f"multiplies shared values but does not invert them)")
                if not entries[k][i]:                   # stored coefficients are non-zero residues: only an empty dot is 0
                    raise ValueError(f"ShareSolvePlan: division by the constant 0 in constraint {j}")
            s = int(base.wire[i])
            if is_product:
                mu[s] = depth + 1
                product.setdefault(depth + 1, []).append(i)
            else:
                mu[s] = depth
                sub[s] = max((sub[x] + 1 for x in read if mu[x] == depth and x in sub), default=0)
                linear.setdefault((depth, sub[s]), []).append(i)
        by_row = lambda pos: sorted(pos, key=lambda i: int(base.row[i]))
        self.n_rounds = D = max(product, default=0)
        order, local_level_ptr, phase_ptr = [], [0], [0]
        for r in range(D + 1):
            k = 0
            while (r, k) in linear:
                order += by_row(linear[r, k])
                local_level_ptr.append(len(order))
                k += 1
            phase_ptr.append(len(local_level_ptr) - 1)
        self.n_linear = len(order)
        round_ptr = [0]
        for r in range(1, D + 1):
            order += by_row(product[r])
            round_ptr.append(len(order) - self.n_linear)
        self.n_in, self.m, self.d = base.n_in, base.m, base.d
        self.n_checks = int((base.kind == KIND_CHECK).sum())
        self.local_level_ptr = np.asarray(local_level_ptr, np.uint32)
        self.phase_ptr = np.asarray(phase_ptr, np.uint32)
        self.round_ptr = np.asarray(round_ptr, np.uint32)
        self.n_local_levels = len(local_level_ptr) - 1
        idx = np.asarray(order, np.int64)
        self.row, self.kind, self.wire = base.row[idx], base.kind[idx], base.wire[idx]
        self.inv = [base.inv[i] for i in order]
        self.csr = {}
        for name in "VWY":
            bptr, bcol, bvals = base.csr[name]
            ptr, col, vals = [0], [], []
            for i in order:
                col += bcol[bptr[i]:bptr[i + 1]]
                vals += bvals[bptr[i]:bptr[i + 1]]
                ptr.append(len(col))
            self.csr[name] = (ptr, col, vals)

    def round_rows(self, r):
        """(r0, r1): the positions of P_r, r = 1 .. n_rounds"""
        return self.n_linear + int(self.round_ptr[r - 1]), self.n_linear + int(self.round_ptr[r])

    def device(self, ctx):
        """the plan's arrays on `ctx`, uploaded once per context -> (13 device addresses in SolvePlan.device's order, the
        last one local_level_ptr's; the buffers that hold them)"""
        def make():
            bufs = []
            for name in "VWY":
                ptr, col, vals = self.csr[name]
                bufs += [ctx.upload(np.asarray(ptr, np.uint32)), ctx.upload(np.asarray(col + [0], np.uint32)),
                         ctx.upload(scalars_to_array(vals + [0]))]
            bufs += [ctx.upload(np.append(self.kind, np.uint32(0))), ctx.upload(np.append(self.wire, np.uint32(0))),
                     ctx.upload(scalars_to_array(self.inv + [0])), ctx.upload(self.local_level_ptr)]
            ctx.sync()
            return [b.ptr for b in bufs], bufs
        cache = self.__dict__.setdefault("_device", {})
        if id(ctx) not in cache:
            cache[id(ctx)] = (ctx, make())
        return cache[id(ctx)][1]


def witness_batch_bytes(n_wires, n):
    """device bytes calculate_witness_batch holds for a chunk of n witnesses: the witnesses and one status word each"""
    return (32 * n_wires + 4) * n


def _input_rows(inputs):
    """K input vectors -> (K, n_in, 32) uint8 (any 32-byte values pass as they are; ints are reduced)"""
    if isinstance(inputs, np.ndarray) and inputs.ndim == 3:
        arr = np.ascontiguousarray(inputs, dtype=np.uint8)
        if arr.shape[2] != 32:
            raise ValueError(f"calculate_witness_batch: inputs of {arr.shape[2]} bytes, scalars have 32")
        return arr
    inputs = [list(x) for x in inputs]
    if len({len(x) for x in inputs}) > 1:
        raise ValueError("calculate_witness_batch: every witness takes the same number of inputs")
    n_in = len(inputs[0]) if inputs else 0
    return scalars_to_array([v for x in inputs for v in x]).reshape(len(inputs), n_in, 32)


def calculate_witness_batch(qap, inputs, ctx=None, wide_rows=0):
    """K witnesses of one R1CSQAP from K input vectors -> (K, n_wires, 32) uint8 canonical residues, row w = wire 0 (the
    constant 1), the inputs of witness w in wires 1 .. n_in, every other wire computed on the device: what compute_h_batch,
    compute_proof_batch, prove_batch and verify_batch take.  inputs: K sequences of n_in ints / field elements, or one
    (K, n_in, 32) uint8 array (uploaded as it is; values >= the order are reduced on the device).
    One upload, ONE solve for all K (SolvePlan's levels; narrow levels fused into single launches, wide_rows as in
    include/vmpc.h, 0 = the library's rule), one synchronisation, one read of the K status words, one download.  K is cut
    into chunks of at most BATCH_BUDGET_BYTES (plan_chunks, witness_batch_bytes) and VMPC_BN256_R1CS_MAX_WIT witnesses; a
    chunk boundary changes no value.  A division by zero or a violated check row raises ValueError naming the lowest
    bad witness (0-based) and, of its rows, the first that failed in solve order (1-based constraint)."""
    if not isinstance(qap, R1CSQAP):
        SolvePlan(qap, 0)                   # raises the TypeError that says what to pass
    arr = _input_rows(inputs)
    K, n_in = arr.shape[0], arr.shape[1]
    n_wires = qap.m + 1
    out = np.zeros((K, n_wires, 32), np.uint8)
    if K == 0:
        return out
    plan = SolvePlan(qap, n_in)
    ctx = ctx or get_context()
    ptrs, _ = plan.device(ctx)
    out[:, 1:n_in + 1] = arr
    for lo, hi in plan_chunks(K, BATCH_BUDGET_BYTES, lambda n: witness_batch_bytes(n_wires, n)):
        step = min(hi - lo, _native.BN256_R1CS_MAX_WIT)
        for a in range(lo, hi, step):
            b = min(a + step, hi)
            dc, bad = ctx.upload(out[a:b]), ctx.alloc(4 * (b - a))
            ctx.bn256_r1cs_solve_batch(ptrs, plan.level_ptr, n_in, qap.m, dc.ptr, n_wires, b - a, wide_rows, bad.ptr)
            ctx.sync()
            words = ctx.download(bad.ptr, 4 * (b - a)).view("<u4")
            viol = np.nonzero(words != 0xFFFFFFFF)[0]
            if len(viol):
                w, pos = a + int(viol[0]), int(words[viol[0]])
                j = int(plan.row[pos]) + 1
                if plan.kind[pos] == KIND_CHECK:
                    raise ValueError(f"calculate_witness_batch: witness {w} violates constraint {j} "
                                     f"(V(j) W(j) != Y(j) at j = {j})")
                raise ValueError(f"calculate_witness_batch: witness {w}: division by zero in constraint {j}")
            out[a:b] = ctx.download(dc.ptr, 32 * n_wires * (b - a)).reshape(b - a, n_wires, 32)
            del dc, bad
    return out


def calculate_witness(qap, inputs, ctx=None):
    """The reference's QAP.calculate_witness(inputs): the witness as a list of ints, c[0] == 1, the len(inputs) inputs
    in wires 1 .. len(inputs) - computed on the device from the R1CS (calculate_witness_batch with K = 1)."""
    raw = calculate_witness_batch(qap, [list(inputs)], ctx=ctx)[0].tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


def prove_batch_inputs(qap, inputs, key, deltas=None):
    """prove_batch from the inputs: calculate_witness_batch, then prove_batch on its witnesses -> (K proof dicts, the
    (K, n_wires, 32) witness array, of which verify / verify_batch read the io wires)."""
    ctx = key.ctx if isinstance(key, PreparedKey) else None
    cs = calculate_witness_batch(qap, inputs, ctx=ctx)
    return prove_batch(qap, cs, key, deltas), cs
