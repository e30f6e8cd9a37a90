"""The knowledge-of-exponent pivot of AC20 (section 9) over BN-256 on MI355X: constant-size openings of a linear form.

    trusted_setup                  verifiable_mpc/ac20/knowledge_of_exponent.py:50-72
    restriction_argument_prover    knowledge_of_exponent.py:75-95
    restriction_argument_verifier  knowledge_of_exponent.py:98-102
    opening_linear_form_prover     knowledge_of_exponent.py:105-133
    opening_linear_form_verifier   knowledge_of_exponent.py:136-153

Same names, arguments and return values as the reference.  The group work is the BN-256 layer of pynocchio.py
(csrc/bn256.hip MSMs over fixed-base tables, csrc/bn256_pairing.hip pairing products); the scalar work is
csrc/bn256_koe.hip over csrc/fr_bn.h: the powers g_exp z^(i+1) of the setup and the prover's one super-linear step,
the product of two degree-n polynomials over GF(order) (no NTT exists in that field: order - 1 = 2^5 * odd).

A `pp` is {"pp_lhs": ..., "pp_rhs": ...}.  trusted_setup returns the two sides as `PPVector`s: sequences of
BN256Point / BN256TwistPoint (len, indexing, iteration) whose points stay in HBM and whose MSM tables are built once,
at first use.  A plain dict of point lists - foreign (MPyC-style) points included - is accepted wherever a pp is taken.
Points are written additively here (the reference switches its groups to multiplicative notation): `g ** k` there is
`k * g` here.  The verifier evaluates both checks as "product of pairings == 1" in ONE pairing_product launch; points
not on their curve raise ValueError; G2 subgroup membership is not checked (as in pynocchio.verify).

x and L's coefficients may be device vectors (device.BnScalarVector): the prover's operands, the split of the product
and the verifier's reversed form are then made on the device (csrc/bn256_koe.hip), which is how Protocol 8 over a
SparseCircuit of this order opens its L (circuit_sat_gpu.py).  Lists take the host path.

`opening_linear_form_verifier_batch` (not in the reference) verifies K openings under one pp with the answers of K
single calls: the proofs' 5 K pairings in one pairing_product launch, their sums R as rows of PPVector.msm_rows
(vmpc_bn256_table_msm_rows_dev); DESIGN.md section 31.

`restriction_argument_prover_batch` and `opening_linear_form_prover_batch` (not in the reference) are the prover's side
of that: K commitments and K openings under one pp with the points and scalars of K single calls - one staged matrix,
one batched product, one split launch and one msm_rows per sum, whatever K is (csrc/bn256_koe.hip
vmpc_bn256_koe_stage_batch_dev / _split_batch_dev).

`update_setup` is one party's pass over a pp - every point times that party's own g_exp z^(i+1) - and what the joint
setup of mpc_koe.koe_trusted_setup is made of.

Not here: prove_nullity_koe (its challenge hashes repr() of an MPyC point).
"""
from random import SystemRandom

import numpy as np

from . import _native
from .device import BnScalarVector, get_context
from .pynocchio import (ORDER, BN256Point, BN256TwistPoint, _as_bytes, _neg_g1_rows, _pairing_product_arrays,
                        scalars_to_array)

prng = SystemRandom()

_CLS = {1: BN256Point, 2: BN256TwistPoint}
_CURVE = {1: "BN-256 curve", 2: "BN-256 twist"}


class PPVector:
    """One side of a pp on the device: n affine points (64 B in G1, 128 B on the twist).  Read like a list of points;
    the fixed-base table behind its MSMs is built at the first MSM and kept."""

    def __init__(self, ctx, group, buf, n, tabulate=True):
        self.ctx, self.group, self.buf, self.n = ctx, group, buf, n
        self.width = 64 * group
        self._tabulate, self._table, self._rows = tabulate, None, None

    @classmethod
    def from_points(cls, ctx, points, what, group):
        """upload a list of (possibly foreign) points, all of `group`, and check that they are on their curve; such a
        vector lives for one call, so its sums run without a table"""
        enc = [_as_bytes(p) for p in points]
        if any(g != group for g, _ in enc):
            raise ValueError(f"{what}: not a point of the {_CURVE[group]}")
        rows = np.frombuffer(b"".join(r for _, r in enc), np.uint8).reshape(-1, 64 * group)
        buf = ctx.upload(rows)
        if ctx.bn256_validate(group, buf.ptr, len(rows)):
            raise ValueError(f"{what}: point not on the {_CURVE[group]}")
        self = cls(ctx, group, buf, len(rows), tabulate=False)
        self._rows = rows
        return self

    def rows(self):
        """(n, width) uint8 host copy of the points (downloaded once)"""
        if self._rows is None:
            self.ctx.sync()
            self._rows = self.ctx.download(self.buf.ptr, self.width * self.n).reshape(self.n, self.width)
        return self._rows

    def __len__(self):
        return self.n

    def __getitem__(self, key):
        if isinstance(key, slice):
            return [self[i] for i in range(*key.indices(self.n))]
        i = key + self.n if key < 0 else key
        if not 0 <= i < self.n:
            raise IndexError(key)
        return _CLS[self.group].from_bytes(self.rows()[i].tobytes())

    def __iter__(self):
        return (self[i] for i in range(self.n))

    def msm(self, scalars):
        """sum_{i < m} scalars[i] * self[i] for an (m, 32) uint8 array or a device buffer of m scalars -> point"""
        ctx = self.ctx
        ds, m = scalars if isinstance(scalars, tuple) else (ctx.upload(scalars), len(scalars))
        assert 0 < m <= self.n
        out = ctx.alloc(self.width)
        if self._tabulate:
            if self._table is None:
                self._table = ctx.bn256_table_build(self.group, self.buf.ptr, self.n)
            ctx.bn256_table_msm(self.group, self._table.ptr, self.n, ds.ptr, m, out.ptr, None)
        else:
            ctx.bn256_msm(self.group, ds.ptr, self.buf.ptr, m, out.ptr)
        ctx.sync()
        return _CLS[self.group].from_bytes(ctx.download(out.ptr, self.width).tobytes())

    def msm_rows(self, matrix, m, rows, row_stride=None):
        """sum_{i < m} matrix[r][i] * self[i] for r < rows -> (rows, width) uint8 affine points (all zero: infinity).
        matrix: a device buffer of scalar rows, row_stride (default m) scalars apart.  One call of
        vmpc_bn256_table_msm_rows_dev over the vector's table and one synchronisation; an untabulated vector (from_points)
        runs its sums one by one."""
        ctx = self.ctx
        stride = m if row_stride is None else row_stride
        assert 0 < m <= self.n and stride >= m
        if rows == 0:
            return np.zeros((0, self.width), np.uint8)
        out = ctx.alloc(self.width * rows)
        if self._tabulate:
            if self._table is None:
                self._table = ctx.bn256_table_build(self.group, self.buf.ptr, self.n)
            ctx.bn256_table_msm_rows(self.group, self._table.ptr, self.n, matrix.ptr, stride, m, rows, out.ptr)
        else:
            for r in range(rows):
                ctx.bn256_msm(self.group, matrix.ptr + 32 * stride * r, self.buf.ptr, m, out.ptr + self.width * r)
        ctx.sync()
        return ctx.download(out.ptr, self.width * rows).reshape(rows, self.width)


def _side(ctx, pp, name, count=None):
    """pp[name] as a PPVector (its first `count` points when it arrives as a list)"""
    side = pp[name]
    if isinstance(side, PPVector):
        return side
    return PPVector.from_points(ctx, list(side[:count] if count is not None else side), name, 1 if name == "pp_lhs" else 2)


def _scalar_bytes(v):
    return np.frombuffer((int(v) % ORDER).to_bytes(32, "little"), np.uint8)


def fr_powers(z, scale, count, ctx=None):
    """device buffer of `count` scalars scale * z^(i+1) mod ORDER (csrc/bn256_koe.hip)"""
    ctx = ctx or get_context()
    dz, dscale, out = ctx.upload(_scalar_bytes(z)), ctx.upload(_scalar_bytes(scale)), ctx.alloc(max(32, 32 * count))
    ctx.bn256_fr_powers(dz.ptr, dscale.ptr, count, out.ptr)
    return out


def fr_poly_mul(a, b, ctx=None, method=None):
    """coefficients (lists of ints / field elements, or (len, 32) uint8 arrays of any 32-byte values) of two polynomials
    over GF(ORDER) -> (len(a) + len(b) - 1, 32) uint8 canonical coefficients of their product (csrc/bn256_koe.hip).
    method None: what the context's mode says (device.poly_product; schoolbook unless set); "ntt": the NTT over the
    integers (csrc/bn256_ntt.hip); "schoolbook": that kernel, whatever the mode.  Same bits."""
    if method not in (None, "ntt", "schoolbook"):
        raise ValueError(f"fr_poly_mul method {method!r}: None, 'ntt' or 'schoolbook'")
    ctx = ctx or get_context()
    a, b = scalars_to_array(a), scalars_to_array(b)
    da, db = ctx.upload(a), ctx.upload(b)
    out = ctx.alloc(32 * (len(a) + len(b) - 1))
    if method == "ntt":
        ctx.bn256_fr_poly_mul_ntt(da.ptr, len(a), db.ptr, len(b), out.ptr)
    elif method == "schoolbook":
        prev = ctx.get_poly_product()
        ctx.set_poly_product(_native.POLY_PRODUCT_SCHOOLBOOK)
        try:
            ctx.bn256_fr_poly_mul(da.ptr, len(a), db.ptr, len(b), out.ptr)
        finally:
            ctx.set_poly_product(prev)
    else:
        ctx.bn256_fr_poly_mul(da.ptr, len(a), db.ptr, len(b), out.ptr)
    ctx.sync()
    return ctx.download(out.ptr, 32 * (len(a) + len(b) - 1)).reshape(-1, 32)


def trusted_setup(_g1, _g2, n, order, progress_bar=False):
    """pp_lhs[i] = (g_exp z^(i+1)) * _g1 and pp_rhs[i] = (g_exp alpha z^(i+1)) * _g2 for i < 2n, with g_exp, alpha, z
    drawn from this module's `prng` in the reference's order (knowledge_of_exponent.py:50-72).  The 2n exponents are
    one launch (fr_powers), the points one fixed-base launch per group.  `progress_bar` is accepted and ignored."""
    if int(order) != ORDER:
        raise ValueError("trusted_setup: order is not the BN-256 group order")
    g_exp = prng.randrange(1, order)
    alpha = prng.randrange(order)
    z = prng.randrange(order)
    return setup_under(_g1, _g2, n, g_exp, alpha, z)


def setup_under(_g1, _g2, n, g_exp, alpha, z):
    """trusted_setup's pp under a GIVEN trapdoor (g_exp, alpha, z): the first party's contribution to a jointly made pp
    (mpc_koe.koe_trusted_setup), which the later parties' update_setup passes then multiply into"""
    ctx = get_context()
    pp = {}
    for name, group, base, scale in (("pp_lhs", 1, _g1, g_exp), ("pp_rhs", 2, _g2, g_exp * alpha % ORDER)):
        grp, raw = _as_bytes(base)
        if grp != group:
            raise ValueError(f"trusted_setup: generator {group} is not a point of the {_CURVE[group]}")
        dbase = ctx.upload(np.frombuffer(raw, np.uint8))
        if ctx.bn256_validate(group, dbase.ptr, 1):
            raise ValueError(f"trusted_setup: generator {group} is not on the {_CURVE[group]}")
        exps = fr_powers(z, scale, 2 * n, ctx)
        pts = ctx.alloc(max(1, 64 * group * 2 * n))
        ctx.bn256_fixed_base(group, dbase.ptr, exps.ptr, 2 * n, pts.ptr)
        ctx.sync()
        pp[name] = PPVector(ctx, group, pts, 2 * n)
    return pp


def update_setup(pp, g_exp, alpha, z):
    """One party's pass over a pp: a new pp with
        lhs'[i] = (g_exp z^(i+1)) * lhs[i]          rhs'[i] = (g_exp alpha z^(i+1)) * rhs[i]
    so that update_setup(trusted_setup under (a, b, c), a', b', c') IS trusted_setup under (a a', b b', c c'), byte for
    byte - the trapdoors multiply, and a pp that went through M parties has a trapdoor nobody knows unless all M
    collude.  The exponents are one fr_powers launch per side, the points one vmpc_bn256_scale_points_dev launch
    (csrc/bn256_scale.hip: every point with a scalar of its own).  The sides may be PPVectors or lists of points; lists
    are uploaded and validated (a point off its curve: ValueError naming the side).  A factor that is 0 mod the order
    would send the whole pp to infinity: ValueError."""
    factors = {"g_exp": int(g_exp) % ORDER, "alpha": int(alpha) % ORDER, "z": int(z) % ORDER}
    for name, v in factors.items():
        if v == 0:
            raise ValueError(f"update_setup: {name} is 0 mod the group order")
    ctx = get_context()
    out = {}
    for name, group, scale in (("pp_lhs", 1, factors["g_exp"]),
                               ("pp_rhs", 2, factors["g_exp"] * factors["alpha"] % ORDER)):
        side = _side(ctx, pp, name)
        n = len(side)
        exps = fr_powers(factors["z"], scale, n, ctx)
        pts = ctx.alloc(max(1, side.width * n))
        ctx.bn256_scale_points(group, side.buf.ptr, exps.ptr, n, pts.ptr)
        ctx.sync()
        out[name] = PPVector(ctx, group, pts, n)
    return out


def _restriction_scalars(S, x, gamma):
    """(max(S) + 2, 32) scalars: gamma, then x[i] at position i + 1 for i in S and 0 elsewhere"""
    if isinstance(S, range) and S.step == 1 and S.start == 0:
        return scalars_to_array([gamma] + [x[i] for i in S])
    S = list(S)
    sc = [0] * (max(S) + 2 if S else 1)
    sc[0] = gamma
    for i in S:
        sc[i + 1] = x[i]
    return scalars_to_array(sc)


def _on_device(v):
    """is v a device vector of scalars of this order (device.BnScalarVector)?"""
    return isinstance(v, BnScalarVector)


def _staged(ctx, x, gamma, L_coeffs):
    """(lhs, rhs) device buffers: lhs = (gamma, x_0, .., x_{n-1}) from a device x (None: no lhs), rhs = (L_{n-1}, ..,
    L_0) from device coefficients (None: no rhs) - csrc/bn256_koe.hip, nothing passes through the host"""
    n = len(x) if x is not None else len(L_coeffs)
    lhs = ctx.alloc(32 * (n + 1)) if x is not None else None
    rhs = ctx.alloc(max(32, 32 * n)) if L_coeffs is not None else None
    ptr = lambda v: v.ptr if v is not None else None      # noqa: E731
    ctx.bn256_koe_stage(ptr(x), int(gamma) % ORDER if x is not None else None, ptr(L_coeffs), n, ptr(lhs), ptr(rhs))
    return lhs, rhs


def restriction_argument_prover(S, x, gamma, pp):
    """(P, pi): the commitment gamma pp_lhs[0] + sum_{i in S} x[i] pp_lhs[i+1] to the S-indices of x and the same sum
    over pp_rhs (knowledge_of_exponent.py:75-95).  One G1 MSM and one G2 MSM.  x may be a device BnScalarVector when S
    is all of it: the scalars (gamma, x) are then put together on the device."""
    ctx = get_context()
    if _on_device(x):
        if not (isinstance(S, range) and S == range(len(x))):
            raise ValueError("restriction_argument_prover: a device vector x is committed to as a whole, S = range(len(x))")
        ds = (_staged(ctx, x, gamma, None)[0], len(x) + 1)
    else:
        sc = _restriction_scalars(S, x, gamma)
        ds = (ctx.upload(sc), len(sc))
    return _side(ctx, pp, "pp_lhs", ds[1]).msm(ds), _side(ctx, pp, "pp_rhs", ds[1]).msm(ds)


def _proof_point(ctx, pt, group, name):
    grp, raw = _as_bytes(pt)
    row = np.frombuffer(raw, np.uint8)
    if grp != group or ctx.bn256_validate(group, ctx.upload(row).ptr, 1):
        raise ValueError(f"{name} is not on the {_CURVE[group]}")
    return row


def restriction_argument_verifier(P, pi, pp):
    """e(P, pp_rhs[0]) == e(pp_lhs[0], pi) (knowledge_of_exponent.py:98-102), as e(P, g2) e(-g1, pi) == 1"""
    ctx = get_context()
    g1, g2 = _side(ctx, pp, "pp_lhs", 1).rows()[0], _side(ctx, pp, "pp_rhs", 1).rows()[0]
    rP, rpi = _proof_point(ctx, P, 1, "P"), _proof_point(ctx, pi, 2, "pi")
    _, ones = _pairing_product_arrays(ctx, np.stack([rP, _neg_g1_rows(g1[None])[0]]), np.stack([g2, rpi]), [0, 2],
                                      validate=False)
    return ones[0]


def _form_parts(L):
    """(coefficients as a list, constant) of a LinearForm / AffineForm, this package's or the reference's"""
    coeffs = L.coeffs.to_ints() if hasattr(L.coeffs, "to_ints") else L.coeffs
    return coeffs, getattr(L, "constant", 0)


def _reversed_coeffs(coeffs, n):
    """[coeffs[n - (j + 1)] for j < n] as (n, 32) scalars: the linear form as the polynomial it is multiplied in as"""
    return np.ascontiguousarray(scalars_to_array(coeffs[:n])[::-1])


def _like(sample, value):
    """`value` (an int mod ORDER) in the field type of `sample` when that is a field element of this order"""
    cls = type(sample)
    if hasattr(sample, "value") and getattr(cls, "modulus", None) == ORDER:
        return cls(value)
    return value


def opening_linear_form_prover(L, x, gamma, pp, P=None, pi=None):
    """(proof, u): proof = {"P", "pi", "Q"} opens L on the committed x to u = L(x) (knowledge_of_exponent.py:105-133).
    c = (gamma, x_0, ..., x_{n-1}) * (L_{n-1}, ..., L_0) is one launch of the polynomial-product kernel; its
    coefficient n is u minus L's constant, and Q = -sum_{i != n} c[i] pp_lhs[i] is one G1 MSM.  u comes back as a field
    element when L's coefficients (or its constant) are field elements of this order, else as an int below ORDER."""
    ctx = get_context()
    proof = {}
    n = len(x)
    S = range(n)
    n_lhs = len(pp["pp_lhs"])
    assert 2 * n - 1 <= n_lhs, "Requirement does not hold: 2*len(x)-1 <= number of generators in first group."
    if P is None:
        P, pi = restriction_argument_prover(S, x, gamma, pp)
    proof["P"] = P
    proof["pi"] = pi

    on_device = _on_device(x) and _on_device(L.coeffs)
    if on_device:
        # z and L never pass through the host: the operands are put together, the product split and Q's scalars
        # left where the MSM reads them (csrc/bn256_koe.hip); only u's 32 bytes come back, after the MSM has synchronised
        coeffs, constant = L.coeffs, getattr(L, "constant", 0)
        assert len(coeffs) == n, "Length of inputs to be equal to coefficients of linear form."
        (d_lhs, d_rhs), c_bar, d_u = _staged(ctx, x, gamma, coeffs), ctx.alloc(32 * 2 * n), ctx.alloc(32)
        ctx.bn256_fr_poly_mul(d_lhs.ptr, n + 1, d_rhs.ptr, n, c_bar.ptr)
        ctx.bn256_koe_split(c_bar.ptr, n, d_u.ptr)
    else:
        if _on_device(x):
            x = x.to_ints()
        coeffs, constant = _form_parts(L)
        assert len(coeffs) == n, "Length of inputs to be equal to coefficients of linear form."
        lhs = scalars_to_array([gamma] + list(x))
        rhs = _reversed_coeffs(coeffs, n)
        d_lhs, d_rhs, c_bar = ctx.upload(lhs), ctx.upload(rhs), ctx.alloc(32 * 2 * n)
        ctx.bn256_fr_poly_mul(d_lhs.ptr, n + 1, d_rhs.ptr, n, c_bar.ptr)
        ctx.sync()
        u_linear = int.from_bytes(ctx.download(c_bar.ptr + 32 * n, 32).tobytes(), "little")
        ctx.upload_into(c_bar.ptr + 32 * n, np.zeros(32, np.uint8))
    assert n_lhs == 2 * n
    Q = _side(ctx, pp, "pp_lhs").msm((c_bar, 2 * n))
    if Q.coords is not None:
        Q = BN256Point((Q.coords[0], -Q.coords[1]))
    proof["Q"] = Q
    if on_device:
        u_linear = int.from_bytes(ctx.download(d_u.ptr, 32).tobytes(), "little")
        sample = constant
    else:
        sample = constant if hasattr(constant, "value") else (coeffs[0] if n else 0)
    u = _like(sample, (u_linear + int(constant)) % ORDER)
    return proof, u


# ---- K openings under one pp ---------------------------------------------------------------------
# device bytes one chunk of opening_linear_form_prover_batch / restriction_argument_prover_batch may hold in its operand
# matrices (lhs, L, rhs, c) and the product's arena: K is cut into chunks of that many (circuit_sat_gpu.BATCH_BUDGET_BYTES
# is the same rule one layer up)
PROVE_BATCH_BUDGET_BYTES = 1 << 30
MAX_BATCH = 65535           # VMPC_BN256_QAP_MAX_WIT of include/vmpc.h


class StagedRows:
    """K rows lhs_p = (gamma_p, x_p[0..n-1]) of one device buffer, `stride` scalars apart: what the restriction argument
    sums over pp_lhs and pp_rhs and the opening multiplies by the reversed form.  Made once (stage_lhs_batch) and
    handed from the commitment to the opening."""

    def __init__(self, buf, stride, n, K, ptr=None):
        self.buf, self.ptr, self.stride, self.n, self.K = buf, buf.ptr if ptr is None else ptr, stride, n, K

    def rows(self, lo, hi):
        """rows lo..hi-1 as a StagedRows of the same buffer"""
        assert 0 <= lo <= hi <= self.K
        return StagedRows(self.buf, self.stride, self.n, hi - lo, self.ptr + 32 * self.stride * lo)


def _input_rows(xs, K, stride, n):
    """(xs, stride, n) of K rows: a device BnScalarVector (rows `stride` scalars apart, default len / K, the first n of
    each - default all - being x_p) or K host lists of one length"""
    if _on_device(xs):
        if stride is None:
            if len(xs) % K:
                raise ValueError(f"xs holds {len(xs)} scalars, not a multiple of the {K} rows")
            stride = len(xs) // K
        n = stride if n is None else n
        if n > stride or len(xs) < (K - 1) * stride + n:
            raise ValueError(f"xs: {K} rows of {n} scalars, {stride} apart, do not fit {len(xs)} scalars")
        return xs, stride, n
    xs = [x.to_ints() if _on_device(x) else list(x) for x in xs]
    if len(xs) != K or any(len(x) != len(xs[0]) for x in xs):
        raise ValueError(f"xs: {K} vectors of one length expected")
    return xs, len(xs[0]), len(xs[0])


def stage_lhs_batch(xs, gammas, stride=None, n=None, ctx=None):
    """StagedRows of K = len(gammas) rows (gamma_p, x_p).  xs on the device (a BnScalarVector of K rows, `stride` scalars
    apart, n of each read): the gammas are one upload and the rows one launch (vmpc_bn256_koe_stage_batch_dev); K host
    lists: the matrix is put together on the host and is one upload."""
    ctx = ctx or get_context()
    gammas = list(gammas)
    K = len(gammas)
    xs, stride, n = _input_rows(xs, K, stride, n)
    if _on_device(xs):
        buf = ctx.alloc(32 * (n + 1) * K)
        dg = ctx.upload(scalars_to_array(gammas))
        ctx.bn256_koe_stage_batch(xs.ptr, stride, dg.ptr, None, n, n, K, buf.ptr, n + 1, None, n)
    else:
        buf = ctx.upload(np.concatenate([scalars_to_array([g] + x) for g, x in zip(gammas, xs)]))
    return StagedRows(buf, n + 1, n, K)


def _points_of_rows(rows, group):
    return [_CLS[group].from_bytes(r.tobytes()) for r in rows]


def restriction_argument_prover_batch(xs, gammas, pp, stride=None, n=None, lhs=None, return_lhs=False):
    """[restriction_argument_prover(range(n), x_p, gamma_p, pp) for p < K] -> [(P_p, pi_p)], the same points, for K
    vectors of one length under one pp: ONE staged matrix lhs of K rows (gamma_p, x_p), one PPVector.msm_rows over
    pp_lhs and one over pp_rhs (m = n + 1 each), two synchronisations whatever K is.

    xs: a device BnScalarVector of K rows of n scalars, `stride` (default n) scalars apart, or K host lists (one upload).
    lhs: the rows already staged (stage_lhs_batch), xs is then not read.  return_lhs: (pairs, lhs) instead, so that
    opening_linear_form_prover_batch does not stage the rows again; the matrix is then ONE buffer of K (n + 1) scalars.
    Otherwise K is cut into chunks of PROVE_BATCH_BUDGET_BYTES of lhs."""
    ctx = get_context()
    gammas = list(gammas)
    K = len(gammas)
    if K == 0:
        return ([], None) if return_lhs else []
    if lhs is None and not return_lhs:
        xs, stride, n = _input_rows(xs, K, stride, n)
        step = max(1, min(K, MAX_BATCH, PROVE_BATCH_BUDGET_BYTES // (32 * (n + 1))))
        if step < K:
            pairs = []
            for lo in range(0, K, step):
                hi = min(K, lo + step)
                part = xs[lo * stride:(hi - 1) * stride + n] if _on_device(xs) else xs[lo:hi]
                pairs += restriction_argument_prover_batch(part, gammas[lo:hi], pp, stride, n,
                                                           lhs=stage_lhs_batch(part, gammas[lo:hi], stride, n, ctx))
            return pairs
    if lhs is None:
        lhs = stage_lhs_batch(xs, gammas, stride, n, ctx)
    assert lhs.K == K
    m = lhs.n + 1
    g1, g2 = _side(ctx, pp, "pp_lhs", m), _side(ctx, pp, "pp_rhs", m)
    pairs = list(zip(_points_of_rows(g1.msm_rows(lhs, m, K, lhs.stride), 1),
                     _points_of_rows(g2.msm_rows(lhs, m, K, lhs.stride), 2)))
    return (pairs, lhs) if return_lhs else pairs


def _product_arena_bytes(ctx, n, k):
    """the arena bytes the batched product of k openings of length n reserves on ctx, by the route its mode selects"""
    mode = ctx.get_poly_product()
    if mode == _native.POLY_PRODUCT_NTT or (mode == _native.POLY_PRODUCT_AUTO and n >= _native.BN256_FR_NTT_MIN):
        return _native.bn256_fr_poly_mul_ntt_batch_bytes(n + 1, n, 0, 2 * n, k)
    return _native.bn256_fr_poly_mul_batch_bytes(n + 1, n, 0, 2 * n, k)


def prove_batch_bytes(n, k, ctx=None):
    """device bytes of k openings of length n inside opening_linear_form_prover_batch: lhs (n + 1), the gathered L (n),
    rhs (n) and c (2n) scalars per opening, u, and the product's arena"""
    return 32 * k * ((n + 1) + n + n + 2 * n + 1) + _product_arena_bytes(ctx or get_context(), n, k)


def prove_chunk_size(n, K, ctx=None):
    """the most openings (<= K) whose prove_batch_bytes stay within PROVE_BATCH_BUDGET_BYTES, at least one"""
    ctx = ctx or get_context()
    lo, hi = 1, min(K, MAX_BATCH)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if prove_batch_bytes(n, mid, ctx) <= PROVE_BATCH_BUDGET_BYTES:
            lo = mid
        else:
            hi = mid - 1
    return lo


def opening_linear_form_prover_batch(Ls, xs, gammas, pp, Ps=None, pis=None, stride=None, n=None, lhs=None):
    """[opening_linear_form_prover(L_p, x_p, gamma_p, pp, P_p, pi_p) for p < K] -> [(proof_p, u_p)] with the same points
    and the same u (value and type), for K forms of one length n under one pp, every stage once per chunk of openings:

        one vmpc_bn256_koe_stage_batch_dev     the rows (gamma_p, x_p) - unless `lhs` brings them, or the restriction
                                               argument (Ps None) has just made them - and the rows L_p reversed
        one ctx.bn256_fr_poly_mul_batch        c_p = lhs_p * rhs_p, b_stride = n, the whole window [0, 2n): schoolbook
                                               or NTT by the context's poly_product mode, as in the single call
        one vmpc_bn256_koe_split_batch_dev     u_p = c_p[n], c_p[n] = 0
        one PPVector.msm_rows over pp_lhs      Q_p = -sum_i c_p[i] pp_lhs[i], m = 2n, negated on the host; an all-zero
                                               row is the point at infinity, returned as the single call returns it
        one download of the K scalars u

    xs, stride, n, lhs: as in restriction_argument_prover_batch (host lists: the rows are one upload).  The forms'
    coefficients may be device BnScalarVectors (gathered into one matrix by device copies, nothing passes through the
    host) or lists (one upload).  K is cut into chunks of at most PROVE_BATCH_BUDGET_BYTES (prove_batch_bytes); the product's arena is
    reserved by the entry itself."""
    ctx = get_context()
    Ls, gammas = list(Ls), list(gammas)
    K = len(Ls)
    if len(gammas) != K or (Ps is not None and (len(Ps) != K or pis is None or len(pis) != K)):
        raise ValueError("opening_linear_form_prover_batch: Ls, gammas, Ps and pis differ in length")
    if K == 0:
        return []
    if lhs is None:
        xs, stride, n = _input_rows(xs, K, stride, n)
    else:
        assert lhs.K == K
        n = lhs.n
    n_lhs = len(pp["pp_lhs"])
    assert 2 * n - 1 <= n_lhs, "Requirement does not hold: 2*len(x)-1 <= number of generators in first group."
    for L in Ls:
        assert len(L.coeffs) == n, "Length of inputs to be equal to coefficients of linear form."
    assert n_lhs == 2 * n
    side = _side(ctx, pp, "pp_lhs")
    step = prove_chunk_size(n, K, ctx)
    out = []
    for lo in range(0, K, step):
        hi = min(K, lo + step)
        k = hi - lo
        forms = Ls[lo:hi]
        on_device = all(_on_device(L.coeffs) for L in forms)
        if on_device:
            d_L = ctx.alloc(32 * n * k)
            for j, L in enumerate(forms):
                ctx.copy(d_L.ptr + 32 * n * j, L.coeffs.ptr, 32 * n)
            host_coeffs = None
        else:
            host_coeffs = [_form_parts(L)[0] for L in forms]
            d_L = ctx.upload(np.concatenate([scalars_to_array(co[:n]) for co in host_coeffs]))
        rhs, c_bar, d_u = ctx.alloc(32 * n * k), ctx.alloc(32 * 2 * n * k), ctx.alloc(32 * k)
        if lhs is None and _on_device(xs):
            # the one launch makes both operands
            rows = StagedRows(ctx.alloc(32 * (n + 1) * k), n + 1, n, k)
            dg = ctx.upload(scalars_to_array(gammas[lo:hi]))
            ctx.bn256_koe_stage_batch(xs.ptr + 32 * stride * lo, stride, dg.ptr, d_L.ptr, n, n, k, rows.ptr, n + 1, rhs.ptr,
                                      n)
        else:
            rows = lhs.rows(lo, hi) if lhs is not None else stage_lhs_batch(xs[lo:hi], gammas[lo:hi], ctx=ctx)
            ctx.bn256_koe_stage_batch(None, n, None, d_L.ptr, n, n, k, None, n + 1, rhs.ptr, n)
        if Ps is None:
            pairs = restriction_argument_prover_batch(None, gammas[lo:hi], pp, lhs=rows)
        else:
            pairs = list(zip(Ps[lo:hi], pis[lo:hi]))
        ctx.bn256_fr_poly_mul_batch(rows.ptr, rows.stride, n + 1, rhs.ptr, n, n, 0, 2 * n, c_bar.ptr, 2 * n, k)
        ctx.bn256_koe_split_batch(c_bar.ptr, 2 * n, n, k, d_u.ptr)
        Q_rows = side.msm_rows(c_bar, 2 * n, k, row_stride=2 * n)        # synchronises
        us = ctx.download(d_u.ptr, 32 * k).reshape(k, 32)
        for j, (L, (P, pi)) in enumerate(zip(forms, pairs)):
            Q = BN256Point.from_bytes(Q_rows[j].tobytes())
            if Q.coords is not None:
                Q = BN256Point((Q.coords[0], -Q.coords[1]))
            # u's type is the single call's: the constant's when that is a field element (or the coefficients live on
            # the device), else that of the first coefficient
            constant = getattr(L, "constant", 0)
            if hasattr(constant, "value") or _on_device(L.coeffs):
                sample = constant
            else:
                sample = host_coeffs[j][0] if n else 0
            u = _like(sample, (int.from_bytes(us[j].tobytes(), "little") + int(constant)) % ORDER)
            out.append(({"P": P, "pi": pi, "Q": Q}, u))
    return out


def opening_linear_form_verifier(L, pp, proof, u):
    """{"restriction_arg_check", "PRQ_check"} -> bool (knowledge_of_exponent.py:136-153).  R = sum_j L[n-1-j] pp_rhs[j]
    is one G2 MSM; then both checks in one pairing_product launch, five Miller loops and two final exponentiations:
        e(P, g2) e(-g1, pi) == 1      and      e(P, R) e(Q, g2) e(-g1, u pp_rhs[n]) == 1"""
    ctx = get_context()
    on_device = _on_device(L.coeffs)
    coeffs, constant = (L.coeffs, getattr(L, "constant", 0)) if on_device else _form_parts(L)
    n = len(coeffs)
    lhs, rhs = _side(ctx, pp, "pp_lhs", 1), _side(ctx, pp, "pp_rhs", n + 1)
    if len(rhs) <= n:
        raise ValueError("pp_rhs holds fewer than len(L) + 1 points")
    u_linear = (int(u) - int(constant)) % ORDER
    rP, rpi, rQ = (_proof_point(ctx, proof[k], g, k) for k, g in (("P", 1), ("pi", 2), ("Q", 1)))
    # R's scalars: L's coefficients reversed - on the device when that is where they are
    r_scalars = (_staged(ctx, None, None, coeffs)[1], n) if on_device else _reversed_coeffs(coeffs, n)
    R = np.frombuffer(rhs.msm(r_scalars).to_bytes(), np.uint8)
    # u * pp_rhs[n]: the one-base case of the verifier's small linear combinations (csrc/bn256_pairing.hip)
    uT = ctx.alloc(128)
    ctx.bn256_lincomb_batch(2, rhs.buf.ptr + 128 * n, 1, ctx.upload(_scalar_bytes(u_linear)).ptr, None, 0, 1, False,
                            uT.ptr)
    ctx.sync()
    uT = ctx.download(uT.ptr, 128)
    g2 = rhs.rows()[0]
    neg_g1 = _neg_g1_rows(lhs.rows()[:1])[0]
    _, ones = _pairing_product_arrays(ctx, np.stack([rP, neg_g1, rP, rQ, neg_g1]), np.stack([g2, rpi, R, g2, uT]),
                                      [0, 2, 5], validate=False)
    return {"restriction_arg_check": ones[0], "PRQ_check": ones[1]}


# bytes of reversed linear forms (32 N each) that opening_linear_form_verifier_batch holds on the device at a time: the
# proofs' sums R go through msm_rows in chunks of this many bytes' worth of rows (circuit_sat_gpu.BATCH_BUDGET_BYTES)
BATCH_ROWS_BUDGET_BYTES = 1 << 28


def _batch_proof_points(ctx, proofs, name, group):
    """(K, width) uint8 rows of proofs[i][name], uploaded and validated in one call each; a point off its curve is then
    found proof by proof: ValueError with the single verifier's message, prefixed with the proof's index"""
    enc = [_as_bytes(proof[name]) for proof in proofs]
    for i, (grp, _) in enumerate(enc):
        if grp != group:
            raise ValueError(f"proof {i}: {name} is not on the {_CURVE[group]}")
    rows = np.frombuffer(b"".join(raw for _, raw in enc), np.uint8).reshape(len(proofs), 64 * group)
    if ctx.bn256_validate(group, ctx.upload(rows).ptr, len(rows)):
        for i, proof in enumerate(proofs):
            try:
                _proof_point(ctx, proof[name], group, name)
            except ValueError as e:
                raise ValueError(f"proof {i}: {e}") from None
    return rows


def opening_linear_form_verifier_batch(Ls, pp, proofs, us):
    """[opening_linear_form_verifier(L, pp, proof, u) for L, proof, u in zip(Ls, proofs, us)] - the same dicts with the
    same booleans - for K openings under one pp, all forms of one length N.  The K proofs are 5 K
    pairs and 2 K products of ONE pairing_product launch (a lane runs a whole Miller loop or final exponentiation, so
    the launch lasts as long as for one proof); the sums R_p = sum_j L_p[N-1-j] pp_rhs[j] are rows of msm_rows, the
    points u_p pp_rhs[N] one lincomb launch.  No random weights: every proof keeps its own two checks.  Forms of
    different lengths: ValueError; a point off its curve: ValueError naming the proof and the point."""
    Ls, proofs, us = list(Ls), list(proofs), list(us)
    K = len(Ls)
    if len(proofs) != K or len(us) != K:
        raise ValueError("opening_linear_form_verifier_batch: Ls, proofs and us differ in length")
    if K == 0:
        return []
    ctx = get_context()
    forms = [(L.coeffs, getattr(L, "constant", 0)) if _on_device(L.coeffs) else _form_parts(L) for L in Ls]
    n = len(forms[0][0])
    if any(len(coeffs) != n for coeffs, _ in forms):
        raise ValueError("opening_linear_form_verifier_batch: the linear forms differ in length")
    lhs, rhs = _side(ctx, pp, "pp_lhs", 1), _side(ctx, pp, "pp_rhs", n + 1)
    if len(rhs) <= n:
        raise ValueError("pp_rhs holds fewer than len(L) + 1 points")
    rP, rpi, rQ = (_batch_proof_points(ctx, proofs, k, g) for k, g in (("P", 1), ("pi", 2), ("Q", 1)))
    # R's scalars: every L reversed, one row of a (G, n) device matrix per proof; G under the byte budget
    R = np.empty((K, 128), np.uint8)
    G = max(1, min(K, BATCH_ROWS_BUDGET_BYTES // (32 * n)))
    matrix = ctx.alloc(32 * n * G)
    for k0 in range(0, K, G):
        chunk = forms[k0:k0 + G]
        for j, (coeffs, _) in enumerate(chunk):
            row = matrix.ptr + 32 * n * j
            if _on_device(coeffs):
                ctx.bn256_koe_stage(None, None, coeffs.ptr, n, None, row)
            else:
                ctx.upload_into(row, _reversed_coeffs(coeffs, n))
        R[k0:k0 + len(chunk)] = rhs.msm_rows(matrix, n, len(chunk))
    # u_p * pp_rhs[n] for every proof: one launch, one base
    u_linear = scalars_to_array([(int(u) - int(constant)) % ORDER for u, (_, constant) in zip(us, forms)])
    uT = ctx.alloc(128 * K)
    ctx.bn256_lincomb_batch(2, rhs.buf.ptr + 128 * n, 1, ctx.upload(u_linear).ptr, None, 0, K, False, uT.ptr)
    ctx.sync()
    uT = ctx.download(uT.ptr, 128 * K).reshape(K, 128)
    g2 = np.broadcast_to(rhs.rows()[0], (K, 128))
    neg_g1 = np.broadcast_to(_neg_g1_rows(lhs.rows()[:1])[0], (K, 64))
    # per proof: e(P, g2) e(-g1, pi)  and  e(P, R) e(Q, g2) e(-g1, u pp_rhs[n])
    g1_rows = np.stack([rP, neg_g1, rP, rQ, neg_g1], axis=1).reshape(5 * K, 64)
    g2_rows = np.stack([g2, rpi, R, g2, uT], axis=1).reshape(5 * K, 128)
    offsets = np.sort(np.concatenate([5 * np.arange(K + 1), 5 * np.arange(K) + 2]))
    _, ones = _pairing_product_arrays(ctx, g1_rows, g2_rows, offsets, validate=False)
    return [{"restriction_arg_check": ones[2 * i], "PRQ_check": ones[2 * i + 1]} for i in range(K)]
