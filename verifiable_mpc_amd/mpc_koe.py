"""The knowledge-of-exponent pivot of AC20 over a SECRET-SHARED vector, and a pp that the parties make together
(verifiable_mpc/ac20/mpc_ac20.py:54-138).  One party's side, on its GPU.

    koe_trusted_setup                     mpc_ac20.py:54-84
    koe_restriction_argument_prover       mpc_ac20.py:87-109
    koe_opening_linear_form_prover        mpc_ac20.py:112-138

Shares are Shamir shares mod n, the BN-256 group order: `Runtime` is trinocchio.Runtime (the hub, the deal round, the
opening, the exchange and the recombination of points in the exponent) with the one operation a Pinocchio proof never
needed, the product of two shared vectors, over csrc/mpc_share.hip's GF(n) entries.  `SharedVector` is a party's shares
of a vector as ONE device vector (device.BnScalarVector); mpc_ac20.SecureVector is GF(l) throughout and stays so.

The pp.  Whoever ran knowledge_of_exponent.trusted_setup knows (g_exp, alpha, z) and can open any commitment under that pp
to anything, so an M-party prover over such a pp convinces nobody who did not run the setup himself.
koe_trusted_setup is a powers-of-tau pass instead: party 0 makes a pp under its own draws, every later party in turn
multiplies element i of both sides by ITS g_p z_p^(i+1) (and alpha_p on the twist) - knowledge_of_exponent.update_setup,
one vmpc_bn256_scale_points_dev launch per side - and passes it on.  The result is trusted_setup's pp under the PRODUCT
trapdoor, which nobody knows unless all M parties pool their draws.  [The reference's loop appends the unchanged base 2n
times (mpc_ac20.py:71-76), so there is nothing to mirror bit for bit.]  The parties are semi-honest, as everywhere in
this package: a received pp is checked to be points of the curves, none at infinity, but NOT - by pairings - to be the
previous pp times powers of ONE z; a deviating party could hand on a pp under which the later proofs do not verify.

The provers.  Everything the two provers do to the committed vector is linear - the MSMs, and the product
(gamma, x) * reversed(L), because L is public - so each party runs the single-party device path of
knowledge_of_exponent on its share vector, and the M results are recombined in the exponent
(Runtime.recombine_points, csrc/bn256_recombine.hip).  The proof is the single prover's byte for byte.
"""
import numpy as np

from . import knowledge_of_exponent as koe
from . import pynocchio as pn
from . import trinocchio
from .device import BnScalarVector, get_context

ORDER = pn.ORDER


class SharedVector:
    """This party's shares of n values mod the BN-256 order as one device vector.  Local operations only: len, slices
    (views) and the value of a PUBLIC form; a product of two shared vectors is `Runtime.schur_prod`."""
    __slots__ = ("sv", "rt")

    def __init__(self, sv, rt):
        self.sv, self.rt = sv, rt

    @classmethod
    def from_shares(cls, shares, rt, ctx=None):
        """from an (n, 32) uint8 array of residues below the order, or a list of ints"""
        ctx = ctx or rt._context()
        if isinstance(shares, np.ndarray):
            return cls(BnScalarVector.from_array(shares, ctx), rt)
        return cls(BnScalarVector.from_ints([int(v) for v in shares], ctx), rt)

    def __len__(self):
        return len(self.sv)

    def __getitem__(self, key):
        if isinstance(key, slice):
            return SharedVector(self.sv[key], self.rt)
        return self.sv[key]                                 # this party's share, an int

    def form(self, L):
        """this party's share of L(self) for a public form: a device inner product, plus the constant (every party's
        share of a public value is the value itself)"""
        coeffs = L.coeffs if isinstance(L.coeffs, BnScalarVector) else \
            BnScalarVector.from_ints([int(v) for v in L.coeffs], self.sv.ctx)
        assert len(coeffs) == len(self)
        return (coeffs.dot(self.sv) + int(getattr(L, "constant", 0))) % ORDER

    def __repr__(self):
        return f"<{len(self)} secret shares mod n>"       # never enters a transcript


def as_shared(x, rt):
    """a SharedVector as it is; an (n, 32) uint8 array or a list of ints as this party's shares"""
    if isinstance(x, SharedVector):
        return x
    if rt is None:
        raise ValueError("shares given as an array or a list need rt=")
    return SharedVector.from_shares(x, rt)


class Runtime(trinocchio.Runtime):
    """trinocchio.Runtime with the product of two shared vectors.  2 t >= M is refused by the constructor it inherits,
    and again by schur_prod (the threshold is a plain attribute), both before any launch."""

    def shared(self, sv):
        """a device vector of this party's shares (whatever class carries it) as a SharedVector"""
        return SharedVector(BnScalarVector(sv.v, sv.ctx), self)

    async def schur_prod(self, a, b, out=None, dst=None):
        """mpc.schur_prod over GF(n): shares of the element-wise product of two degree-t shared vectors.  Every party
        re-shares its product of shares with degree t (vmpc_bn256_fr_share_mul_deal_dev), one exchange, and the degree-2t
        polynomial through the M products is reduced with the Lagrange weights at 0
        (vmpc_bn256_fr_share_combine_dev).  out, dst: write result i to out[dst[i]] (dst: device pointer to uint32)
        instead of a new vector."""
        t, M = self.threshold, self.parties
        if 2 * t >= M:
            raise ValueError(f"schur_prod: a product of degree-{t} sharings has degree {2 * t}, which {M} parties "
                             f"cannot reduce (2 t < M)")
        assert len(a) == len(b)
        n, ctx = len(a), a.sv.ctx
        if n == 0:
            return SharedVector(BnScalarVector.empty(0, ctx), self)
        coeffs = ctx.upload(trinocchio.random_residues(self.rng, t * n)) if t else None
        dealt = ctx.alloc(32 * M * n)
        ctx.bn256_share_mul_deal(a.sv.ptr, b.sv.ptr, n, coeffs.ptr if t else None, t, M, dealt.ptr, n)
        table = ctx.download(dealt.ptr, 32 * M * n, (M, n, 32))
        got = await self.exchange_vectors([table[q] for q in range(M)])
        parts = ctx.upload(np.ascontiguousarray(np.stack(got)))
        res = out.sv if out is not None else BnScalarVector.empty(n, ctx)
        ctx.bn256_share_combine(parts.ptr, M, n, n, self.weights, dst, None, res.ptr)
        return out if out is not None else SharedVector(res, self)


# ---- the pp ------------------------------------------------------------------------------------------------------------
def _received_side(ctx, raw, n_points, group, name):
    """the bytes of one side of a pp as another party sent them -> a PPVector; ValueError unless they are n_points points
    of the curve, none at infinity"""
    width = 64 * group
    if not isinstance(raw, (bytes, bytearray)) or len(raw) != width * n_points:
        raise ValueError(f"koe_trusted_setup: {name} as received is not {n_points} points of {width} bytes")
    rows = np.frombuffer(bytes(raw), np.uint8).reshape(n_points, width)
    if not rows.any(axis=1).all():
        raise ValueError(f"koe_trusted_setup: {name} as received holds the point at infinity")
    buf = ctx.upload(rows)
    if ctx.bn256_validate(group, buf.ptr, n_points):
        raise ValueError(f"koe_trusted_setup: {name} as received holds a point not on the {koe._CURVE[group]}")
    return koe.PPVector(ctx, group, buf, n_points)


async def koe_trusted_setup(group, sectype, input_length, progress_bar=False, rt=None):
    """A pp for vectors of `input_length` scalars - 2 input_length points on either side - whose trapdoor is the product
    of the M parties' draws (mpc_ac20.py:54-84; the module's text says why this is not the reference's loop).  group:
    [G1, G2], each with `.generator`.  M rounds of one exchange each: in round p party p alone contributes, both sides of
    its pp as bytes; party 0's is trusted_setup's body under three draws from rt.rng (randrange(1, n) each: g_exp, alpha,
    z), party p > 0 applies update_setup under its three draws to what it received in round p - 1.  Every party validates
    what it receives (points of the curves, none at infinity: ValueError) and returns the same pp as PPVectors.
    `sectype` and `progress_bar` are the reference's arguments; they are accepted and not used."""
    if rt is None:
        raise ValueError("koe_trusted_setup: rt= (an mpc_koe.Runtime or a trinocchio.Runtime) is required")
    n = int(input_length)
    g1, g2 = group[0].generator, group[1].generator
    ctx = rt._context()
    pp = None
    for p in range(rt.parties):
        mine = None
        if p == rt.pid:
            g_exp, alpha, z = (rt.rng.randrange(1, ORDER) for _ in range(3))
            own = koe.setup_under(g1, g2, n, g_exp, alpha, z) if p == 0 else koe.update_setup(pp, g_exp, alpha, z)
            mine = (own["pp_lhs"].rows().tobytes(), own["pp_rhs"].rows().tobytes())
        every = await rt.hub.exchange(rt.pid, rt._next_tag("pp"), mine)
        if any((part is not None) != (q == p) for q, part in enumerate(every)):
            raise ValueError(f"koe_trusted_setup: round {p} takes a pp from party {p} and from nobody else")
        lhs, rhs = every[p]
        pp = {"pp_lhs": _received_side(ctx, lhs, 2 * n, 1, "pp_lhs"), "pp_rhs": _received_side(ctx, rhs, 2 * n, 2, "pp_rhs")}
    return pp


# ---- the provers -------------------------------------------------------------------------------------------------------
def _runtime(x, rt):
    rt = rt or x.rt
    if not isinstance(rt, trinocchio.Runtime):
        raise ValueError("the knowledge-of-exponent pivot over shares takes a runtime over GF(n): mpc_koe.Runtime")
    return rt


async def koe_restriction_argument_prover(S, x, gamma, pp, rt=None):
    """(P, pi) of knowledge_of_exponent.restriction_argument_prover for a shared x and a shared gamma (this party's
    share, an int): a local G1 MSM and a local G2 MSM over the shares (gamma's first), ONE exchange of the two points,
    and their recombination in the exponent (mpc_ac20.py:87-109).  x is committed to as a whole: S = range(len(x))."""
    x = as_shared(x, rt)
    rt = _runtime(x, rt)
    if not (isinstance(S, range) and S == range(len(x))):
        raise ValueError("koe_restriction_argument_prover: a shared vector is committed to as a whole, S = range(len(x))")
    P_p, pi_p = koe.restriction_argument_prover(S, x.sv, int(gamma) % ORDER, pp)
    P, pi = rt.recombine_points(await rt.exchange_points([P_p, pi_p]))
    return P, pi


async def koe_opening_linear_form_prover(L, x, gamma, pp, P=None, pi=None, rt=None):
    """(proof, u) of knowledge_of_exponent.opening_linear_form_prover for a shared x and gamma and a PUBLIC form L
    (mpc_ac20.py:112-138).  The product (gamma, x) * reversed(L) is linear in the shares: each party runs the device
    path on its share vector - stage, product (device.poly_product selects its method), split - and its Q_p is a local
    MSM; Q_p and the party's share of the product's coefficient n travel in ONE exchange, Q is recombined in the exponent,
    and u comes back OPENED: the recombined coefficient plus L's constant, an int below the order."""
    x = as_shared(x, rt)
    rt = _runtime(x, rt)
    ctx, n = x.sv.ctx, len(x)
    if len(pp["pp_lhs"]) != 2 * n:
        raise ValueError(f"koe_opening_linear_form_prover: a vector of {n} scalars takes a pp of {2 * n} points a side, "
                         f"this one has {len(pp['pp_lhs'])}")
    gamma = int(gamma) % ORDER
    if P is None:
        P, pi = await koe_restriction_argument_prover(range(n), x, gamma, pp, rt=rt)
    coeffs = L.coeffs if isinstance(L.coeffs, BnScalarVector) else BnScalarVector.from_ints([int(v) for v in L.coeffs], ctx)
    if len(coeffs) != n:
        raise ValueError("koe_opening_linear_form_prover: the form and the vector differ in length")
    (d_lhs, d_rhs), c_bar, d_u = koe._staged(ctx, x.sv, gamma, coeffs), ctx.alloc(32 * 2 * n), ctx.alloc(32)
    ctx.bn256_fr_poly_mul(d_lhs.ptr, n + 1, d_rhs.ptr, n, c_bar.ptr)
    ctx.bn256_koe_split(c_bar.ptr, n, d_u.ptr)
    Q_p = koe._side(ctx, pp, "pp_lhs").msm((c_bar, 2 * n))
    if Q_p.coords is not None:
        Q_p = pn.BN256Point((Q_p.coords[0], -Q_p.coords[1]))
    u_share = ctx.download(d_u.ptr, 32, (1, 32))
    every, opened = await rt.exchange_points([Q_p], scalars=u_share)
    Q = rt.recombine_points(every)[0]
    u = (opened[0] + int(getattr(L, "constant", 0))) % ORDER
    return {"P": P, "pi": pi, "Q": Q}, u
