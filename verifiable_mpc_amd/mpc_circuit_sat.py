"""Protocol 8 of AC20 over a SECRET-SHARED witness (verifiable_mpc/ac20/mpc_ac20_cb.py:39-189): M parties that hold
Shamir shares of x jointly produce ONE circuit-satisfiability proof, and nobody sees x.  One party's side, on its GPU.

    protocol_8_excl_pivot_prover     mpc_ac20_cb.py:39-154
    circuit_sat_prover               mpc_ac20_cb.py:157-189 (PivotChoice.compressed and .pivot)

The join of circuit_sat_gpu.py (Protocol 8 from a SparseCircuit, one prover who knows x) and mpc_ac20.py (the pivot over
shares).  Everything Protocol 8 does to z is linear - the wires' forms, the extension of f and g, the three forms at the
challenge, the commitment - except the gate outputs and h = f g: those are `PartyRuntime.schur_prod`
(csrc/mpc_share.hip), one exchange per depth level and one for h.  The share vector stays in HBM from x to z'.

Compact transcript only (DESIGN.md sections 15 and 18): the proof has the keys and types of
circuit_sat_gpu.circuit_sat_prover's and the unchanged single-party verifiers accept it.

Generators that are a knowledge-of-exponent pp ({"pp_lhs", "pp_rhs"}) select the same flow over GF(n), the BN-256 group
order: a SparseCircuit of that order, GF(n), an mpc_koe.Runtime, x as an mpc_koe.SharedVector (or
this party's shares as an (n_in, 32) uint8 array or a list of ints), the commitment and the opening by mpc_koe.  The
share vector's class and the `bn=` of the kernels are read from the circuit's field; the witness is computed by ONE
body for both fields.  The proof is 256 bytes of points at every N and is the single prover's under the same draws.
"""
import numpy as np

from . import circuit_sat_gpu as cs
from . import compressed_pivot as cp
from . import pivot
from . import mpc_koe
from .device import ScalarVector
from .groups import ORDER
from .mpc_ac20 import SecureScalar, SecureVector, _as_secure_vector, protocol_5_prover, vector_commitment


STAGE_HOOK = None       # scripts/mpc_circuit_sat_probe.py sets it: STAGE_HOOK(rt, name) when a stage of the prover ends


def _stage_end(rt, name):
    if STAGE_HOOK is not None:
        STAGE_HOOK(rt, name)


class _Levels:
    """A and B with their rows in depth-level order, in HBM: the rows of one level are then consecutive, and a launch
    over rows lo..hi leaves that level's wire values as two dense vectors, ready for the product kernel"""

    def __init__(self, circuit, ctx):
        order = circuit.level_order.astype(np.int64)
        self.order = order
        self.mats = []
        for M in (circuit.A, circuit.B):
            lens = np.diff(M.row_ptr)[order]
            ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            # entry e of the permuted matrix is entry src[e] of M
            src = np.repeat(M.row_ptr[:-1][order] - ptr[:-1], lens) + np.arange(int(ptr[-1]), dtype=np.int64)
            nnz = len(src)
            self.mats.append((ctx.upload(ptr.astype(np.uint32)),
                              ctx.upload(M.col[src].astype(np.uint32)) if nnz else ctx.alloc(4),
                              ctx.upload(np.ascontiguousarray(M.vals[src])) if nnz else ctx.alloc(32),
                              ctx.upload(np.ascontiguousarray(M.consts[order]))))

    def csr(self, which, lo):
        """rows lo.. of the permuted A (0) / B (1): row_ptr holds absolute entry offsets, so only it and the constants
        are offset"""
        ptr, col, vals, consts = self.mats[which]
        return (ptr.ptr + 4 * lo, col.ptr, vals.ptr, consts.ptr + 32 * lo)


def _levels(circuit, ctx):
    lv = getattr(circuit, "_mpc_levels", None)
    if lv is None:
        lv = circuit._mpc_levels = _Levels(circuit, ctx)
    return lv


def _shares_class(circuit):
    """(the class of a party's share vector, what turns the caller's shares into one) in the circuit's field"""
    if circuit.field.bn:
        return mpc_koe.SharedVector, mpc_koe.as_shared
    return SecureVector, _as_secure_vector


async def _witness_on_device(circuit, x, rt, gamma_witness=None, n_random=2):
    """this party's shares of z = (x, f(0), g(0), h(0), h(1..2m)) as a share vector of the circuit's field (SecureVector
    over GF(l), mpc_koe.SharedVector over GF(n)), and of the n_random >= 2 dealt secrets: r_a, r_b, then the caller's"""
    n_in, m, n_x = len(x), circuit.m, circuit.n_x
    d = circuit.device()
    ctx, bn = d["ctx"], circuit.field.bn
    Vec, (Shares, as_shares) = circuit.field.vector, _shares_class(circuit)
    N, g_off = n_in + 3 + 2 * m, n_in + 3
    z = Vec.empty(N, ctx)
    zs = Shares(z, rt)
    if n_in:
        ctx.copy(z.ptr, x.sv.ptr, 32 * n_in)
    a, b = Vec.empty(m + 1, ctx), Vec.empty(m + 1, ctx)
    if gamma_witness is not None:
        if len(gamma_witness) != m:
            raise ValueError(f"gamma_witness: {m} gate outputs expected")
        if m:
            ctx.copy(z.ptr + 32 * g_off, as_shares(gamma_witness, rt).sv.ptr, 32 * m)
    elif m:
        # level by level: shares of the wires (local), shares of their products (one exchange), into z's gammas
        lv = _levels(circuit, ctx)
        zpos = ctx.upload((g_off + lv.order).astype(np.uint32))
        widest = int(np.diff(circuit.level_ptr).max())
        a_lv, b_lv = Vec.empty(widest, ctx), Vec.empty(widest, ctx)
        for level in range(len(circuit.level_ptr) - 1):
            lo, hi = int(circuit.level_ptr[level]), int(circuit.level_ptr[level + 1])
            ctx.cs_triples(lv.csr(0, lo), lv.csr(1, lo), None, hi - lo, n_x, g_off, z.ptr, a_lv.ptr, b_lv.ptr, 2, bn=bn)
            await rt.schur_prod(Shares(a_lv[:hi - lo], rt), Shares(b_lv[:hi - lo], rt), out=zs,
                                dst=zpos.ptr + 4 * lo)
    _stage_end(rt, "triples")
    if m:
        # the wires in gate order, for f and g: z's gammas are all there now, one launch
        ctx.cs_triples(d["A"].csr(), d["B"].csr(), None, m, n_x, g_off, z.ptr, a.ptr, b.ptr, 2, bn=bn)
    r = await rt.random_shares(n_random)                # r_a, r_b: degree `threshold`, they are multiplied below
    r_ptr = getattr(r, "sv", r).ptr                     # (a SecureVector over GF(l), a bare device vector over GF(n))
    ctx.copy(a.ptr + 32 * m, r_ptr, 32)
    ctx.copy(b.ptr + 32 * m, r_ptr + 32, 32)
    k = max(m, 1)
    f, g = Vec.empty(k, ctx), Vec.empty(k, ctx)
    ctx.cs_extend_fg(a.ptr, b.ptr, m, d["fact"].ptr, d["ifact"].ptr, f.ptr, g.ptr, bn=bn)
    if m:
        # (f(0), f(m+1), f(m+2..2m)) times g's gives (h(0), h(m+1), h(m+2..2m)): z[n_in + 2] and z's last m positions
        F, G = Vec.empty(m + 1, ctx), Vec.empty(m + 1, ctx)
        for V, v, src in ((F, f, a), (G, g, b)):
            ctx.copy(V.ptr, v.ptr, 32)
            ctx.copy(V.ptr + 32, src.ptr + 32 * m, 32)
            if m > 1:
                ctx.copy(V.ptr + 64, v.ptr + 32, 32 * (m - 1))
        dst = ctx.upload(np.concatenate([[n_in + 2], g_off + m + np.arange(m)]).astype(np.uint32))
    else:
        F, G = f, g                                     # f = r_a, g = r_b: z = x + [r_a, r_b, r_a r_b]
        dst = ctx.upload(np.array([n_in + 2], np.uint32))
    _stage_end(rt, "extension")
    await rt.schur_prod(Shares(F, rt), Shares(G, rt), out=zs, dst=dst.ptr)
    ctx.copy(z.ptr + 32 * n_in, f.ptr, 32)
    ctx.copy(z.ptr + 32 * (n_in + 1), g.ptr, 32)
    _stage_end(rt, "schur")
    return zs, r


async def protocol_8_excl_pivot_prover(generators, circuit, x, gf, use_koe=False, rt=None, gamma_witness=None):
    """mpc_ac20_cb.py:39-154 for a SparseCircuit (anything `as_sparse` takes is converted): (proof, z_commitment, L, z,
    gamma) with z a SecureVector, gamma a SecureScalar and L a public AffineForm over device coefficients.  x: a
    SecureVector or a list of SecureScalar.  gamma_witness: shares of the gate outputs the parties already hold from
    their computation (a SecureVector or a list) - no exchange per depth level then; whether they are the products of
    their wires is settled by y1 y2 = y3.  Generators that are a knowledge-of-exponent pp take the same flow over GF(n)
    (_protocol_8_koe below): z is then a mpc_koe.SharedVector, gamma this party's share as an int, z_commitment
    {"P", "pi"}."""
    if "pp_lhs" in generators:
        return await _protocol_8_koe(generators, circuit, x, gf, rt, gamma_witness)
    if use_koe or "g" not in generators:
        raise NotImplementedError("Protocol 8 over shares: the knowledge-of-exponent variant takes a pp over BN-256 "
                                  "(mpc_koe.koe_trusted_setup) as generators; these are Ed25519's")
    circuit = cs.as_sparse(circuit)
    x = _as_secure_vector(x, rt)
    rt = rt or x.rt
    g, h = generators["g"], generators["h"]
    order = gf.order
    assert order == ORDER
    n_in, m, n_x = len(x), circuit.m, circuit.n_x
    if n_in < n_x:
        raise ValueError(f"the circuit has {n_x} inputs, {n_in} given")
    z, _ = await _witness_on_device(circuit, x, rt, gamma_witness)
    d = circuit.device()
    ctx, g_off = d["ctx"], n_in + 3

    gamma = (await rt.random_shares(1))[0]
    z_commitment = await vector_commitment(z, gamma, g, h)
    _stage_end(rt, "commitment")
    proof = {"z_commitment": z_commitment}
    digest = cs._first_digest(z_commitment, circuit, n_in)
    c = cs.first_challenge(digest, order)
    cs._check_not_node(c, m)

    # the forms are public; their values on the share vector are shares of y1, y2, y3 and of the outputs
    forms = cs._Forms(circuit, n_in, c, order)
    secret = [SecureScalar(v, rt) for v in forms.values(z.sv)]
    if circuit.n_out:
        o1 = ScalarVector.empty(circuit.n_out, ctx)
        ctx.cs_triples(d["O"].csr(), d["O"].csr(), None, circuit.n_out, n_x, g_off, z.sv.ptr, o1.ptr, o1.ptr, 2)
        secret += [SecureScalar(v, rt) for v in o1.to_ints()]
    opened = await rt.output(secret)
    y1, y2, y3 = opened[:3]
    if y1 * y2 != y3:
        raise ValueError("inconsistent shares: f(c) g(c) != h(c), the shared z is not a witness of this circuit")
    proof["y1"], proof["y2"], proof["y3"] = y1, y2, y3
    outputs = list(opened[3:])
    proof["outputs"] = outputs
    rho = cs._second_challenge(digest, (y1, y2, y3), outputs, order)
    L = forms.combine(rho, (y1, y2, y3), outputs, gf)
    proof["L"] = L
    return proof, z_commitment, L, z, gamma


async def _protocol_8_koe(generators, circuit, x, gf, rt, gamma_witness):
    """protocol_8_excl_pivot_prover over GF(n) with a knowledge-of-exponent pp: the same flow
    with the field read from the circuit, z a mpc_koe.SharedVector, gamma this party's share (an int) and z_commitment
    {"P", "pi"}.  D + 3 exchanges up to here for D depth levels (levels, ONE deal of r_a, r_b and gamma, h, the
    commitment's points, the opening of y and the outputs) - the pivot's opening is the last, D + 5 in all.  Everything
    that can be refused is refused before the first exchange."""
    circuit = cs.as_sparse(circuit, cs._Koe.order)
    cs._check_field(cs._Koe, circuit, gf)
    rt = rt or getattr(x, "rt", None)
    if not isinstance(rt, mpc_koe.Runtime):
        raise ValueError("Protocol 8 over shares with a knowledge-of-exponent pp: the shares are mod the BN-256 order and "
                         "the runtime is an mpc_koe.Runtime, not a runtime over GF(l)")
    x = mpc_koe.as_shared(x, rt)
    order = gf.order
    n_in, m, n_x = len(x), circuit.m, circuit.n_x
    if n_in < n_x:
        raise ValueError(f"the circuit has {n_x} inputs, {n_in} given")
    N = n_in + 3 + 2 * m
    if len(generators["pp_lhs"]) != 2 * N or len(generators["pp_rhs"]) != 2 * N:
        raise ValueError(f"the pp holds {len(generators['pp_lhs'])} and {len(generators['pp_rhs'])} points; a witness "
                         f"of {N} scalars takes {2 * N} on either side")
    z, r = await _witness_on_device(circuit, x, rt, gamma_witness, n_random=3)
    d = circuit.device()
    ctx, g_off = d["ctx"], n_in + 3

    gamma = int.from_bytes(ctx.download(r.ptr + 64, 32).tobytes(), "little")
    P, pi = await mpc_koe.koe_restriction_argument_prover(range(N), z, gamma, generators, rt=rt)
    z_commitment = {"P": P, "pi": pi}
    _stage_end(rt, "commitment")
    proof = {"z_commitment": z_commitment}
    digest = cs._first_digest(z_commitment, circuit, n_in)
    c = cs.first_challenge(digest, order)
    cs._check_not_node(c, m)

    forms = cs._Forms(circuit, n_in, c, order)
    secret = forms.values(z.sv)
    if circuit.n_out:
        o1 = circuit.field.vector.empty(circuit.n_out, ctx)
        ctx.cs_triples(d["O"].csr(), d["O"].csr(), None, circuit.n_out, n_x, g_off, z.sv.ptr, o1.ptr, o1.ptr, 2, bn=True)
        secret += o1.to_ints()
    opened = [gf(v) for v in await rt.output(circuit.field.vector.from_ints(secret, ctx))]
    y1, y2, y3 = opened[:3]
    if y1 * y2 != y3:
        raise ValueError("inconsistent shares: f(c) g(c) != h(c), the shared z is not a witness of this circuit")
    proof["y1"], proof["y2"], proof["y3"] = y1, y2, y3
    outputs = list(opened[3:])
    proof["outputs"] = outputs
    rho = cs._second_challenge(digest, (y1, y2, y3), outputs, order, cs._Koe.second_tag)
    L = forms.combine(rho, (y1, y2, y3), outputs, gf)
    proof["L"] = L
    return proof, z_commitment, L, z, gamma


async def prove_linear_form_eval(g, h, P, L, y, x, gamma, gf, rt=None):
    """Protocol 2 (pivot.py:156-181) over a SecureVector x: (z, phi, c) as pivot.verify_linear_form_proof takes them.
    Its response IS the opened vector z = c x + r."""
    rt = rt or x.rt
    L, y = pivot.affine_to_linear(L, y, len(x))
    order = gf.order
    if isinstance(y, SecureScalar):
        y = await rt.output(y)
    r = SecureVector(cp.masks(len(x), x.sv.ctx), rt)        # used linearly only
    rho = rt._random()
    A = await vector_commitment(r, rho, g, h)
    t = await rt.output(r.form(L))
    c = pivot._pis_challenge(t, A, g, h, P, L, y, order)
    z = await rt.output(x.axpy(c, r))
    phi = int(await rt.output(c * gamma + rho)) % order
    return z, phi, c


async def circuit_sat_prover(generators, circuit, x, gf, pivot_choice="compressed", rt=None, gamma_witness=None):
    """mpc_ac20_cb.py:157-189 for a SparseCircuit: every party returns the same compact proof, which
    circuit_sat_gpu.circuit_sat_verifier and circuit_sat_verifier_batch accept as they are.  With a knowledge-of-exponent
    pp as generators (and PivotChoice.koe) the pivot is mpc_koe.koe_opening_linear_form_prover: three points, and L(z) is
    opened by it - anything but 0 is ValueError"""
    choice = cs._choice(pivot_choice)
    if "pp_lhs" in generators:
        cs._check_choice(choice, True)                   # a pp goes with PivotChoice.koe, and with nothing else
        proof, z_commitment, L, z, gamma = await protocol_8_excl_pivot_prover(generators, circuit, x, gf, rt=rt,
                                                                              gamma_witness=gamma_witness)
        proof["pivot_proof"], u = await mpc_koe.koe_opening_linear_form_prover(L, z, gamma, generators, z_commitment["P"],
                                                                               z_commitment["pi"], rt=z.rt)
        _stage_end(z.rt, "pivot")
        if u != 0:
            raise ValueError("inconsistent shares: L(z) opens to a value other than 0")
        return proof
    if choice == "koe":
        raise NotImplementedError("PivotChoice.koe over shares takes a pp over BN-256 (mpc_koe.koe_trusted_setup) as "
                                  "generators; these are Ed25519's")
    if choice not in ("compressed", "pivot"):
        raise NotImplementedError
    proof, z_commitment, L, z, gamma = await protocol_8_excl_pivot_prover(generators, circuit, x, gf, rt=rt,
                                                                          gamma_witness=gamma_witness)
    y = z.form(L)                                        # shares of L(z) = 0, opened by the pivot
    if choice == "compressed":
        proof["pivot_proof"] = await protocol_5_prover(generators, z_commitment, L, y, z, gamma, gf, rt=z.rt,
                                                       transcript="compact")
    else:
        proof["pivot_proof"] = await prove_linear_form_eval(generators["g"], generators["h"], z_commitment, L, y, z,
                                                            gamma, gf, rt=z.rt)
    _stage_end(z.rt, "pivot")
    return proof


def dispatching(name, original):
    """the coroutine `install_mpc` binds in the reference's mpc_ac20_cb: a SparseCircuit goes to this module, any other
    circuit object to the reference's own coroutine"""
    mine = globals()[name]

    async def dispatch(generators, circuit, x, gf, *args, **kwargs):
        if isinstance(circuit, cs.SparseCircuit):
            return await mine(generators, circuit, x, gf, *args, **kwargs)
        return await original(generators, circuit, x, gf, *args, **kwargs)
    dispatch.__name__ = name
    return dispatch
