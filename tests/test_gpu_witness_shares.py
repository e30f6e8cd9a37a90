"""The R1CS solve on Shamir shares on the GPU (csrc/bn256_r1cs_share.hip, trinocchio.calculate_witness_shares and
prove_inputs).  The two kernels bit for bit against the big-int restatement of
tests/witness_share_ref.py - round widths at the wave and workgroup edges, strides with guards, every operand n - 1,
the argument rules; the protocol over one LocalHub - any t + 1 outputs recombine to the clear witness, one exchange per
round, batches, schedules, fresh randomness, the degree of what a party sends; and end to end from shares of the inputs
to one proof that pynocchio.verify accepts."""
import asyncio
import ctypes
import functools
import itertools
import random

import numpy as np
import pytest

from tests import keygen_ref as K
from tests import witness_ref as WR
from tests import witness_share_ref as SR
from tests.test_gpu_pinocchio_h import ALL_TRUE, _gen, _qaps, _seeded_td, load_golden
from tests.test_gpu_trinocchio import RecordingHub, _same, _to_ints

pytestmark = pytest.mark.gpu
N = K.N
MT = [(1, 0), (3, 1), (4, 1), (5, 2)]
PARTIES = [(3, 1), (5, 2)]
GUARD = 0xA5


@pytest.fixture(scope="module")
def pn():
    import verifiable_mpc_amd as v
    v.get_context()
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def tn(pn):
    from verifiable_mpc_amd import trinocchio
    return trinocchio


@pytest.fixture(scope="module")
def ctx(pn):
    from verifiable_mpc_amd import get_context
    return get_context()


@pytest.fixture(scope="module")
def nat():
    from verifiable_mpc_amd import _native
    return _native


def qap_of(pn, r1cs, out_ix):
    V, W, Y, m = r1cs
    return pn.R1CSQAP(WR.csr(V), WR.csr(W), WR.csr(Y), out_ix, m=m)


def to_ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


# ---- the two kernels, bit for bit ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _one_round(n_r):
    """a circuit whose only round has n_r product rows, behind a local phase (so r0 > 0) -> (r1cs, the round's rows)"""
    r1cs = SR.share_layered_r1cs([n_r], [1, 1], seed=300 + n_r)
    ph, _ = SR.phases(r1cs, 2)
    assert SR.round_widths(ph) == [n_r]
    return r1cs, ph[1][2]


def _round_on_device(pn, ctx, r1cs, body, k, M, t, rng, worst=False):
    """one mul_deal and one finish over the circuit's round on k random share vectors, strides wider than needed and
    filled with a guard -> nothing; asserts every byte"""
    qap = qap_of(pn, r1cs, 2)
    plan = pn.ShareSolvePlan(qap, 2)
    ptrs, _ = plan.device(ctx)
    r0, r1 = plan.round_rows(1)
    n_r, m = r1 - r0, qap.m
    assert n_r == len(body) and r0 > 0
    n_e, c_stride, out_stride = k * n_r, m + 1 + 3, k * n_r + 5
    draw = (lambda: N - 1) if worst else (lambda: rng.randrange(N))
    c = [[1] + [draw() for _ in range(m)] for _ in range(k)]
    coeffs = [[draw() for _ in range(n_e)] for _ in range(t)]
    host = np.full((k, c_stride, 32), GUARD, np.uint8)
    host[:, :m + 1] = np.stack([K.to_array(cw) for cw in c])
    dc = ctx.upload(host)
    dco = ctx.upload(K.to_array([x for row in coeffs for x in row])) if t else None
    out = ctx.upload(np.full((M, out_stride, 32), GUARD, np.uint8))
    ctx.bn256_r1cs_share_mul_deal(ptrs, r0, r1, m, dc.ptr, c_stride, k, dco.ptr if t else None, t, M, out.ptr, out_stride)
    ctx.sync()
    got = ctx.download(out.ptr, 32 * M * out_stride, (M, out_stride, 32))
    assert (got[:, n_e:] == GUARD).all()
    assert np.array_equal(ctx.download(dc.ptr, host.nbytes, host.shape), host)          # the deal stores nothing in c
    want = [[None] * n_e for _ in range(M)]
    for w in range(k):
        for i, x in enumerate(body):
            e = w * n_r + i
            for q, v in enumerate(SR.deal_element(x, c[w], [coeffs[j][e] for j in range(t)], M)):
                want[q][e] = v
    assert np.array_equal(got[:, :n_e], np.stack([K.to_array(row) for row in want]))
    # finish: any canonical parts and weights
    parts = [[draw() for _ in range(out_stride)] for _ in range(M)]
    weights = [draw() for _ in range(M)]
    dp = ctx.upload(np.stack([K.to_array(row) for row in parts]))
    ctx.bn256_r1cs_share_finish(ptrs, r0, r1, m, dp.ptr, M, out_stride, weights, dc.ptr, c_stride, k)
    ctx.sync()
    got = ctx.download(dc.ptr, host.nbytes, host.shape)
    assert (got[:, m + 1:] == GUARD).all()
    for w in range(k):
        cw = list(c[w])
        for i, x in enumerate(body):
            cw[x["wire"]] = SR.finish_element(x, c[w], [parts[p][w * n_r + i] for p in range(M)], weights)
        assert np.array_equal(got[w, :m + 1], K.to_array(cw)), w


@pytest.mark.parametrize("n_r", [1, 63, 64, 65, 256, 257])
def test_kernels_against_the_restatement(pn, ctx, n_r):
    r1cs, body = _one_round(n_r)
    rng = random.Random(n_r)
    for k in (1, 3):
        for M, t in MT:
            _round_on_device(pn, ctx, r1cs, body, k, M, t, rng)


def test_kernels_with_every_operand_n_minus_1(pn, ctx):
    """65 rows (-x1 - x2 - 1)(-x1 - x2 - 1) = -s - x1: plan coefficients, share vectors, dealt coefficients, parts and
    weights all n - 1, three entries per dot, four parties (four products of n - 1 need 513 bits)"""
    n_r = 65
    side = [(1, -1), (2, -1), (0, -1)]
    r1cs = ([side] * n_r + [[(0, -1)]], [side] * n_r + [[(1, -1)]],
            [[(3 + i, -1), (1, -1), (2, -1)] for i in range(n_r)] + [[(3 + n_r, -1)]], 3 + n_r)
    ph, _ = SR.phases(r1cs, 2)
    assert SR.round_widths(ph) == [n_r] and SR.local_depths(ph) == [1, 0]
    for k in (1, 3):
        for t in (1, 3):
            _round_on_device(pn, ctx, r1cs, ph[1][2], k, 4, t, random.Random(1), worst=True)


def test_argument_rules(pn, ctx, nat):
    deal, fin, h = ctx.lib.vmpc_bn256_r1cs_share_mul_deal_dev, ctx.lib.vmpc_bn256_r1cs_share_finish_dev, ctx.handle
    nil6, nil5, big = [None] * 6, [None] * 5, (1 << 31) + 1
    w1 = ctypes.create_string_buffer(K.to_array([1] * 65).tobytes(), 32 * 65)
    # deal: (6 plan pointers, r0, r1, m, c, c_stride, n_wit, coeffs, t, parties, out, out_stride)
    # finish: (5 plan pointers, r0, r1, m, parts, parties, part_stride, weights, c, c_stride, n_wit)
    # VMPC_E_RANGE before any pointer is looked at
    assert deal(h, *nil6, 0, 2, 4, None, 5, 1, None, 1, 65, None, 2) == nat.E_RANGE              # parties
    assert fin(h, *nil5, 0, 2, 4, None, 65, 2, w1, None, 5, 1) == nat.E_RANGE
    assert deal(h, *nil6, 0, 2, 4, None, 5, nat.BN256_R1CS_MAX_WIT + 1, None, 1, 3, None, 1 << 20) == nat.E_RANGE
    assert fin(h, *nil5, 0, 2, 4, None, 3, 1 << 20, w1, None, 5, nat.BN256_R1CS_MAX_WIT + 1) == nat.E_RANGE
    assert deal(h, *nil6, 0, 2, 4, None, big, 1, None, 1, 3, None, 2) == nat.E_RANGE             # c_stride
    assert deal(h, *nil6, 0, 2, 4, None, 5, 1, None, 1, 3, None, big) == nat.E_RANGE             # out_stride
    assert fin(h, *nil5, 0, 2, 4, None, 3, big, w1, None, 5, 1) == nat.E_RANGE                   # part_stride
    assert deal(h, *nil6, 0, 1 << 20, 4, None, 5, 1 << 12, None, 1, 3, None, 1 << 31) == nat.E_RANGE      # n_e = 2^32
    assert fin(h, *nil5, 0, 1 << 20, 4, None, 3, 1 << 31, w1, None, 5, 1 << 12) == nat.E_RANGE
    assert deal(h, *nil6, 0, 2, 4, None, 4, 1, None, 1, 3, None, 2) == nat.E_RANGE               # c_stride < m + 1
    assert fin(h, *nil5, 0, 2, 4, None, 3, 2, w1, None, 4, 1) == nat.E_RANGE
    # VMPC_E_INVAL
    assert deal(h, *nil6, 0, 2, 4, None, 5, 1, None, 3, 3, None, 2) == nat.E_INVAL               # t >= parties
    assert deal(h, *nil6, 0, 2, 4, None, 5, 3, None, 1, 3, None, 5) == nat.E_INVAL               # out_stride < n_e = 6
    assert fin(h, *nil5, 0, 2, 4, None, 3, 5, w1, None, 5, 3) == nat.E_INVAL                     # part_stride < n_e
    assert deal(h, *nil6, 2, 1, 4, None, 5, 1, None, 1, 3, None, 2) == nat.E_INVAL               # r1 < r0
    assert fin(h, *nil5, 2, 1, 4, None, 3, 2, w1, None, 5, 1) == nat.E_INVAL
    assert deal(h, *nil6, 0, 2, 4, None, 5, 1, None, 1, 3, None, 2) == nat.E_INVAL               # null pointers, work
    assert fin(h, *nil5, 0, 2, 4, None, 3, 2, w1, None, 5, 1) == nat.E_INVAL
    assert fin(h, *nil5, 0, 2, 4, None, 3, 2, None, None, 5, 1) == nat.E_INVAL                   # no weights
    # an empty range or no witness: VMPC_OK, nothing launched (the null pointers would fault a launch)
    ctx.profile(True)
    try:
        ctx.profile_read()
        assert deal(h, *nil6, 2, 2, 4, None, 5, 1, None, 1, 3, None, 0) == nat.OK
        assert deal(h, *nil6, 0, 2, 4, None, 5, 0, None, 1, 3, None, 0) == nat.OK
        assert fin(h, *nil5, 2, 2, 4, None, 3, 0, w1, None, 5, 1) == nat.OK
        assert fin(h, *nil5, 0, 2, 4, None, 3, 0, w1, None, 5, 0) == nat.OK
        ctx.sync()
        assert all(count == 0 for _, count in ctx.profile_read().values())
    finally:
        ctx.profile(False)
    # a weight >= n: VMPC_E_NONCANON at once, an empty range included
    wn = ctypes.create_string_buffer(K.to_array([1, N, 1]).tobytes(), 96)
    assert fin(h, *nil5, 2, 2, 4, None, 3, 0, wn, None, 5, 1) == nat.E_NONCANON


def test_noncanonical_part_is_reported_and_its_wire_left_alone(pn, ctx, nat):
    r1cs, body = _one_round(3)
    qap = qap_of(pn, r1cs, 2)
    plan = pn.ShareSolvePlan(qap, 2)
    ptrs, _ = plan.device(ctx)
    r0, r1 = plan.round_rows(1)
    m = qap.m
    c = [1] + [7 + i for i in range(m)]
    parts = [[1, 2, 3], [4, N, 6]]
    dc, dp = ctx.upload(K.to_array(c)), ctx.upload(K.to_array(parts[0] + parts[1]))
    ctx.bn256_r1cs_share_finish(ptrs, r0, r1, m, dp.ptr, 2, 3, [1, 1], dc.ptr, m + 1, 1)
    with pytest.raises(nat.VmpcError) as e:
        ctx.sync()
    assert e.value.code == nat.E_NONCANON
    want = list(c)
    for i in (0, 2):
        want[body[i]["wire"]] = SR.finish_element(body[i], c, [parts[0][i], parts[1][i]], [1, 1])
    assert to_ints(ctx.download(dc.ptr, 32 * (m + 1))) == want                 # row 1's wire keeps its old value
    ctx.sync()                                                                 # reported once


# ---- the protocol over one hub -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fixture_cases():
    return {c["name"]: c for c in load_golden("pinocchio_keygen.json")["cases"]}


@functools.lru_cache(maxsize=None)
def _circuit(name):
    """-> (r1cs, n_in, three input vectors, their clear witnesses by the restatement): made once, never changed"""
    if name == "generated":
        r1cs, n_in = SR.share_layered_r1cs([65, 1, 257], [3, 0, 2, 1], seed=23), 2
    else:
        case = _fixture_cases()[name]
        r1cs, n_in = WR.from_dense(case), len(case["inputs"])
    rng = random.Random(name)
    inputs = [[rng.randrange(N) for _ in range(n_in)] for _ in range(2)] + [[N - 1 - i for i in range(n_in)]]
    if name != "generated":
        inputs[0] = list(_fixture_cases()[name]["inputs"])
    return r1cs, n_in, inputs, [WR.solve(r1cs, x) for x in inputs]


def _qap(pn, name):
    if name == "generated":
        return qap_of(pn, _circuit(name)[0], 2)
    return _qaps(pn, _fixture_cases()[name])["r1cs"]


def _run(tn, qap, x_shares, M, t, seed, **kw):
    """the M parties as coroutines over one hub -> (outputs in party order, runtimes, hub)"""
    hub = RecordingHub(tn, M)
    rts = [tn.Runtime(p, M, t, random.Random(1000 * seed + p), hub) for p in range(M)]

    async def main():
        return await asyncio.gather(*(tn.calculate_witness_shares(rts[p], qap, x_shares[p], **kw) for p in range(M)))
    return asyncio.run(main()), rts, hub


def _assert_recombines(outs, want, M, t):
    """every (t + 1)-subset of the parties' outputs recombines, wire by wire, to `want`: the value and the degree"""
    cols = [to_ints(o) for o in outs]
    for subset in itertools.combinations(range(M), t + 1):
        lam = SR.lagrange_at_zero([p + 1 for p in subset])
        got = [sum(l * cols[p][w] for l, p in zip(lam, subset)) % N for w in range(len(want))]
        assert got == want, subset


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", ["demo", "larger", "generated"])
def test_shares_of_the_witness(pn, tn, name, M, t):
    r1cs, n_in, inputs, want = _circuit(name)
    qap = _qap(pn, name)
    plan = pn.ShareSolvePlan(qap, n_in)
    assert pn.calculate_witness(qap, inputs[0]) == want[0]
    rng = random.Random(M)
    # one input vector, as a list of ints and as an (n_in, 32) array
    xs = SR.share(inputs[0], t, M, rng)
    outs, rts, hub = _run(tn, qap, xs, M, t, seed=1)
    assert all(o.shape == (qap.m + 1, 32) and o.dtype == np.uint8 for o in outs)
    assert all(to_ints(o[0]) == [1] for o in outs)
    assert [to_ints(outs[p][1:n_in + 1]) for p in range(M)] == xs
    _assert_recombines(outs, want[0], M, t)
    assert [rt.exchanges for rt in rts] == [plan.n_rounds] * M and len(hub.log) == plan.n_rounds
    again, _, _ = _run(tn, qap, [K.to_array(x) for x in xs], M, t, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(outs, again))
    # K = 3: as many exchanges, every witness of the batch
    shared = [SR.share(x, t, M, rng) for x in inputs]
    batch = [np.stack([K.to_array(shared[w][p]) for w in range(3)]) for p in range(M)]
    outs, rts, hub = _run(tn, qap, batch, M, t, seed=2)
    assert all(o.shape == (3, qap.m + 1, 32) for o in outs)
    clear = pn.calculate_witness_batch(qap, inputs)
    for w in range(3):
        assert to_ints(clear[w]) == want[w]
        _assert_recombines([o[w] for o in outs], want[w], M, t)
    assert [rt.exchanges for rt in rts] == [plan.n_rounds] * M


def test_fixture_rounds_on_the_device_plan(pn):
    assert [pn.ShareSolvePlan(_qap(pn, name), _circuit(name)[1]).n_rounds for name in ("demo", "larger", "generated")] == \
        [2, 7, 3]


@pytest.mark.parametrize("name", ["larger", "generated"])
def test_one_party_is_the_clear_solve(pn, tn, name):
    r1cs, n_in, inputs, want = _circuit(name)
    qap = _qap(pn, name)
    outs, rts, _ = _run(tn, qap, [np.stack([K.to_array(x) for x in inputs])], 1, 0, seed=4)
    assert np.array_equal(outs[0], pn.calculate_witness_batch(qap, inputs))
    assert rts[0].exchanges == pn.ShareSolvePlan(qap, n_in).n_rounds


def test_schedules_agree_byte_for_byte(pn, tn):
    r1cs, n_in, inputs, want = _circuit("generated")
    qap = _qap(pn, "generated")
    xs = SR.share(inputs[1], 1, 3, random.Random(8))
    runs = [_run(tn, qap, xs, 3, 1, seed=6, wide_rows=wide)[0] for wide in (0, 1)]
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    _assert_recombines(runs[0], want[1], 3, 1)


@pytest.mark.parametrize("M,t", PARTIES)
def test_randomness_and_the_degree_of_what_a_party_sends(pn, tn, M, t):
    """two runs that differ only in the parties' rng seeds send different tables and end in the same witness; in a
    recorded round the M values a party dealt for an element lie on a polynomial of degree <= t: the Lagrange
    extrapolation from its first t + 1 values gives the others"""
    r1cs, n_in, inputs, want = _circuit("larger")
    qap = _qap(pn, "larger")
    xs = SR.share(inputs[1], t, M, random.Random(11))
    runs = [_run(tn, qap, xs, M, t, seed=s) for s in (1, 2)]
    for outs, _, _ in runs:
        _assert_recombines(outs, want[1], M, t)
    logs = [hub.log for _, _, hub in runs]
    assert list(logs[0]) == list(logs[1]) and all(tag[0] == "vec" for tag in logs[0])
    widths = SR.round_widths(SR.phases(r1cs, n_in)[0])
    for (tag, a), b, width in zip(logs[0].items(), logs[1].values(), widths):
        for p in range(M):
            assert len(a[p]) == M and all(row.shape == (width, 32) for row in a[p])
            assert not any(np.array_equal(a[p][q], b[p][q]) for q in range(M)), (tag, p)
    nodes = list(range(1, t + 2))
    for p in range(M):
        sent = [_to_ints(row) for row in logs[0][("vec", 1)][p]]                    # sent[q][e]
        for e in range(widths[0]):
            for q in range(t + 1, M):
                basis = [SR.recombine([int(i == j) for j in range(t + 1)], [x - (q + 1) for x in nodes])
                         for i in range(t + 1)]
                assert sum(b_i * sent[i][e] for i, b_i in enumerate(basis)) % N == sent[q][e], (p, e, q)
        assert len({sent[q][0] for q in range(M)}) == M                             # not a constant polynomial


def test_shared_divisor_is_refused_before_any_device_call_or_exchange(pn, tn, ctx):
    shared = ([[(1, 1)], [(3, 1)]], [[(1, 1)], [(2, 1)]], [[(4, 1)], [(1, 1)]], 4)       # row 2: wire 3 = x1 / x2
    qap = qap_of(pn, shared, 2)
    hub = RecordingHub(tn, 3)
    rt = tn.Runtime(0, 3, 1, random.Random(1), hub)
    ctx.profile(True)
    try:
        ctx.profile_read()
        with pytest.raises(ValueError, match=r"division by a shared value in constraint 2 "):
            asyncio.run(tn.calculate_witness_shares(rt, qap, [5, 6]))
        assert all(count == 0 for _, count in ctx.profile_read().values())
    finally:
        ctx.profile(False)
    assert rt.exchanges == 0 and not hub.log


def test_refusals_of_the_inputs(pn, tn):
    qap = _qap(pn, "demo")
    rt = tn.Runtime(0, 3, 1, random.Random(1), tn.LocalHub(3))
    with pytest.raises(ValueError, match="below n"):
        asyncio.run(tn.calculate_witness_shares(rt, qap, K.to_array([N - 1, N])[1:]))
    out = asyncio.run(tn.calculate_witness_shares(rt, qap, np.zeros((0, 1, 32), np.uint8)))
    assert out.shape == (0, qap.m + 1, 32) and rt.exchanges == 0

    class Dense:
        d, m, out_ix, v, w, y, t = 1, 1, 1, [], [], [], None
    with pytest.raises(TypeError, match=r"R1CSQAP\(V, W, Y, out_ix\)"):
        asyncio.run(tn.calculate_witness_shares(rt, Dense(), [1]))


# ---- end to end: shares of the inputs -> one proof -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def keys(pn):
    """name -> (qap, prepared key, verikey), the golden keys as tests/test_gpu_trinocchio.py builds them; made once"""
    cache = {}

    def get(name):
        if name not in cache:
            case = _fixture_cases()[name]
            qap, td = _qap(pn, name), _seeded_td(pn, case)
            gen = _gen(pn, td)
            cache[name] = (qap, pn.PreparedKey.generate(td, qap, gen), pn.generate_verikey(td, qap, gen))
        return cache[name]
    return get


@pytest.mark.parametrize("M,t", PARTIES)
@pytest.mark.parametrize("name", ["demo", "larger"])
def test_prove_inputs_end_to_end(pn, tn, keys, name, M, t):
    qap, key, verikey = keys(name)
    r1cs, n_in, inputs, want = _circuit(name)
    xs = SR.share(inputs[0], t, M, random.Random(M))
    hub = RecordingHub(tn, M)
    rts = [tn.Runtime(p, M, t, random.Random(70 + p), hub) for p in range(M)]

    async def main():
        return await asyncio.gather(*(tn.prove_inputs(rts[p], qap, key, xs[p]) for p in range(M)))
    results = asyncio.run(main())
    proof, c_client = results[0]
    for other, oc in results[1:]:
        assert _same(proof, other) and oc == c_client
    assert c_client == [1] + want[0][1:qap.out_ix + 1]
    assert pn.verify(qap, verikey, proof, c_client) == ALL_TRUE
    assert [rt.exchanges for rt in rts] == [pn.ShareSolvePlan(qap, n_in).n_rounds + 4] * M


def test_prove_inputs_refusals(tn, keys):
    qap, key, _ = keys("demo")
    rt = tn.Runtime(0, 3, 1, random.Random(1), tn.LocalHub(3))
    with pytest.raises(ValueError, match="one input vector per proof"):
        asyncio.run(tn.prove_inputs(rt, qap, key, np.zeros((2, 1, 32), np.uint8)))
    with pytest.raises(TypeError, match="PreparedKey"):
        asyncio.run(tn.prove_inputs(rt, qap, {}, [3]))
    assert rt.exchanges == 0
