"""Stall-injection cases for the library's cross-stream ordering points (EXPERIMENTS.md O.3, the inventory table).

A plain script: `python tests/stream_order_cases.py --out FILE` runs every case on the GPU and writes one JSON record
per case (a list) to FILE.  tests/test_gpu_stream_order.py starts it once, as a child process with
GPU_MAX_HW_QUEUES=16 - the queue count the library itself asks for (csrc/api.hip), which the suite's own process
does not run under - and its tests only read the records.

Why a stall: the suite's shapes are tiny, so a producer kernel has long finished when the host enqueues its consumer
on another stream, and a missing wait between the two reads the right bytes anyway.  vmpc_ctx_debug_delay keeps a
stream busy for a requested time; what is enqueued behind it is still pending when the consumer is enqueued.

Three helpers:
  stalled(ctx, usec)   the delay on a context's stream (and the host time it was enqueued at)
  Recorder             wraps Context.wait_for for the length of a case: (call site, waiter, other, other.done()) of
                       every call, read BEFORE the real wait is issued.  done() False: the producer's stream was
                       still busy when its consumer was about to be enqueued - the wait is what makes the answer
                       right.  A read-after-write case that does not see this at its row's site is BLIND and fails.
                       It can also delay the WAITER at a site (write-after-read cases: the consumer runs late, the
                       caller goes on with the same buffers).
  canary(A, B)         is the pair concurrent at all under this queue count?  old bytes in `buf`; A: delay, then
                       new -> buf; B: buf -> snap with NO wait.  snap must be the OLD bytes (plain bytes inside live
                       allocations).  With B.wait_for(A) it must be the new ones.  A pair that reads `new` without
                       the wait is serialised by the runtime (streams sharing a hardware queue run in order) and
                       every case over it would pass whatever the library does: the run fails and names the pair.

Every context is created up front, in a fixed order, before any case runs: streams map onto hardware queues in
creation order (EXPERIMENTS.md R6.7).
"""
import argparse
import hashlib
import json
import os
import random
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

QUEUES = "16"                       # csrc/api.hip vmpc_hw_queues_default, verifiable_mpc_amd/__init__.py
AUX_ORDER = [0, 2, 3, 5, 6, 7, 20, 21, 10, 11]      # creation order of the aux contexts, after the main one
CANARY_US = 1000
HOOK_CAP_US = 20000
# the delay kernel's bounds (csrc/api.hip k_debug_delay): 4 polls per requested microsecond + 64, each under 2048 shader
# clocks, at a shader clock of at least 500 MHz
HOOK_POLLS_PER_US, HOOK_POLLS_EXTRA, HOOK_POLL_CLOCKS, HOOK_MIN_MHZ = 4, 64, 2048, 500

# Delay per case, in microseconds: at least twice the host time measured between enqueuing the stall and the recorded
# wait_for, rounded up to a millisecond (EXPERIMENTS.md O.3 lists both).  A case that is not named here uses DEFAULT_US.
DEFAULT_US = 2000
DELAY_US = {
    "scalar_text_raw": 4000,        # (the first case of the process: 0.75 ms of first-use allocations on the host)
    "batch_check_foreign_forms_raw": 4000,
}


OVERRIDE_US = None                  # --delay-us: one delay for every case (to measure the host times again)


def delay_of(case):
    return OVERRIDE_US or DELAY_US.get(case, DEFAULT_US)


class Env:
    """the contexts of this process, by name, and what the cases share"""

    def __init__(self):
        import verifiable_mpc_amd as vm
        from verifiable_mpc_amd import _native, device
        self.vm, self.native = vm, _native
        self.main = vm.get_context()
        self.ctxs = {"main": self.main}
        for i in AUX_ORDER:
            self.ctxs[f"aux{i}"] = device.get_aux_context(i)
        # the shared bucket stream of a pipeline (vmpc_stream_create), and a context that runs ON it: the canary's
        # copies need a context
        self.bucket = _native.SharedStream(self.main.device, -1)
        self.on_bucket = _native.Context(self.main.device)
        self.on_bucket.set_stream(self.bucket.handle.value)
        self.ctxs["bucket"] = self.on_bucket
        self.names = {c.handle.value: n for n, c in self.ctxs.items()}
        self.stall_t = None

    def name(self, ctx):
        return self.names.get(ctx.handle.value, "ctx@%x" % ctx.handle.value)

    def sync_all(self):
        for c in self.ctxs.values():
            c.sync()

    def stalled(self, ctx, usec):
        self.stall_t = time.perf_counter()
        ctx.debug_delay(usec)


def site_of(frame):
    return f"{os.path.basename(frame.f_code.co_filename)}:{frame.f_code.co_name}"


class Recorder:
    """Context.wait_for wrapped for the length of a `with` block; delay_waiter: {site: microseconds} - a delay enqueued
    on the WAITER's stream right before the real wait at that site (the consumer then runs late)"""

    def __init__(self, env, delay_waiter=None):
        self.env, self.calls, self.delay_waiter = env, [], dict(delay_waiter or {})

    def __enter__(self):
        cls = self.env.native.Context
        self.orig = orig = cls.wait_for
        rec = self

        def wait_for(ctx, other):
            frame = sys._getframe(1)
            site = site_of(frame)
            done = other.done()
            now = time.perf_counter()
            rec.calls.append({"site": site, "line": frame.f_lineno, "waiter": rec.env.name(ctx),
                              "other": rec.env.name(other), "done": bool(done),
                              "host_us": None if rec.env.stall_t is None else round((now - rec.env.stall_t) * 1e6, 1)})
            if site in rec.delay_waiter:
                ctx.debug_delay(rec.delay_waiter[site])
            return orig(ctx, other)
        cls.wait_for = wait_for
        return self

    def __exit__(self, *exc):
        self.env.native.Context.wait_for = self.orig
        return False

    def at(self, site, waiter=None, other=None):
        return [c for c in self.calls if c["site"] == site and (waiter is None or c["waiter"] == waiter)
                and (other is None or c["other"] == other)]


class Blind(AssertionError):
    pass


def need_busy(rec, site, waiter=None, other=None):
    """the row's wait_for saw its producer still busy; returns the host time (microseconds since the stall)"""
    calls = rec.at(site, waiter, other)
    if not calls:
        raise Blind(f"no wait_for recorded at {site} ({waiter} <- {other}): the case does not take that path")
    # (host_us None: a wait issued before the case's stall - busy with the library's own earlier work)
    busy = [c for c in calls if not c["done"] and c["host_us"] is not None]
    if not busy:
        raise Blind(f"{site}: the producer's stream had drained at every wait_for ({calls}) - the stall was spent "
                    "before the consumer was enqueued, the case proves nothing")
    return busy[0]["host_us"]


class patched:
    """setattr for the length of a `with` block"""

    def __init__(self, obj, name, value):
        self.obj, self.name, self.value = obj, name, value

    def __enter__(self):
        self.old = getattr(self.obj, self.name)
        setattr(self.obj, self.name, self.value)

    def __exit__(self, *exc):
        setattr(self.obj, self.name, self.old)
        return False


def stall_before(env, obj, name, pick_ctx, usec, times=1):
    """`obj.name` patched so that its first `times` calls enqueue the delay on pick_ctx(*args) before they run: the
    stall right in front of a producer that sits deep inside a library call"""
    orig = getattr(obj, name)
    left = [times]

    def wrapper(*args, **kw):
        if left[0] > 0:
            left[0] -= 1
            env.stalled(pick_ctx(*args, **kw), usec)
        return orig(*args, **kw)
    return patched(obj, name, wrapper)


# ---- the canary and the hook's own check ------------------------------------------------------------------------------

CANARY_PAIRS = [("main", "aux2"), ("main", "aux0"), ("main", "aux5"), ("main", "aux6"), ("main", "aux7"),
                ("aux7", "main"), ("aux5", "main"), ("aux6", "main"), ("main", "aux10"), ("main", "aux11"),
                ("main", "aux20"), ("main", "aux21"), ("aux3", "main"), ("main", "bucket"), ("bucket", "main")]


def canary(env, a_name, b_name):
    import numpy as np
    A, B = env.ctxs[a_name], env.ctxs[b_name]
    n = 4096
    old, new = np.full(n, 0x5a, np.uint8), np.full(n, 0xc3, np.uint8)
    buf, src, snap = A.alloc(n), A.upload(new), B.alloc(n)
    out = {}
    for with_wait in (False, True):
        A.upload_into(buf.ptr, old)
        B.upload_into(snap.ptr, np.zeros(n, np.uint8))
        A.sync()
        B.sync()
        A.debug_delay(CANARY_US)
        A.copy(buf.ptr, src.ptr, n)
        if with_wait:
            B.wait_for(A)
        B.copy(snap.ptr, buf.ptr, n)
        A.sync()
        B.sync()
        got = B.download(snap.ptr, n)
        out["with_wait" if with_wait else "no_wait"] = \
            "old" if (got == old).all() else "new" if (got == new).all() else "mixed"
    assert out["with_wait"] == "new", f"canary {a_name}->{b_name}: with the wait the copy read {out['with_wait']} bytes"
    assert out["no_wait"] == "old", (
        f"HARNESS CONDITION, not a finding about the library: the streams of {a_name} and {b_name} are serialised by the "
        f"runtime under GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} (without a wait {b_name}'s copy read "
        f"{out['no_wait']} bytes): every case over this pair is blind")
    return out


def hook_timing(env, name):
    """a 2000-us delay timed with HIP events (ctx.profile): at least the requested time, at most the kernel's poll bound
    converted to time - a property of the code (csrc/api.hip), not a measurement"""
    ctx, usec = env.main, 2000
    ctx.sync()
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        ctx.debug_delay(usec)
        ctx.sync()
        ms, launches = ctx.profile_read(reset=True)["debug_delay"]
    finally:
        ctx.profile(False)
    upper_ms = (HOOK_POLLS_PER_US * usec + HOOK_POLLS_EXTRA) * HOOK_POLL_CLOCKS / HOOK_MIN_MHZ / 1000.0
    print(f"hook_timing: {usec} us requested, {ms:.3f} ms measured, bound {upper_ms:.1f} ms", flush=True)
    assert launches == 1
    assert ms >= usec / 1000.0, f"a {usec}-us delay took {ms} ms"
    assert ms <= upper_ms, f"a {usec}-us delay took {ms} ms, above its poll bound of {upper_ms} ms"
    return {"requested_us": usec, "measured_ms": ms, "upper_ms": upper_ms}


def hook_range(env, name):
    native, ctx = env.native, env.main
    ctx.sync()
    for call in (lambda us: ctx.debug_delay(us), lambda us: env.bucket.debug_delay(us)):
        call(0)
        assert ctx.done() and env.on_bucket.done()           # 0: VMPC_OK and nothing launched
        try:
            call(HOOK_CAP_US + 1)
        except native.VmpcError as e:
            assert e.code == native.E_RANGE, e
        else:
            raise AssertionError("a delay above the cap was accepted")
        assert ctx.done() and env.on_bucket.done()           # above the cap: nothing launched
        t0 = time.perf_counter()
        call(HOOK_CAP_US)                                    # the cap itself is served
        env.main.sync()
        env.on_bucket.sync()
        assert time.perf_counter() - t0 >= HOOK_CAP_US * 1e-6
    return {}


# ---- shared inputs ---------------------------------------------------------------------------------------------------

_SHARED = {}


def shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def ell():
    from oracle import ed25519_ref as ed
    return ed.ELL


def rand_scalars(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(ell()) for _ in range(n)]


def points_300(env):
    """300 generators g_i = e_i * B as the C oracle makes them, (n, 64) affine bytes + the device vector"""
    def make():
        import numpy as np
        from oracle import c_oracle
        vm = env.vm
        ex = c_oracle.scalars_to_array(rand_scalars(71, 300))
        base = np.frombuffer(vm.Ed25519Point.generator.to_proj_bytes(), np.uint8)
        _, aff = c_oracle.fixed_base(base, ex)
        return aff, vm.PointVector.from_affine_array(aff, keep_proj=True)
    return shared("points_300", make)


def oracle_commitment(scalars, aff):
    """<scalars, points> as affine bytes, by the C restatement of the reference algorithm"""
    import numpy as np
    from oracle import c_oracle
    _, want = c_oracle.vector_commitment(c_oracle.scalars_to_array(scalars), np.zeros(32, np.uint8), aff, aff[0])
    return bytes(want)


def golden_n1023():
    def make():
        with open(os.path.join(ROOT, "tests", "golden", "ac20_ed25519_n1023.json")) as f:
            return json.load(f)
    return shared("golden_n1023", make)


h2i = lambda s: int(s, 16)
hx = lambda v: format(int(v), "x")


def n1023_setup(env, precompute):
    """generators, statement and masks of the reference-made N = 1024 fixture (tests/test_gpu_protocol.py
    test_protocol5_n1023_device_mode), on the device"""
    vm, case = env.vm, golden_n1023()
    group = vm.EllipticCurve("Ed25519", "projective")
    h = vm.circuit_sat.as_point(group.generator)
    g = vm.PointVector.fixed_base(h, [h2i(v) for v in case["gen_exponents"]])
    k = vm.Ed25519Point.repeat(h, h2i(case["gen_exponent_k"]))
    if precompute:
        g.precompute([h, k])
    gens = {"g": g, "h": h, "k": k}
    gf = vm.GF(group.order)
    x = vm.ScalarVector.from_ints([h2i(v) for v in case["x"]])
    L = vm.pivot.LinearForm(vm.ScalarVector.from_ints([h2i(v) for v in case["L"]]))
    gamma, y = h2i(case["gamma"]), gf(h2i(case["y"]))
    P = vm.Ed25519Point((h2i(case["P"][0]), h2i(case["P"][1]), 1))
    return gens, gf, x, L, gamma, y, P


def n1023_prove_and_check(env, gens, gf, x, L, gamma, y, P):
    """protocol_5_prover on the fixture's inputs; the proof and every Fiat-Shamir challenge against the reference's"""
    vm, case = env.vm, golden_n1023()
    hashes = []
    orig, orig_v = vm.pivot.fiat_shamir_hash, vm.pivot.fiat_shamir_hash_variants

    def one(input_list, order):
        hashes.append(orig(input_list, order))
        return hashes[-1]

    def many(common, tails, order):
        cs = orig_v(common, tails, order)
        hashes.extend(cs)
        return cs
    with patched(vm.pivot, "fiat_shamir_hash", one), patched(vm.pivot, "fiat_shamir_hash_variants", many):
        proof = vm.compressed_pivot.protocol_5_prover(gens, P, L, y, x, gamma, gf, r=[h2i(v) for v in case["r"]],
                                                      rho=h2i(case["rho"]))
    pr = case["proof"]
    aff = lambda pt: [hx(c) for c in pt.normalize().coords[:2]]
    assert hx(int(proof["t"]) % ell()) == pr["t"]
    assert aff(proof["A"]) == pr["A"]
    for i in range(case["rounds"]):
        assert aff(proof[f"A{i}"]) == pr["A_i"][i], f"A{i}"
        assert aff(proof[f"B{i}"]) == pr["B_i"][i], f"B{i}"
    assert [hx(int(v) % ell()) for v in proof["z_prime"]] == pr["z_prime"]
    assert [hx(c) for c in hashes] == [h["c"] for h in case["hashes"]]
    return proof


# ---- the cases -------------------------------------------------------------------------------------------------------
# Each returns a dict that goes into the case's record; `host_us` is the host time between the stall and the row's
# wait_for.  A case fails by raising.

def scalar_text_raw(env, name):
    """device.py ScalarVector.text_begin: main (k_fr_axpy writes the vector) -> aux2 (formatter reads it)"""
    from oracle import ed25519_ref as ed
    vm, n, c = env.vm, 300, 12345678901234567890
    a, b = rand_scalars(1, n), rand_scalars(2, n)
    va, vb = vm.ScalarVector.from_ints(a), vm.ScalarVector.from_ints(b)
    want = "".join(ed.scalar_repr((c * x + y) % ell()) + ", " for x, y in zip(a, b))
    with Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        w = va.axpy(c, vb)
        w.text_begin()
        got = bytes(w.text()).decode()
    host_us = need_busy(rec, "device.py:text_begin", "aux2", "main")
    assert got == want
    return {"host_us": host_us, "waits": rec.calls}


def scalar_text_war(env, name):
    """... and write after read: the formatter runs late, the caller drops the vector and goes on allocating and
    writing vectors of the same size class on the main stream"""
    from oracle import ed25519_ref as ed
    vm, n, c = env.vm, 300, 987654321
    a, b = rand_scalars(3, n), rand_scalars(4, n)
    va, vb = vm.ScalarVector.from_ints(a), vm.ScalarVector.from_ints(b)
    want = "".join(ed.scalar_repr((c * x + y) % ell()) + ", " for x, y in zip(a, b))
    with Recorder(env, delay_waiter={"device.py:text_begin": delay_of(name)}) as rec:
        w = va.axpy(c, vb)
        w.text_begin()
        pend = w._pending_text[1]
        del w                                   # the text keeps the vector's block alive (PendingText.keepalive)
        others = [va.scale(7 + i) for i in range(4)]            # same size class: would reuse a released block
        got = bytes(pend.result()).decode()
        again = [o.to_ints() for o in others]
    assert rec.at("device.py:text_begin")
    assert got == want
    assert again == [[(7 + i) * x % ell() for x in a] for i in range(4)]
    return {"waits": rec.calls}


def _fold_inputs(env, n):
    aff, g = points_300(env)
    assert 2 * n <= len(g)
    return g[:n], g[n:2 * n]


def point_text_raw(env, name):
    """device.py PointVector.text_begin (through fold(stream_text=True), not sliced): main (k_fold writes X:Y:Z) ->
    aux2 (formatter); the restatement is the plain fold formatted synchronously, as tests/test_gpu_formats.py has it"""
    n, c = 130, 0x1234567890abcdef1234567890abcdef
    gl, gr = _fold_inputs(env, n)
    plain = gl.fold(gr, c)
    want, want_aff = bytes(plain.text()), plain.affine_array().tobytes()
    with Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        out = gl.fold(gr, c, stream_text=True)
        got = bytes(out.text())
    host_us = need_busy(rec, "device.py:text_begin", "aux2", "main")
    assert got == want and out.affine_array().tobytes() == want_aff
    return {"host_us": host_us, "waits": rec.calls}


def point_text_war(env, name):
    n, c = 130, 0xfedcba9876543210
    gl, gr = _fold_inputs(env, n)
    plain = gl.fold(gr, c)
    want = bytes(plain.text())
    with Recorder(env, delay_waiter={"device.py:text_begin": delay_of(name)}) as rec:
        out = gl.fold(gr, c, stream_text=True)
        pend = out._pending_text[1]
        del out                                 # the next round's vector replaces it
        nxt = gl.fold(gr, c + 1)                # same size classes on the main stream
        got = bytes(pend.result())
        nxt_text = bytes(nxt.text())
    assert rec.at("device.py:text_begin")
    assert got == want
    assert nxt_text == bytes(gl.fold(gr, c + 1).text())
    return {"waits": rec.calls}


def _sliced(env):
    """the smallest sliced fold: TEXT_SLICE 64 -> with a co-runner (after_first) folds of 128 elements or more are
    sliced, first slice 16, then slices of 64 (device.py fold: sliced_from = 2 * TEXT_SLICE, step = TEXT_SLICE // 4)"""
    return patched(env.vm.PointVector, "TEXT_SLICE", 64)


def fold_sliced_text_raw(env, name):
    """device.py fold, sliced, with after_first: every slice's fold on main -> its formatter on aux2"""
    n, c = 150, 0x0123456789abcdef0123456789abcdef0123
    gl, gr = _fold_inputs(env, n)
    plain = gl.fold(gr, c)
    want, want_aff = bytes(plain.text())[:-2], plain.affine_array().tobytes()
    seen = []
    with _sliced(env), Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        out = gl.fold(gr, c, stream_text=True, after_first=seen.append)
        parts = len(out._pending_text[1].parts)
        got = b"".join(bytes(p) for p in out.text_chunks())
    assert parts == 4 and seen == [True], (parts, seen)        # 16 + 64 + 64 + 6
    calls = rec.at("device.py:fold", "aux2", "main")
    assert len(calls) == parts
    host_us = need_busy(rec, "device.py:fold", "aux2", "main")
    assert not calls[-1]["done"], "the LAST slice's wait found the main stream drained"
    assert got == want and out.affine_array().tobytes() == want_aff
    return {"host_us": calls[-1]["host_us"], "first_wait_us": host_us, "waits": rec.calls}


def fold_sliced_text_war(env, name):
    n, c = 150, 0xabcdef
    gl, gr = _fold_inputs(env, n)
    want = bytes(gl.fold(gr, c).text())[:-2]
    want_next = bytes(gl.fold(gr, c + 2).text())[:-2]
    with _sliced(env), Recorder(env, delay_waiter={"device.py:fold": delay_of(name) // 4}) as rec:
        out = gl.fold(gr, c, stream_text=True, after_first=lambda more: None)
        seq = out._pending_text[1]
        del out
        nxt = gl.fold(gr, c + 2, stream_text=True, after_first=lambda more: None)      # the next round's fold
        got = b"".join(bytes(p) for p in seq.chunks(trim=2))
        got_next = b"".join(bytes(p) for p in nxt.text_chunks())
    assert len(rec.at("device.py:fold")) == 8
    assert got == want and got_next == want_next
    return {"waits": rec.calls}


def leaves_hash_raw(env, name):
    """compressed_pivot.py _form_digest_begin: main (k_fr_scale writes the coefficients) -> aux2 (sha256 leaves)"""
    vm, cp = env.vm, env.vm.compressed_pivot
    n, c = 300, 31337                   # 9600 bytes: three leaves, the last one short
    a = rand_scalars(5, n)
    va = vm.ScalarVector.from_ints(a)
    data = b"".join(((c * x) % ell()).to_bytes(32, "little") for x in a)
    want = cp._chunked_digest(b"vmpc-ac20/form/v1", data)
    with Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        L = vm.pivot.LinearForm(va.scale(c))
        cp._form_digest_begin(L)
        got = cp._form_digest(L)
    host_us = need_busy(rec, "compressed_pivot.py:_form_digest_begin", "aux2", "main")
    assert got == want
    return {"host_us": host_us, "waits": rec.calls}


def leaves_hash_war(env, name):
    vm, cp = env.vm, env.vm.compressed_pivot
    n, c = 300, 4242
    a = rand_scalars(6, n)
    va = vm.ScalarVector.from_ints(a)
    data = b"".join(((c * x) % ell()).to_bytes(32, "little") for x in a)
    want = cp._chunked_digest(b"vmpc-ac20/form/v1", data)
    with Recorder(env, delay_waiter={"compressed_pivot.py:_form_digest_begin": delay_of(name)}) as rec:
        L = vm.pivot.LinearForm(va.scale(c))
        cp._form_digest_begin(L)
        pending, L._pending_leaves = L._pending_leaves, None
        del L                               # the digest in flight keeps the coefficients alive (keepalive)
        others = [va.scale(9 + i) for i in range(4)]
        leaves = pending.result()
        again = [o.to_ints() for o in others]
    got = hashlib.sha256(b"vmpc-ac20/form/v1" + (32 * n).to_bytes(8, "little") + leaves).digest()
    assert rec.at("compressed_pivot.py:_form_digest_begin")
    assert got == want
    assert again == [[(9 + i) * x % ell() for x in a] for i in range(4)]
    return {"waits": rec.calls}


def commitment_pair_raw(env, name):
    """pivot.py vector_commitment_pair over an untabulated vector: main (k_fr_scale writes both scalar vectors) ->
    aux0 (the second commitment's recoding reads x_b)"""
    vm = env.vm
    aff, g = points_300(env)
    n, ca, cb = 300, 1000003, 1000033
    a, b = rand_scalars(7, n), rand_scalars(8, n)
    va, vb = vm.ScalarVector.from_ints(a), vm.ScalarVector.from_ints(b)
    want = (oracle_commitment([ca * x % ell() for x in a], aff), oracle_commitment([cb * x % ell() for x in b], aff))
    h = vm.Ed25519Point.generator
    with Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        xa, xb = va.scale(ca), vb.scale(cb)
        A, B = vm.pivot.vector_commitment_pair(xa, 0, g, xb, 0, g, h)
    host_us = need_busy(rec, "pivot.py:vector_commitment_pair", "aux0", "main")
    assert (A.to_affine_bytes(), B.to_affine_bytes()) == want
    return {"host_us": host_us, "waits": rec.calls}


def commitment_pair_war(env, name):
    vm = env.vm
    aff, g = points_300(env)
    n = 300
    a, b = rand_scalars(9, n), rand_scalars(10, n)
    h = vm.Ed25519Point.generator
    want = [(oracle_commitment([(3 + i) * x % ell() for x in a], aff),
             oracle_commitment([(5 + i) * x % ell() for x in b], aff)) for i in range(2)]
    va, vb = vm.ScalarVector.from_ints(a), vm.ScalarVector.from_ints(b)
    got = []
    with Recorder(env, delay_waiter={"pivot.py:vector_commitment_pair": delay_of(name)}) as rec:
        for i in range(2):                                  # the next round's pair with fresh vectors, same sizes
            A, B = vm.pivot.vector_commitment_pair(va.scale(3 + i), 0, g, vb.scale(5 + i), 0, g, h)
            got.append((A.to_affine_bytes(), B.to_affine_bytes()))
    assert len(rec.at("pivot.py:vector_commitment_pair")) == 2
    assert got == want
    return {"waits": rec.calls}


def p5_plain_pairs_raw(env, name):
    """the N = 1024 reference-transcript proof over an UNTABULATED CRS: every round's pair through
    vector_commitment_pair (aux0), every text through aux2; the stall sits in front of the fold of the witness
    (ScalarVector.axpy, main) that produces the next round's z_l, z_r"""
    vm = env.vm
    args = n1023_setup(env, precompute=False)
    with patched(vm.pivot, "AUTO_TABLE_MIN", 1 << 30), Recorder(env) as rec, \
            stall_before(env, vm.ScalarVector, "axpy", lambda self, *a: self.ctx, delay_of(name), times=2):
        n1023_prove_and_check(env, *args)
    host_us = need_busy(rec, "pivot.py:vector_commitment_pair", "aux0", "main")
    text_us = need_busy(rec, "device.py:text_begin", "aux2", "main")
    return {"host_us": host_us, "text_begin_host_us": text_us, "waits": rec.calls}


def _table_rounds(env):
    """the round context from 32-element rounds up, on aux 7 (tests/test_gpu_protocol.py's "table_rounds")"""
    return patched(env.vm.compressed_pivot, "REF_TABLE_PAIR_MIN", 16)


def p5_table_rounds_war(env, name):
    """compressed_pivot.py _ref_table_rounds (aux7 <- main) and the round hook (main <- aux7), consumers late: the
    round context copies z_hat and L~ late, the fold's later slices start late; the proof and every challenge are
    the reference's"""
    vm = env.vm
    args = n1023_setup(env, precompute=True)
    d = delay_of(name)
    with _table_rounds(env), _sliced(env), \
            Recorder(env, delay_waiter={"compressed_pivot.py:_ref_table_rounds": d, "compressed_pivot.py:hook": d // 4,
                                        "device.py:fold": d // 8}) as rec:
        n1023_prove_and_check(env, *args)
    assert rec.at("compressed_pivot.py:_ref_table_rounds", "aux7", "main")
    assert rec.at("compressed_pivot.py:hook", "main", "aux7")
    return {"waits": rec.calls}


def p5_round_hook_raw(env, name):
    """compressed_pivot.py round hook: aux7 (the round's pair, round_begin) -> main (the exact fold's later slices are
    ordered behind it); the stall sits in front of round_begin on aux7"""
    vm = env.vm
    args = n1023_setup(env, precompute=True)
    with _table_rounds(env), _sliced(env), Recorder(env) as rec, \
            stall_before(env, env.native.P4Rounds, "round_begin", lambda self, *a: self.ctx, delay_of(name), times=1):
        n1023_prove_and_check(env, *args)
    host_us = need_busy(rec, "compressed_pivot.py:hook", "main", "aux7")
    return {"host_us": host_us, "waits": rec.calls}


def p5_early_pair_raw(env, name):
    """compressed_pivot.py _early_pair_prepare (aux5, aux6 <- main: the scaled halves of the folded witness) and
    _early_pair_launch (main <- aux5, aux6); the stall sits on main in front of the scalars"""
    vm, cp = env.vm, env.vm.compressed_pivot
    args = n1023_setup(env, precompute=False)
    with patched(cp, "EARLY_PAIR_MIN", 64), patched(vm.pivot, "AUTO_TABLE_MIN", 1 << 30), Recorder(env) as rec, \
            stall_before(env, cp, "_early_pair_prepare", lambda main, *a: main, delay_of(name), times=1):
        n1023_prove_and_check(env, *args)
    host_us = max(need_busy(rec, "compressed_pivot.py:_early_pair_prepare", "aux5", "main"),
                  need_busy(rec, "compressed_pivot.py:_early_pair_prepare", "aux6", "main"))
    # (main <- aux5, aux6 orders the FOLD behind the four commitments: scheduling, the fold reads nothing of theirs)
    assert rec.at("compressed_pivot.py:_early_pair_launch", "main", "aux5")
    assert rec.at("compressed_pivot.py:_early_pair_launch", "main", "aux6")
    return {"host_us": host_us, "waits": rec.calls}


def p5_early_pair_war(env, name):
    vm, cp = env.vm, env.vm.compressed_pivot
    args = n1023_setup(env, precompute=False)
    d = delay_of(name)
    with patched(cp, "EARLY_PAIR_MIN", 64), patched(vm.pivot, "AUTO_TABLE_MIN", 1 << 30), \
            Recorder(env, delay_waiter={"compressed_pivot.py:_early_pair_prepare": d // 2}) as rec:
        n1023_prove_and_check(env, *args)
    assert rec.at("compressed_pivot.py:_early_pair_prepare")
    return {"waits": rec.calls}


def batch_check_foreign_forms_raw(env, name):
    """compressed_pivot.py _batch_check: forms whose coefficients live on another context (aux3 here) -> main
    (k_fr_batch_products reads them).  Through protocol_5_verifier_batch the forms' digests are collected first and
    that drains the foreign stream (a blocking copy), so the stall goes right in front of the combined check: the
    coefficients are re-made on the stalled foreign stream."""
    vm, cp = env.vm, env.vm.compressed_pivot
    n, K = 15, 2
    rng = random.Random(88)
    foreign = env.ctxs["aux3"]
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    gens = {"g": vm.PointVector.fixed_base(group.generator, [rng.randrange(1, ell()) for _ in range(n)], keep_proj=False),
            "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, rng.randrange(1, ell()))}
    # statements as tests/test_gpu_batch_verify.py makes them (the single verifier is the restatement), the forms'
    # coefficients - halved here, doubled again on the device below - on the foreign context
    statements = []
    for p in range(K):
        x = vm.ScalarVector.from_ints([rng.randrange(ell()) for _ in range(n)])
        coeffs = [rng.randrange(ell()) for _ in range(n)]
        L = vm.pivot.LinearForm(vm.ScalarVector.from_ints(coeffs))
        gamma = rng.randrange(1, ell())
        P = vm.pivot.vector_commitment(x, gamma, gens["g"], gens["h"])
        y = gf(L(x))
        proof = cp.protocol_5_prover(gens, P, L, y, x, gamma, gf, transcript="compact")
        assert cp.protocol_5_verifier(gens, P, L, y, proof, gf, transcript="compact") is True
        half = vm.ScalarVector.from_ints([c * pow(2, -1, ell()) % ell() for c in coeffs], foreign)
        statements.append((P, half, y, proof))
    weights = [rng.randrange(1, 1 << 128) for _ in range(K)]
    orig = cp._batch_check
    seen = []

    def check(items, ws, g_hat, k, order):
        for it in items:                     # the same coefficients, produced NOW on the stalled foreign stream
            env.stalled(foreign, delay_of(name))
            it.coeffs = it.coeffs.scale(1)
        seen.append(orig(items, ws, g_hat, k, order))
        return seen[-1]
    with Recorder(env) as rec, patched(cp, "_batch_check", check):
        stmts = [(P, vm.pivot.LinearForm(half.scale(2)), y, proof) for P, half, y, proof in statements]
        got = cp.protocol_5_verifier_batch(gens, stmts, gf, transcript="compact", weights=weights)
    host_us = need_busy(rec, "compressed_pivot.py:_batch_check", "main", "aux3")
    assert got == [True] * K and seen == [True]
    # ... and a wrong statement is still refused
    bad = [(P, vm.pivot.LinearForm(half.scale(2)), y + (1 if i == 1 else 0), proof)
           for i, (P, half, y, proof) in enumerate(statements)]
    assert cp.protocol_5_verifier_batch(gens, bad, gf, transcript="compact", weights=weights) == [True, False]
    return {"host_us": host_us, "waits": rec.calls}


def sharded_partial_raw(env, name):
    """sharded.py DeviceOps.partial with a stream index: main (k_fr_scale writes the block's scalars) -> aux0 (the
    block's table commitment)"""
    import numpy as np
    vm = env.vm
    from verifiable_mpc_amd import sharded
    aff, g = points_300(env)
    n, c = 300, 777
    a = rand_scalars(11, n)
    block = shared("block_300", lambda: vm.PointVector.from_affine_array(aff).precompute([vm.Ed25519Point.generator],
                                                                                          rows=16))
    ops = sharded.DeviceOps(env.main)
    va = vm.ScalarVector.from_ints(a)
    want = oracle_commitment([c * x % ell() for x in a], aff)
    out = env.main.alloc(128)
    with Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        v = va.scale(c)
        ctx, keep = ops.partial(block, v, None, out.ptr, 1)
        ctx.sync()
    host_us = need_busy(rec, "sharded.py:partial", "aux0", "main")
    raw = env.main.download(out.ptr, 128).tobytes()
    assert vm.Ed25519Point.from_proj_bytes(raw[:96]).to_affine_bytes() == want
    return {"host_us": host_us, "waits": rec.calls}


def hipbackend_slots_raw(env, name):
    """parallel.py HipBackend: main (k_fr_scale writes the scalars) -> the slot contexts aux10, aux11, per launch
    (launch_partial) and once for a pipelined driver (inputs_ready)"""
    vm = env.vm
    from verifiable_mpc_amd import parallel
    aff, g = points_300(env)
    n = 300
    a = rand_scalars(12, n)
    va = vm.ScalarVector.from_ints(a)
    be = parallel.HipBackend(env.main, torch=None, n_slots=3)
    assert [env.name(c) for c in be.ctxs] == ["main", "aux10", "aux11"]
    want = [oracle_commitment([(11 + s) * x % ell() for x in a], aff) for s in range(4)]
    for slot in (1, 2):                     # once without a stall: a slot's first commitment sizes its workspace, and
        be.launch_partial(va, g, slot, True)        # growing one synchronises the slot's stream (the host would sit
        be.wait(slot)                               # out the stall there)
    with Recorder(env) as rec:
        env.stalled(env.main, delay_of(name))
        vs = [va.scale(11 + s) for s in range(4)]
        be.launch_partial(vs[1], g, 1, True)
        be.launch_partial(vs[2], g, 2, True)
        got = [None, be.affine_result(1).to_affine_bytes(), be.affine_result(2).to_affine_bytes()]
    host_us = max(need_busy(rec, "parallel.py:launch_partial", "aux10", "main"),
                  need_busy(rec, "parallel.py:launch_partial", "aux11", "main"))
    assert got[1:] == want[1:3]
    with Recorder(env) as rec2:
        env.stalled(env.main, delay_of(name))
        v3 = va.scale(14)
        be.pipelined = True                 # -> inputs_ready(): every slot ordered behind the main stream once
        be.launch_partial(v3, g, 2, True)
        got3 = be.affine_result(2).to_affine_bytes()
        be.pipelined = False
    need_busy(rec2, "parallel.py:inputs_ready", "aux11", "main")
    assert not rec2.at("parallel.py:launch_partial")
    assert got3 == want[3]
    return {"host_us": host_us, "waits": rec.calls + rec2.calls}


def bucket_stream(env, name):
    """vmpc_ctx_set_bucket_stream: the commitment's bucket stage on the shared stream, ordered by ev_sorted /
    ev_bucketed (csrc/msm.hip).  The delay on the bucket stream (the bucket kernel starts late: the reduction on the
    context's stream must wait for it), then on the context's stream (the sort is late: the bucket kernel must wait)"""
    vm = env.vm
    aff, g = points_300(env)
    n = 300
    ctx = env.main
    a = rand_scalars(13, n)
    va = vm.ScalarVector.from_ints(a)
    want = oracle_commitment(a, aff)
    out = ctx.alloc(128)
    pending = {}
    ctx.set_bucket_stream(env.bucket, 2)
    try:
        for where in ("bucket", "ctx", "both"):
            env.sync_all()
            if where in ("bucket", "both"):
                env.bucket.debug_delay(delay_of(name))
            if where in ("ctx", "both"):
                env.stalled(ctx, delay_of(name))
            ctx.on_general_path(lambda: ctx.msm(va.ptr, g.affine_ptr, n, None, None, 0, out.ptr, None))
            pending[where] = not ctx.done()
            ctx.sync()
            raw = ctx.download(out.ptr, 128).tobytes()
            assert vm.Ed25519Point.from_proj_bytes(raw[:96]).to_affine_bytes() == want, where
    finally:
        ctx.set_bucket_stream(None, 0)
    assert all(pending.values()), pending       # the call returned with its work still queued behind the stall
    return {"pending_when_enqueued": pending}


def chunked_format(env, name):
    """vmpc_format_*_chunked_dev: the delay on the formatter's own stream before the call - the pieces' landed count
    (stream writes between the chunk copies) must not run ahead of the copies"""
    vm = env.vm
    side = env.ctxs["aux2"]
    n = 300
    a = rand_scalars(14, n)
    va = vm.ScalarVector.from_ints(a)
    aff, g = points_300(env)
    want_s, want_p = bytes(va.text())[:-2], bytes(g.text())[:-2]
    with patched(env.native.Context, "TEXT_CHUNK_BYTES", 4096):
        env.sync_all()
        env.stalled(side, delay_of(name))
        ps = side.format_begin("scalars", va.ptr, n, vm.formats.scalar_signed(), keepalive=va.v.buf, own_signal=True)
        pp = side.format_begin("points", g.p.ptr, n, keepalive=g.p.buf, own_signal=True)
        busy = not side.done()
        assert ps.chunk_bytes == 4096 and ps.n_chunks > 4 and pp.n_chunks > 16
        got_s = b"".join(bytes(p) for p in ps.chunks(trim=2))
        got_p = b"".join(bytes(p) for p in pp.chunks(trim=2))
    assert busy
    assert got_s == want_s and got_p == want_p
    return {"pending_when_enqueued": busy}


def pinocchio_war(env, name):
    """pynocchio.py compute_proof over a PreparedKey with compute_h's HPoly (twice) and the batch form on two witnesses:
    aux20 (twist sum) and aux21 (h sum) <- main.  Their inputs reach the device through blocking uploads on the main stream, which drain a
    stall there before the waits are issued (no read-after-write case: EXPERIMENTS.md O.3); here the consumers run late
    and the caller proves again with the same key.  Against the reference-made proofs of tests/golden/pinocchio_keygen.json."""
    from tests import test_gpu_pinocchio_h as TH
    from verifiable_mpc_amd import pynocchio as pn
    with open(os.path.join(ROOT, "tests", "golden", "pinocchio_keygen.json")) as f:
        case = json.load(f)["cases"][0]
    td = TH._seeded_td(pn, case)
    qap = TH._qaps(pn, case)["r1cs"]
    gen = TH._gen(pn, td)
    c, deltas = TH._case_inputs(case)
    key = pn.PreparedKey.generate(td, qap, gen)
    site = "pynocchio.py:_compute_proof_batch_prepared"       # the one proof assembly: compute_proof is its batch of one
    with Recorder(env, delay_waiter={site: delay_of(name)}) as rec:
        proofs, ends = [], []
        for _ in range(2):
            h = pn.compute_h(qap, c, deltas)
            proofs.append(pn.compute_proof(qap, c, h, key, deltas))
            ends.append(len(rec.calls))
        hs = pn.compute_h_batch(qap, [c, c], [deltas, deltas])
        proofs += pn.compute_proof_batch(qap, [c, c], hs, key, [deltas, deltas])
        ends.append(len(rec.calls))
    for proof in proofs:
        for k, enc in case["proof"].items():
            assert TH._enc(proof[k]) == enc, k
    # per call, whatever K is: aux20 <- main; aux21 <- main (the result buffer) and aux21 <- the context that made h (main)
    for lo, hi in zip([0] + ends, ends):
        waits = [(w["waiter"], w["other"]) for w in rec.calls[lo:hi] if w["site"] == site]
        assert sorted(waits) == [("aux20", "main"), ("aux21", "main"), ("aux21", "main")], waits
    assert len(rec.at(site, "aux20", "main")) == 3 and len(rec.at(site, "aux21")) == 6 and len(rec.at(site)) == 9
    return {"waits": rec.calls}


CASES = [
    ("hook_range", "hook", hook_range),
    ("hook_timing", "hook", hook_timing),
    ("scalar_text_raw", "raw", scalar_text_raw),
    ("scalar_text_war", "war", scalar_text_war),
    ("point_text_raw", "raw", point_text_raw),
    ("point_text_war", "war", point_text_war),
    ("fold_sliced_text_raw", "raw", fold_sliced_text_raw),
    ("fold_sliced_text_war", "war", fold_sliced_text_war),
    ("leaves_hash_raw", "raw", leaves_hash_raw),
    ("leaves_hash_war", "war", leaves_hash_war),
    ("commitment_pair_raw", "raw", commitment_pair_raw),
    ("commitment_pair_war", "war", commitment_pair_war),
    ("p5_plain_pairs_raw", "raw", p5_plain_pairs_raw),
    ("p5_table_rounds_war", "war", p5_table_rounds_war),
    ("p5_round_hook_raw", "raw", p5_round_hook_raw),
    ("p5_early_pair_raw", "raw", p5_early_pair_raw),
    ("p5_early_pair_war", "war", p5_early_pair_war),
    ("batch_check_foreign_forms_raw", "raw", batch_check_foreign_forms_raw),
    ("sharded_partial_raw", "raw", sharded_partial_raw),
    ("hipbackend_slots_raw", "raw", hipbackend_slots_raw),
    ("bucket_stream", "native", bucket_stream),
    ("chunked_format", "native", chunked_format),
    ("pinocchio_war", "war", pinocchio_war),
]
CASE_NAMES = [f"canary_{a}_{b}" for a, b in CANARY_PAIRS] + [name for name, _, _ in CASES]


def run(out_path, only=None):
    assert os.environ.get("GPU_MAX_HW_QUEUES") == QUEUES, "start this script with GPU_MAX_HW_QUEUES=" + QUEUES
    t_start = time.perf_counter()
    env = Env()
    todo = [(f"canary_{a}_{b}", "canary", (lambda e, n, a=a, b=b: canary(e, a, b))) for a, b in CANARY_PAIRS]
    todo += [(name, kind, fn) for name, kind, fn in CASES]
    records, fatal = [], False
    for name, kind, fn in todo:
        if only and name not in only and kind != "canary":
            continue
        rec = {"case": name, "kind": kind, "ok": False, "blind": False, "delay_us": delay_of(name), "error": None}
        t0 = time.perf_counter()
        try:
            env.sync_all()
            env.stall_t = None
            rec.update(fn(env, name) or {})
            env.sync_all()
            rec["ok"] = True
        except Blind as e:
            rec["blind"], rec["error"] = True, str(e)
        except env.native.VmpcError as e:
            rec["error"] = traceback.format_exc()
            fatal = e.code == env.native.E_HIP      # a HIP error: nothing more is started on the GPU
        except Exception:
            rec["error"] = traceback.format_exc()
        rec["wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        records.append(rec)
        print(f"{name}: {'ok' if rec['ok'] else 'FAILED'} {rec['wall_ms']} ms host_us={rec.get('host_us')}", flush=True)
        if rec["error"]:
            print(rec["error"], flush=True)
        if fatal:
            break
        if not rec["ok"]:
            try:
                env.sync_all()                      # a failed case leaves nothing queued for the next one
            except Exception:
                fatal = True
                break
    total = round(time.perf_counter() - t_start, 3)
    with open(out_path, "w") as f:
        json.dump({"queues": os.environ.get("GPU_MAX_HW_QUEUES"), "wall_s": total, "records": records}, f, indent=1)
    print(f"{len(records)} cases in {total} s", flush=True)
    return 3 if fatal else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--delay-us", type=int)
    a = ap.parse_args()
    OVERRIDE_US = a.delay_us
    sys.exit(run(a.out, a.only))
