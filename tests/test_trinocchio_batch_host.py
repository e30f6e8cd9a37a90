"""What the batch M-party prover decides on the host (trinocchio.prove_batch, prove_inputs_batch,
pynocchio.compute_h_share_batch), without a GPU: the refusals that need no device are raised
before any context is asked for, the batch is cut where compute_h_batch cuts it, and the two new entries are declared,
bound and exported."""
import asyncio
import random
import types

import numpy as np
import pytest

from tests import h_ref as H


@pytest.fixture(scope="module")
def pn():
    from verifiable_mpc_amd import build
    build.build(verbose=False)
    from verifiable_mpc_amd import pynocchio
    return pynocchio


@pytest.fixture(scope="module")
def tn(pn):
    from verifiable_mpc_amd import trinocchio
    return trinocchio


@pytest.fixture()
def no_context(pn, tn, monkeypatch):
    """any request for a device context fails the test"""
    def refuse(*a, **kw):
        raise AssertionError("a device context was asked for")
    import verifiable_mpc_amd.device as device
    monkeypatch.setattr(pn, "get_context", refuse)
    monkeypatch.setattr(device, "get_context", refuse)
    monkeypatch.setattr(tn, "get_context", refuse)


def _qap(pn, d=3):
    V, W, Y, out_ix, m, c = H.satisfiable_r1cs(d, seed=d)
    return pn.R1CSQAP(H.csr_arrays(V), H.csr_arrays(W), H.csr_arrays(Y), out_ix, m=m), c


def _key(pn):
    return object.__new__(pn.PreparedKey)           # passes the type check; nothing of it may be touched


def test_key_must_be_prepared(pn, tn, no_context):
    qap, c = _qap(pn)
    rt = tn.Runtime(0, 3, 1, random.Random(1), tn.LocalHub(3))
    arr = np.zeros((2, qap.m + 1, 32), np.uint8)
    with pytest.raises(TypeError, match="PreparedKey"):
        asyncio.run(tn.prove_batch(rt, qap, {}, arr))
    with pytest.raises(TypeError, match="PreparedKey"):
        asyncio.run(tn.prove_inputs_batch(rt, qap, {}, np.zeros((2, 2, 32), np.uint8)))
    assert rt.exchanges == 0


def test_witnesses_of_the_wrong_width(pn, tn, no_context):
    qap, c = _qap(pn)
    rt = tn.Runtime(0, 3, 1, random.Random(1), tn.LocalHub(3))
    with pytest.raises(ValueError, match="rows"):
        asyncio.run(tn.prove_batch(rt, qap, _key(pn), np.zeros((2, qap.m + 2, 32), np.uint8)))
    with pytest.raises(ValueError, match="rows"):
        asyncio.run(tn.prove_batch(rt, qap, _key(pn), [list(c), list(c)[:-1]]))
    with pytest.raises(ValueError, match="rows"):
        pn.compute_h_share_batch(qap, np.zeros((2, qap.m, 32), np.uint8))
    assert rt.exchanges == 0
    assert asyncio.run(tn.prove_batch(rt, qap, _key(pn), np.zeros((0, qap.m + 1, 32), np.uint8))) == []
    assert pn.compute_h_share_batch(qap, []) == []


def test_one_set_of_deltas_per_witness(pn, no_context):
    qap, c = _qap(pn)
    dl = types.SimpleNamespace(v=1, w=2, y=3)
    with pytest.raises(ValueError, match="deltas per witness"):
        pn.compute_h_share_batch(qap, [c, c, c], [dl, dl])
    buf = types.SimpleNamespace(ptr=0, nbytes=32 * 3 * 2)           # a device buffer of 2 x 3 scalars for 3 witnesses
    with pytest.raises(ValueError, match="deltas per witness"):
        pn.compute_h_share_batch(qap, [c, c, c], buf)


def test_batch_ranges_are_compute_h_batch_s_chunks(pn, monkeypatch):
    qap, c = _qap(pn)
    assert pn.batch_ranges(qap, 0) == [] and pn.batch_ranges(qap, 5) == [(0, 5)]
    one = pn.h_batch_bytes(int(qap.d), qap.m + 1, 0, 1)
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", pn.h_batch_bytes(int(qap.d), qap.m + 1, 0, 2))
    assert pn.batch_ranges(qap, 5) == [(0, 2), (2, 4), (4, 5)]
    monkeypatch.setattr(pn, "BATCH_BUDGET_BYTES", one - 1)          # below one witness: one per chunk, never empty
    assert pn.batch_ranges(qap, 3) == [(0, 1), (1, 2), (2, 3)]


def test_the_new_entries_are_declared_bound_and_exported(pn):
    from verifiable_mpc_amd import _native
    lib = _native.load_library()
    for name in ("vmpc_bn256_recombine_dev", "vmpc_bn256_qap_residual_batch_dev"):
        assert name in _native.SYMBOLS and getattr(lib, name).argtypes
    assert {"bn256_recombine", "bn256_qap_residual_batch"} <= set(dir(_native.Context))
