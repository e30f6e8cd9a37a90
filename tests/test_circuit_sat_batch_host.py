"""The host half of the batch Protocol 8 prover (verifiable_mpc_amd/circuit_sat_gpu.py): how `xs` is read, and the
workspace the batched extension asks for (vmpc_fr_cs_extend_batch_bytes: arithmetic on sizes, no device)."""
import numpy as np
import pytest

from tests import p8_ref as ref
from verifiable_mpc_amd import circuit_sat_gpu as cs

ELL = ref.ELL
MAX_M, MAX_WIT = 1 << 20, 65535             # VMPC_FR_CS_MAX_M, VMPC_FR_CS_MAX_WIT of include/vmpc.h


@pytest.fixture(scope="module")
def lib():
    from verifiable_mpc_amd import _native, build
    build.build(verbose=False)
    return _native.load_library()


def _ints(rows):
    return [[int.from_bytes(rows[p, i].tobytes(), "little") for i in range(rows.shape[1])] for p in range(rows.shape[0])]


def test_input_lists_become_rows_of_residues():
    xs = [[1, -3, ELL + 5], (0, 2 ** 300, ELL - 1)]
    K, n_in, rows = cs._batch_inputs(xs, None)
    assert (K, n_in) == (2, 3) and rows.shape == (2, 3, 32) and rows.dtype == np.uint8
    assert _ints(rows) == [[v % ELL for v in x] for x in xs]
    assert cs._input_lists(xs, None) == [list(x) for x in xs]
    assert cs._batch_inputs([], None)[0] == 0
    K, n_in, rows = cs._batch_inputs([[], []], None)          # two witnesses of a circuit without inputs
    assert (K, n_in) == (2, 0) and rows.shape == (2, 0, 32)
    with pytest.raises(ValueError, match="same number of inputs"):
        cs._batch_inputs([[1, 2], [1]], None)


def test_input_array_passes_through_and_is_reduced_where_it_must_be():
    want = [[1, ELL - 1, 0], [2 ** 252, 5, ELL - 2]]
    canonical = np.frombuffer(b"".join(v.to_bytes(32, "little") for x in want for v in x), np.uint8).reshape(2, 3, 32)
    K, n_in, rows = cs._batch_inputs(canonical, None)
    assert (K, n_in) == (2, 3) and _ints(rows) == want
    raw = [[1 + ELL, ELL - 1, ELL], [2 ** 252, 5 + 3 * ELL, 2 ** 256 - 1]]
    wide = np.frombuffer(b"".join(v.to_bytes(32, "little") for x in raw for v in x), np.uint8).reshape(2, 3, 32)
    before = wide.copy()
    K, n_in, rows = cs._batch_inputs(wide, None)
    assert _ints(rows) == [[v % ELL for v in x] for x in raw]
    assert (wide == before).all()                               # the caller's array is not written
    assert cs._input_lists(wide, None) == [[v % ELL for v in x] for x in raw]
    for bad in (np.zeros((2, 3), np.uint8), np.zeros((2, 3, 31), np.uint8)):
        with pytest.raises(ValueError, match=r"\(K, n_in, 32\)"):
            cs._batch_inputs(bad, None)


def test_batched_extension_workspace(lib):
    """the segment length is chosen with the witnesses counted: tiles x segments x K against 8192 workgroups"""
    size = lib.vmpc_fr_cs_extend_batch_bytes
    # K = 1 is the single call's plan: m = 1000 -> 4 segments of 256, 2 x 4 x 999 partial sums
    assert 2 * 4 * 999 * 32 <= size(1000, 1) < 2 * 4 * 999 * 32 + (2 * 1001 + 2002 + 2) * 32 + (1 << 13)
    # m = 1000: 4 x 4 x K workgroups - 4 segments up to K = 512, 2 from 513 on: one more witness, less workspace
    assert size(1000, 512) < 512 * size(1000, 1) + (1 << 13)
    assert size(1000, 513) < size(1000, 512)
    # m = 2^16: 8 witnesses take less than twice one witness's partial sums, not eight times
    assert 0 < size(1 << 16, 1) < size(1 << 16, 8) < 2 * size(1 << 16, 1)
    # a large batch ends at one segment per witness
    assert size(1 << 12, 4096) < 4096 * (2 * 4097 + 2 * 4095 + 2) * 32 + (1 << 20)
    # where the call would answer VMPC_E_RANGE or do nothing
    assert size(MAX_M + 1, 1) == 0 and size(8, MAX_WIT + 1) == 0 and size(8, 0) == 0
    assert size(MAX_M, 1) > 0 and size(0, MAX_WIT) > 0
