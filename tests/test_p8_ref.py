"""tests/p8_ref.py against itself (naive route = barycentric route), against the reference-made fixture
(tests/golden/p8_circuits.json), and the host half of verifiable_mpc_amd.circuit_sat_gpu (SparseCircuit: canonical
form, digest, levels, padding, from_circuit) - no GPU."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from tests import p8_ref as ref
from tests.conftest import load_golden
from verifiable_mpc_amd.circuit_sat_gpu import SparseCircuit

ELL = ref.ELL
GPU_CASES, sparse = ref.GPU_CASES, ref.sparse


def fake_commit(z):
    import hashlib
    return hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in z)).digest()


@pytest.mark.parametrize("m", [0, 1, 2, 3, 7, 12])
def test_naive_and_barycentric_routes_agree(m):
    rng = random.Random(1000 + m)
    n_x = 4
    A, B, O = ref.random_circuit(rng, n_x, m, 2)
    x = [rng.randrange(ELL) for _ in range(n_x)] + [0, 0]
    a, b, gamma = ref.triples(n_x, A, B, x)
    r_a, r_b = rng.randrange(1, ELL), rng.randrange(1, ELL)
    assert ref.z_tail_naive(a, b, r_a, r_b) == ref.z_tail_bary(a, b, r_a, r_b, kronecker=False)
    assert ref.z_tail_bary(a, b, r_a, r_b, kronecker=True) == ref.z_tail_bary(a, b, r_a, r_b, kronecker=False)
    c = rng.randrange(2 * m + 1, ELL)
    assert ref.lagrange_naive(m, c) == ref.lagrange_bary(m, c)
    assert ref.lagrange_naive(2 * m, c) == ref.lagrange_bary(2 * m, c)
    p1 = ref.prove(n_x, A, B, O, x, r_a, r_b, fake_commit, "naive")
    p2 = ref.prove(n_x, A, B, O, x, r_a, r_b, fake_commit, "bary")
    assert p1 == p2
    # the forms open f, g, h at c
    f = ref.interpolate(a + [r_a])
    assert p1["y"][0] == ref.poly_eval(f, p1["c"])


def test_lagrange_on_a_node_has_no_reference_value():
    with pytest.raises(ZeroDivisionError):
        ref.lagrange_naive(4, 3)
    assert ref.lagrange_bary(4, 3) == [0, 0, 0, 1, 0]      # the product form is exact there; the prover still refuses


@pytest.mark.parametrize("m,top", [(2, False), (258, False), (513, False), (513, True)],
                         ids=["m2", "m258", "m513", "m513_top"])
def test_kronecker_convolution_is_the_direct_sum(m, top):
    """tests/test_gpu_p8_primitives.py takes z_tail_bary's Kronecker route from m = 512 on: it is the double loop, with
    random values and with every value l - 1 (the largest terms a 66-byte slot has to hold)"""
    rng = random.Random(5000 + m)
    a, b = ([ELL - 1] * m,) * 2 if top else ([rng.randrange(ELL) for _ in range(m)], [rng.randrange(ELL) for _ in range(m)])
    r_a, r_b = (ELL - 1, ELL - 1) if top else (rng.randrange(ELL), rng.randrange(ELL))
    direct = ref.z_tail_bary(a, b, r_a, r_b, kronecker=False)
    assert ref.z_tail_bary(a, b, r_a, r_b, kronecker=True) == direct
    assert len(direct) == 2 * m + 3 and direct[3:3 + m] == [x * y % ELL for x, y in zip(a, b)]


@pytest.mark.parametrize("K", [1, 33, 8193])
def test_lagrange_bary_on_and_off_the_nodes(K):
    """on a node the product form gives the unit vector (what the GPU test expects of the kernel there); off the nodes
    it is the reference's double loop"""
    for c in sorted({j for j in (0, 1, 31, 32, 33, K // 2, K - 1, K) if 0 <= j <= K}):
        assert ref.lagrange_bary(K, c) == [int(j == c) for j in range(K + 1)], c
    if K <= 33:
        rng = random.Random(K)
        for c in (K + 1, ELL - 1, rng.randrange(K + 1, ELL)):
            assert ref.lagrange_bary(K, c) == ref.lagrange_naive(K, c), c


@pytest.mark.parametrize("seed,n_x,m,n_out", GPU_CASES)
def test_generator_makes_circuits_the_convention_accepts(seed, n_x, m, n_out):
    rng = random.Random(seed)
    A, B, O = ref.random_circuit(rng, n_x, m, n_out, long_col=1 if m >= 100 else None)
    sc = sparse(n_x, A, B, O)        # raises if a row reads a later gamma
    assert (sc.m, sc.n_out, sc.n_x) == (m, n_out, n_x)
    assert sc.digest == ref.circuit_digest(n_x, A, B, O)
    for M in (A, B):
        for i, (e, _) in enumerate(M):
            assert all(c < n_x + i for c in e)
    # levels: every gate sits above every gate it reads
    for M in (A, B):
        for i, (e, _) in enumerate(M):
            for c in e:
                if c >= n_x:
                    assert sc.depth[c - n_x] < sc.depth[i]
    assert sorted(sc.level_order.tolist()) == list(range(m))
    if m >= 1000:
        counts = np.bincount(np.concatenate([sc.A.col, sc.B.col, sc.O.col]))
        assert counts.max() > 64       # the long-column path is exercised


def test_canonical_form_adds_duplicates_and_reduces():
    a = SparseCircuit(2, ([0, 3], [0, 0, 1], [5, -7, ELL + 3], [2 * ELL + 1]), ([0, 1], [1], [1], [0]))
    b = SparseCircuit(2, ([0, 2], [1, 0], [3, ELL - 2], [1]), ([0, 1], [1], np.array([1]), None))
    assert a.digest == b.digest
    c = SparseCircuit(2, ([0, 2], [1, 0], [3, ELL - 2], [2]), ([0, 1], [1], [1], [0]))
    assert c.digest != a.digest
    z = SparseCircuit(2, ([0, 2], [0, 1], [4, 0], [0]), ([0, 1], [1], [1], [0]))       # an explicit zero is no entry
    assert len(z.A.col) == 1


def test_row_reading_a_later_gamma_is_refused():
    with pytest.raises(ValueError, match="row 1 of B reads gamma_1"):
        SparseCircuit(1, ([0, 1, 2], [0, 1], [1, 1]), ([0, 1, 2], [0, 2], [1, 1]))
    with pytest.raises(ValueError, match="row 0 of A reads gamma_0"):
        SparseCircuit(1, ([0, 1], [1], [1]), ([0, 1], [0], [1]))


def test_padding_rule():
    sc = SparseCircuit(3, ([0, 1, 2], [0, 3], [1, 1]), ([0, 1, 2], [1, 2], [1, 1]))       # m = 2
    assert sc.padding() == 5 and len(sc.pad([1, 2, 3])) == 8 and (8 + 3 + 4 + 1) == 16
    assert sc.padding(8) == 0
    from verifiable_mpc_amd.circuit_sat import check_input_length_power_of_2
    assert check_input_length_power_of_2([0] * 3, sc)[1] == 5


def builder_circuit():
    """x0 * x1 -> g0;  t = 3 * g0 + x2 + 7 (scalar-mul, adds, a constant wire);  t * t -> g1;  outputs: g1 and t"""
    op = lambda name: SimpleNamespace(name=name)      # noqa: E731
    var = lambda name, ix=None: SimpleNamespace(name=name, input_index=ix, output_index=None)     # noqa: E731
    x0, x1, x2 = var("x_input_0", 0), var("y_input_1", 1), var("w_input_2", 2)
    d0, d1, d2, d3, d4 = (var(f"dummy_{i}") for i in range(5))
    gates = [SimpleNamespace(op=op("mul"), inputs=[x0, x1], output=d0, mul_index=0),
             SimpleNamespace(op=op("scalar_mul"), inputs=[d0, 3], output=d1, mul_index=None),
             SimpleNamespace(op=op("add"), inputs=[d1, x2], output=d2, mul_index=None),
             SimpleNamespace(op=op("add"), inputs=[d2, 7], output=d3, mul_index=None),
             SimpleNamespace(op=op("mul"), inputs=[d3, d3], output=d4, mul_index=1)]
    d4.output_index, d3.output_index = 0, 1

    class C:
        input_ct, mul_ct, output_gates = 3, 2, [4, 3]

        def mul_gates(self):
            return [g for g in gates if g.op.name == "mul"]

        def __str__(self):
            return "stand-in"
    c = C()
    c.gates = gates
    return c


def test_from_circuit_follows_construct_affine_form():
    sc = SparseCircuit.from_circuit(builder_circuit())
    want = sparse(3, [({0: 1}, 0), ({3: 3, 2: 1}, 7)], [({1: 1}, 0), ({3: 3, 2: 1}, 7)], [({4: 1}, 0), ({3: 3, 2: 1}, 7)])
    assert sc.digest == want.digest
    assert sc.text == "stand-in" and str(sc) == "stand-in"
    assert sc.depth.tolist() == [0, 1]


# ---- against the reference-made fixture --------------------------------------------------------------------------------
FIXTURE = load_golden("p8_circuits.json")["cases"]


@pytest.mark.parametrize("case", FIXTURE, ids=[c["name"] for c in FIXTURE])
def test_both_routes_reproduce_the_reference(case):
    """the restatement's reading of the z layout, the node numbering and the position of the gamma columns is the
    reference's: from the recorded forms, x, r_a, r_b and the recorded challenges, both routes give the recorded
    a, b, c, z, forms of f(c), g(c), h(c), y1..y3, outputs and L (as residues)"""
    n_x, m = case["input_ct"], case["mul_ct"]
    res = lambda s: ref.untyped(s) % ELL      # noqa: E731
    A, B, O = (ref.fixture_rows(case[k]) for k in "ABO")
    x = [res(v) for v in case["x_typed"]]
    a, b, gamma = ref.triples(n_x, A, B, x)
    assert (a, b, gamma) == tuple([res(v) for v in case[k]] for k in ("a_typed", "b_typed", "c_typed"))
    r_a, r_b = int(case["r_a"], 16), int(case["r_b"], 16)
    z = [res(v) for v in case["z_typed"]]
    assert x + ref.z_tail_naive(a, b, r_a, r_b) == z
    assert x + ref.z_tail_bary(a, b, r_a, r_b) == z
    c, rho = int(case["hashes"][0]["c"], 16), int(case["hashes"][1]["c"], 16)
    y = [res(v) for v in case["y_typed"]]
    outputs = [res(v) for v in case["outputs_typed"]]
    assert [ref.row_eval(r, n_x, x, gamma) for r in O] == outputs
    for route in ("naive", "bary"):
        co, const, forms = ref.combine(n_x, n_x, A, B, O, c, rho, y, outputs, route)
        for (fc, fk), key in zip(forms, ("linform_f", "linform_g", "linform_h")):
            assert fc == [res(v) for v in case[key]["coeffs"]]
            assert fk == res(case[key]["constant"])
            assert (ref.dot(fc, z) + fk) % ELL == y[("linform_f", "linform_g", "linform_h").index(key)]
        assert co == [res(v) for v in case["L"]["coeffs"]]
        assert const == res(case["L"]["constant"])


@pytest.mark.parametrize("case", FIXTURE, ids=[c["name"] for c in FIXTURE])
def test_from_circuit_gives_the_recorded_forms(case):
    """SparseCircuit.from_circuit over the recorded gates = the reference's construct_affine_form, coefficient for
    coefficient with its Python types"""
    sc = SparseCircuit.from_circuit(ref.circuit_from_fixture(case))
    raw = sc.raw_forms()
    for key in "ABO":
        want = ref.fixture_rows(case[key])
        got = [({c: v for c, v in e.items() if v != 0}, k) for e, k in raw[key]]
        assert got == want
        assert [[type(v) for v in e.values()] for e, _ in got] == [[type(v) for v in e.values()] for e, _ in want]
    assert sc.text == case["circuit_str"]
    assert sc.digest == sparse(case["input_ct"], *(ref.fixture_rows(case[k]) for k in "ABO")).digest
