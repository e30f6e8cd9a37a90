"""CPU checks of the key-generation restatement (tests/keygen_ref.py) against the reference-made fixture
(tests/golden/pinocchio_keygen.json, tests/golden/make_keygen_fixtures.py): the sparse evaluation equals Horner on the
reference's dense QAP, equals plain Lagrange interpolation on random R1CS, and the fixture's key points are the
oracle's multiples of g1 / g2 by the restated exponents - before any GPU test relies on them."""
import random

import pytest

from oracle import bn256_ref as bn
from tests import keygen_ref as K
from tests.conftest import load_golden

N = K.N
h2i = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def fx():
    return load_golden("pinocchio_keygen.json")["cases"]


def _td(case):
    t = {k: h2i(v) for k, v in case["trapdoor"].items()}
    return K.TD(t["r_v"], t["r_w"], t["s"], t["alpha_v"], t["alpha_w"], t["alpha_y"], t["beta"], t["gamma"], t["r_y"])


def _entries(case):
    r = case["r1cs"]
    return K.entries_of_rows(r["V"]), K.entries_of_rows(r["W"]), K.entries_of_rows(r["Y"])


def test_fixture_shape(fx):
    assert [c["name"] for c in fx] == ["demo", "larger"]
    assert 16 <= fx[1]["d"] <= 64
    for case in fx:
        assert all(case["verification"].values())
        td = _td(case)
        assert td.r_y == td.r_v * td.r_w % N


@pytest.mark.parametrize("which", ["fixture", "0", "1", "d", "random"])
def test_sparse_equals_dense_horner(fx, which):
    """sum_j V[j][i] l_j(s) == the reference's v_i polynomial at s (and w, y, t) for both fixture programs"""
    for case in fx:
        d, n_cols = case["d"], case["m"] + 1
        s = {"fixture": _td(case).s, "0": 0, "1": 1, "d": d, "random": random.Random(7).randrange(N)}[which]
        v, w, y, t = K.qap_at(*_entries(case), n_cols, d, s)
        q = case["qap"]
        for name, got in (("v", v), ("w", w), ("y", y)):
            want = [K.horner([h2i(c) for c in poly], s) for poly in q[name]]
            assert got == want, (case["name"], name, which)
        assert t == K.horner([h2i(c) for c in q["t"]], s)


def _random_r1cs(rng, d, n_cols):
    """entries with negative values, values >= N, duplicates, an empty column (n_cols - 1) and a full one (column 1)"""
    ents = []
    for r in range(d):
        ents.append((r, 1, rng.choice([rng.randrange(-5, 6), rng.randrange(N, 3 * N), -rng.randrange(N)])))
        for _ in range(rng.randrange(0, 3)):
            ents.append((r, rng.randrange(0, n_cols - 1), rng.randrange(-(1 << 300), 1 << 300)))
    ents += [ents[rng.randrange(len(ents))] for _ in range(d // 4 + 1)]       # duplicates add
    return [(r, c, x % N) for r, c, x in ents]


@pytest.mark.parametrize("d", [1, 2, 5, 17, 64])
def test_sparse_equals_interpolation_random(d):
    rng = random.Random(1000 + d)
    n_cols = 7
    ents = _random_r1cs(rng, d, n_cols)
    assert not any(c == n_cols - 1 for _, c, _ in ents)
    cols = K.interpolate_columns(ents, n_cols, d)
    t_poly = [1]
    for j in range(1, d + 1):
        t_poly = [((t_poly[i - 1] if i else 0) - j * (t_poly[i] if i < len(t_poly) else 0)) % N
                  for i in range(len(t_poly) + 1)]
    for s in (0, 1, d, rng.randrange(N), N - 1):
        ell, t = K.lagrange_at(s, d)
        got = K.column_values(ents, n_cols, ell)
        assert got == [K.horner(c, s) for c in cols], s
        assert t == K.horner(t_poly, s)
        assert got[n_cols - 1] == 0


def _point(group, enc):
    if enc is None:
        return None
    v = [h2i(x) for x in enc]
    return (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))


def test_fixture_keys_are_oracle_multiples(fx):
    """every evalkey / verikey point of the fixture == E.mul(restated exponent, G), names in the reference's order"""
    for case in fx:
        td = _td(case)
        d, n_cols, out_ix = case["d"], case["m"] + 1, case["out_ix"]
        v, w, y, t = K.qap_at(*_entries(case), n_cols, d, td.s)
        mid, io0 = range(out_ix + 1, n_cols), range(0, out_ix + 1)
        for key, want in (("evalkey", K.evalkey_exponents(td, v, w, y, t, mid, d)),
                          ("verikey", K.verikey_exponents(td, v, w, y, t, io0))):
            got = case[key]
            assert [name for name, _ in got] == [name for name, _, _ in want], key
            for (name, enc), (_, group, e) in zip(got, want):
                E, G = (bn.E1, bn.G1) if group == 1 else (bn.E2, bn.G2)
                assert _point(group, enc) == E.mul(e, G), (case["name"], key, name)
