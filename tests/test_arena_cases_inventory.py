"""The case table of tests/arena_cases.py names every function of csrc/ that takes memory from a context's arena
(no GPU).  A new arena user without a case - or a case taken out of the table - fails here."""
import os
import re

from tests import arena_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_arena_user_has_a_case_or_a_named_exemption():
    users = A.arena_users()
    assert len(users) >= 39, sorted(users)                      # (the scan itself still finds what it found when written)
    declared = {t for c in A.CASES for t in c.targets}
    assert not declared & set(A.EXEMPT), "a function is both covered and exempt"
    assert users - declared - set(A.EXEMPT) == set(), "arena users without a case in tests/arena_cases.py"
    assert (declared | set(A.EXEMPT)) - users == set(), "cases or exemptions for functions that no longer reserve the arena"
    assert all(reason.strip() for reason in A.EXEMPT.values())
    assert sorted(A.EXEMPT) == [("bn256_probe.hip", "bn_madd_rate"), ("msm.hip", "vmpc_ed25519_madd_rate"),
                                ("probe.hip", "vmpc_gather_probe_dev")]


def test_the_scan_sees_a_reserve_wherever_it_stands():
    """the functions the scan has to find in the hard places: a template in a header, a static helper, a function
    inside extern "C" that reserves in one branch only"""
    users = A.arena_users()
    for u in (("fr_colsum.h", "fr_colsum"), ("prover.hip", "p4_round_enqueue"), ("nullity.hip", "vmpc_fr_rows_combine_dev"),
              ("bn256_koe.hip", "koe_poly_mul"), ("bn256_qap_mtree.hip", "mt_build")):
        assert u in users, u
    assert not any(fn == "vmpc_ws_reserve" for _, fn in users)


def test_cases_are_well_formed():
    names = [c.name for c in A.CASES]
    assert len(set(names)) == len(names)
    for c in A.CASES:
        assert c.targets and callable(c.run), c.name
        assert c.foreign in A.BY_NAME and c.foreign != c.name, (c.name, c.foreign)
        assert c._want is not None or c.name == "prover", c.name       # only the prover is judged by its own verifier


def test_every_case_names_an_existing_test_as_the_source_of_its_shape():
    for c in A.CASES:
        path, _, test = c.source.partition("::")
        full = os.path.join(ROOT, path)
        assert path.startswith("tests/test_gpu_") and os.path.exists(full), (c.name, c.source)
        assert re.search(r"^def %s\(" % re.escape(test), open(full).read(), flags=re.M), (c.name, c.source)


def test_no_fill_value_above_the_cap():
    from tests import test_gpu_arena_independence as T
    assert T.FILL_MAX == 0xFFFF and all(0 <= w <= T.FILL_MAX for w in T.FILLS)
    header = open(os.path.join(ROOT, "include", "vmpc.h")).read()
    assert re.search(r"#define VMPC_DEBUG_ARENA_FILL_MAX 0xFFFFu\b", header)
