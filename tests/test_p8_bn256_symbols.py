"""The header and the binding table name the GF(n) entries of Protocol 8 and of the knowledge-of-exponent opening's
staging step (no GPU; tests/test_cabi_symbols.py holds header, table and library against each other as wholes)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["vmpc_bn256_fr_cs_triples_dev", "vmpc_bn256_fr_cs_tables_dev", "vmpc_bn256_fr_cs_tables_scratch_bytes",
       "vmpc_bn256_fr_cs_lagrange_dev", "vmpc_bn256_fr_cs_lagrange_scratch_bytes", "vmpc_bn256_fr_cs_extend_dev",
       "vmpc_bn256_fr_cs_colsum_dev", "vmpc_bn256_fr_cs_first_diff_dev", "vmpc_bn256_fr_axpy_dev",
       "vmpc_bn256_fr_dot_to_dev", "vmpc_bn256_fr_dot_scratch_bytes", "vmpc_bn256_koe_stage_dev",
       "vmpc_bn256_koe_split_dev"]


def test_header_and_binding_table_name_the_new_entries():
    from verifiable_mpc_amd import _native
    header = open(os.path.join(ROOT, "include", "vmpc.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SYMBOLS, name


def test_the_entries_that_need_scratch_take_it_from_the_caller():
    """tables, lagrange and dot: a scratch pointer is the last parameter, and a _scratch_bytes query goes with it"""
    header = open(os.path.join(ROOT, "include", "vmpc.h")).read()
    for name in ("vmpc_bn256_fr_cs_tables_dev", "vmpc_bn256_fr_cs_lagrange_dev", "vmpc_bn256_fr_dot_to_dev"):
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert re.search(r"void \*scratch\s*$", decl), decl


def test_the_context_binds_both_fields_through_one_method():
    from verifiable_mpc_amd import _native
    import inspect
    for method in ("cs_triples", "cs_tables", "cs_extend", "cs_lagrange", "cs_first_diff", "fr_axpy", "fr_dot_into"):
        assert "bn" in inspect.signature(getattr(_native.Context, method)).parameters, method
