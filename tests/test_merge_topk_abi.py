"""CPU: smatrix_merge_topk (include/smatrix_batch.h) is declared in the header with its 8 arguments, exported by the library and
not by the shim, bound by the ctypes layer with the declared argument count, and reachable from SparseMatrix as merge_topk and
truncated, whose argument checks fire before any handle is touched.  No compute calls."""
import pytest

from tests.merge_abi_helpers import (BAD_MIN_VALUES, BAD_OPS, assert_binding_matches_the_header, assert_methods, assert_raises,  # noqa: F401
                                     built, declared_args, exported, in_the_shim)

NAME, NARGS = "smatrix_merge_topk", 8


def test_the_prototype_is_in_the_header():
    args = declared_args(NAME)
    assert len(args) == NARGS, args
    assert args == ["smatrix_t* dst", "smatrix_t* src", "int op", "uint32_t m", "uint32_t min_value", "uint64_t max_batch",
                    "uint64_t* n_ops", "uint64_t* n_dropped"]


def test_the_symbol_is_exported(built):
    assert NAME in exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert NAME not in in_the_shim(built)


def test_the_binding_matches_the_header(built):
    assert_binding_matches_the_header(NAME, NARGS)      # (the scalars: int op, uint32_t m, uint32_t min_value, uint64_t max_batch)


def test_sparse_matrix_has_the_methods():
    assert_methods("merge_topk", "truncated")


@pytest.mark.parametrize("op", BAD_OPS)
def test_unknown_op_is_refused_before_any_device_call(op):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, op))


@pytest.mark.parametrize("m", [0, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_bad_m_is_refused_before_any_device_call(m):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, m), lambda a, b: a.truncated(m))


@pytest.mark.parametrize("min_value", BAD_MIN_VALUES)
def test_bad_min_value_is_refused_before_any_device_call(min_value):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, "set", min_value), lambda a, b: a.truncated(5, min_value))


def test_something_else_than_a_matrix_is_a_type_error():
    assert_raises(TypeError, lambda a, b: a.merge_topk([1, 2, 3], 5), lambda a, b: a.merge_topk(3, 5, "set", 1))
