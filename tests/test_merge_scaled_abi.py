"""CPU: smatrix_merge_scaled (include/smatrix_batch.h) is declared in the header with its 9 arguments, exported by the library
and not by the shim, bound by the ctypes layer with the declared argument count, and reachable from SparseMatrix as merge_scaled
and pruned, whose argument checks fire before any handle is touched.  No compute calls."""
import pytest

from tests.merge_abi_helpers import (BAD_MIN_VALUES, BAD_OPS, assert_binding_matches_the_header, assert_methods, assert_raises,  # noqa: F401
                                     built, declared_args, exported, in_the_shim)

NAME, NARGS = "smatrix_merge_scaled", 9


def test_the_prototype_is_in_the_header():
    args = declared_args(NAME)
    assert len(args) == NARGS, args
    assert [a.split()[-1].lstrip("*") for a in args] == ["dst", "src", "op", "num", "den", "min_value", "max_batch", "n_ops", "n_dropped"]


def test_the_symbol_is_exported(built):
    assert NAME in exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert NAME not in in_the_shim(built)


def test_the_binding_matches_the_header(built):
    assert_binding_matches_the_header(NAME, NARGS)


def test_sparse_matrix_has_the_methods():
    assert_methods("merge_scaled", "pruned")


@pytest.mark.parametrize("op", BAD_OPS)
def test_unknown_op_is_refused_before_any_device_call(op):
    assert_raises(ValueError, lambda a, b: a.merge_scaled(b, op))


@pytest.mark.parametrize("num, den", [(0, 1), (1, 0), (0, 0), (2, 1), (10, 9), (1, 1 << 32), (1 << 32, 1 << 32), (-1, 2), (1, -2),
                                      (0.5, 1), (1, 2.0), (None, 1), ("1", "2"), (True, True)])
def test_bad_fraction_is_refused_before_any_device_call(num, den):
    assert_raises(ValueError, lambda a, b: a.merge_scaled(b, "incr", num, den), lambda a, b: a.pruned(1, num, den))


@pytest.mark.parametrize("min_value", BAD_MIN_VALUES)
def test_bad_min_value_is_refused_before_any_device_call(min_value):
    assert_raises(ValueError, lambda a, b: a.merge_scaled(b, "set", 1, 2, min_value), lambda a, b: a.pruned(min_value))


def test_something_else_than_a_matrix_is_a_type_error():
    assert_raises(TypeError, lambda a, b: a.merge_scaled([1, 2, 3]), lambda a, b: a.merge_scaled(3, "set", 1, 2, 1))
