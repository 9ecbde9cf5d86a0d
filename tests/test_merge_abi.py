"""CPU: smatrix_merge / smatrix_import_csr / smatrix_import_csr_dev (include/smatrix_batch.h) are declared in the header, exported
by the library, bound by the ctypes layer with the declared argument counts, and reachable from SparseMatrix.  No compute calls."""
import operator

import numpy as np
import pytest

from tests.merge_abi_helpers import (BAD_OPS, assert_binding_matches_the_header, assert_methods, assert_raises, built,  # noqa: F401
                                     declared_args, exported, in_the_shim)

CALLS = {"smatrix_merge": 5, "smatrix_import_csr": 8, "smatrix_import_csr_dev": 9}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_merge_prototypes_are_in_the_header(name):
    assert len(declared_args(name)) == CALLS[name]


def test_merge_symbols_are_exported(built):
    assert set(CALLS) <= exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert not (set(CALLS) & in_the_shim(built))


@pytest.mark.parametrize("name", sorted(CALLS))
def test_merge_binding_matches_the_header(built, name):
    assert_binding_matches_the_header(name, CALLS[name])


def test_sparse_matrix_has_the_merge_methods():
    assert_methods("merge", "__iadd__", "__isub__", "import_csr", "import_csr_dev", "from_sparse_coo")


@pytest.mark.parametrize("op", BAD_OPS)
def test_unknown_op_is_refused_before_any_device_call(op):
    assert_raises(ValueError,
                  lambda a, b: a.merge(b, op),
                  lambda a, b: a.import_csr(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros((0, 2), np.uint32), op),
                  lambda a, b: a.import_csr_dev(0, 0, 0, op, n_rows=0),
                  lambda a, b: a.from_sparse_coo(None, op))


def test_iadd_of_something_else_is_a_type_error():
    assert_raises(TypeError, lambda a, b: operator.iadd(a, 3), lambda a, b: a.merge([1, 2, 3]))
