"""CPU: smatrix_merge_topk_by (include/smatrix_batch.h) is declared in the header with its 9 arguments, exported by the library and
not by the shim, bound by the ctypes layer with the declared argument count, and reachable from SparseMatrix.merge_topk and
SparseMatrix.truncated through rank=, whose argument checks fire before any handle is touched.  No compute calls."""
import inspect
import os
import re

import pytest

from tests.merge_abi_helpers import (BAD_MIN_VALUES, BAD_OPS, ROOT, assert_binding_matches_the_header, assert_raises,  # noqa: F401
                                     built, declared_args, exported, in_the_shim)

NAME, NARGS = "smatrix_merge_topk_by", 9
BAD_RANKS = ["cos", 2, None, True]


def test_the_prototype_is_in_the_header():
    args = declared_args(NAME)
    assert len(args) == NARGS, args
    assert args == ["smatrix_t* dst", "smatrix_t* src", "int op", "int rank", "uint32_t m", "uint32_t min_value", "uint64_t max_batch",
                    "uint64_t* n_ops", "uint64_t* n_dropped"]


def test_the_rank_codes_are_in_the_header():
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    assert re.search(r"enum\s*\{\s*SMATRIX_RANK_VALUE\s*=\s*0\s*,\s*SMATRIX_RANK_COSINE\s*=\s*1\s*\}\s*;", src)


def test_the_symbol_is_exported(built):
    assert NAME in exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert NAME not in in_the_shim(built)


def test_the_binding_matches_the_header(built):
    assert_binding_matches_the_header(NAME, NARGS)      # (the scalars: int op, int rank, uint32_t m, uint32_t min_value, uint64_t max_batch)


def test_the_methods_accept_rank_and_default_to_value():
    from libsmatrix_amd import SparseMatrix
    for meth in (SparseMatrix.merge_topk, SparseMatrix.truncated):
        assert inspect.signature(meth).parameters["rank"].default == "value"


@pytest.mark.parametrize("rank", BAD_RANKS)
def test_unknown_rank_is_refused_before_any_device_call(rank):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, rank=rank), lambda a, b: a.truncated(5, rank=rank))


@pytest.mark.parametrize("op", BAD_OPS)
def test_unknown_op_is_still_refused_with_the_cosine_rank(op):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, op, rank="cosine"))


@pytest.mark.parametrize("m", [0, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_bad_m_is_still_refused_with_the_cosine_rank(m):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, m, rank="cosine"), lambda a, b: a.truncated(m, rank="cosine"))


@pytest.mark.parametrize("min_value", BAD_MIN_VALUES)
def test_bad_min_value_is_still_refused_with_the_cosine_rank(min_value):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, "set", min_value, rank="cosine"),
                  lambda a, b: a.truncated(5, min_value, rank="cosine"))


def test_something_else_than_a_matrix_is_a_type_error():
    assert_raises(TypeError, lambda a, b: a.merge_topk([1, 2, 3], 5, rank="cosine"))
