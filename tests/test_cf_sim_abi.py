"""CPU: the similarity calls (include/smatrix_batch.h smatrix_cf_recommend_sim / _dev, smatrix_merge_topk_sim) are declared with
their 15 / 16 / 10 arguments, exported by the library and not by the shim, bound by the ctypes layer with the declared argument
counts and scalar types, and reachable from SparseMatrix, whose argument checks come before any library call.  No compute calls."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import BAD_MIN_VALUES, BAD_OPS, ROOT, assert_raises, built, declared_args, exported, in_the_shim  # noqa: F401

NARGS = {"smatrix_cf_recommend_sim": 15, "smatrix_cf_recommend_sim_dev": 16, "smatrix_merge_topk_sim": 10}
BAD_SHRINKS = [-1.0, -1e-300, float("nan"), float("inf"), float("-inf"), None, "1", True]
BAD_SIMS = ["cos", "value", 1, None, True, ""]


def test_the_prototypes_are_in_the_header():
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    assert declared_args("smatrix_merge_topk_sim") == ["smatrix_t* dst", "smatrix_t* src", "int op", "int sim", "double shrink", "uint32_t m",
                                                        "uint32_t min_value", "uint64_t max_batch", "uint64_t* n_ops", "uint64_t* n_dropped"]
    args = declared_args("smatrix_cf_recommend_sim")
    assert args[8:12] == ["uint64_t deny_n", "int sim", "double shrink", "uint32_t k"]
    assert declared_args("smatrix_cf_recommend_sim_dev")[-1] == "void* hip_stream"


def test_the_measure_codes_are_in_the_header_and_merge_topk_by_keeps_its_two_ranks():
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    assert re.search(r"enum\s*\{\s*SMATRIX_SIM_COSINE\s*=\s*0\s*,\s*SMATRIX_SIM_JACCARD\s*=\s*1\s*,\s*SMATRIX_SIM_LIFT\s*=\s*2\s*\}\s*;", src)
    assert re.search(r"enum\s*\{\s*SMATRIX_RANK_VALUE\s*=\s*0\s*,\s*SMATRIX_RANK_COSINE\s*=\s*1\s*\}\s*;", src)


def test_the_symbols_are_exported(built):
    assert set(NARGS) <= exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert not set(NARGS) & in_the_shim(built)


@pytest.mark.parametrize("name", sorted(NARGS))
def test_the_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    fn, args = getattr(_lib.load(), name), declared_args(name)
    assert len(fn.argtypes) == len(args) == NARGS[name]
    scalars = dict(A.SCALARS, double=C.c_double, size_t=C.c_size_t)
    for bound, arg in zip(fn.argtypes, args):
        ctype = arg.rsplit(" ", 1)[0]
        assert ctype.endswith("*") or bound is scalars[ctype], (name, arg, bound)


def test_sparse_matrix_has_the_methods_and_their_defaults():
    from libsmatrix_amd import SparseMatrix
    assert callable(getattr(SparseMatrix, "cf_recommend_sim_dev", None))
    p = inspect.signature(SparseMatrix.cf_recommend_filtered).parameters
    assert p["sim"].default == "cosine" and p["shrink"].default == 0.0
    for meth in (SparseMatrix.merge_topk, SparseMatrix.truncated):
        p = inspect.signature(meth).parameters
        assert p["rank"].default == "value" and p["shrink"].default == 0.0


def handle_less():
    from libsmatrix_amd import SparseMatrix
    return SparseMatrix.__new__(SparseMatrix)       # no handle, no library: only the argument checks can run


@pytest.mark.parametrize("shrink", BAD_SHRINKS)
def test_a_bad_shrink_is_refused_before_any_library_call(shrink):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filtered([[1, 2, 3]], 10, sim="lift", shrink=shrink)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_sim_dev(1, 0, 0, None, None, None, None, 0, "lift", shrink, 10, 0, 0, 0)
    for rank in ("cosine", "jaccard", "lift", "value"):
        assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, rank=rank, shrink=shrink), lambda a, b: a.truncated(5, rank=rank, shrink=shrink))


@pytest.mark.parametrize("sim", BAD_SIMS)
def test_an_unknown_measure_is_refused_before_any_library_call(sim):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filtered([[1, 2, 3]], 10, sim=sim)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_sim_dev(1, 0, 0, None, None, None, None, 0, sim, 0.0, 10, 0, 0, 0)
    if sim != "value":
        assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, rank=sim), lambda a, b: a.truncated(5, rank=sim))


def test_shrinkage_needs_a_rank_that_scores():
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, rank="value", shrink=1.0), lambda a, b: a.truncated(5, shrink=0.5))


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_still_refused(k):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filtered([[1, 2, 3]], k, sim="jaccard", shrink=1.0)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_sim_dev(1, 0, 0, None, None, None, None, 0, "jaccard", 1.0, k, 0, 0, 0)


@pytest.mark.parametrize("op", BAD_OPS)
def test_unknown_op_is_still_refused(op):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, op, rank="lift", shrink=2.0))


@pytest.mark.parametrize("m", [0, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_bad_m_is_still_refused(m):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, m, rank="jaccard"), lambda a, b: a.truncated(m, rank="lift", shrink=3))


@pytest.mark.parametrize("min_value", BAD_MIN_VALUES)
def test_bad_min_value_is_still_refused(min_value):
    assert_raises(ValueError, lambda a, b: a.merge_topk(b, 5, "set", min_value, rank="lift"),
                  lambda a, b: a.truncated(5, min_value, rank="jaccard", shrink=1.0))


def test_something_else_than_a_matrix_is_a_type_error():
    assert_raises(TypeError, lambda a, b: a.merge_topk([1, 2, 3], 5, rank="lift", shrink=1.0))


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed (-0.0, an integer shrink, every measure): the call gets as far as the library,
    which a handle-less object does not have"""
    for sim, shrink in (("cosine", 0.1), ("jaccard", 0), ("lift", -0.0), ("lift", 10)):
        with pytest.raises(AttributeError):
            handle_less().cf_recommend_filtered([[1, 2, 3], []], 10, weights=[[0.0, 1.0, 2.5], []], sim=sim, shrink=shrink)
        assert_raises(AttributeError, lambda a, b: a.merge_topk(b, 5, rank=sim, shrink=shrink))
