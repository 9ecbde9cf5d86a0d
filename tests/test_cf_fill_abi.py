"""CPU: the popular call and the fill call (include/smatrix_batch.h smatrix_cf_popular / _dev, smatrix_cf_recommend_fill / _dev) are
declared with their exact argument lists, exported by the library and not by the shim, bound by the ctypes layer with the declared
argument counts and scalar types, and reachable from SparseMatrix, whose argument checks come before any library call.  No compute
calls."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import handle_less

NARGS = {"smatrix_cf_popular": 8, "smatrix_cf_popular_dev": 9, "smatrix_cf_recommend_fill": 18, "smatrix_cf_recommend_fill_dev": 19}


def test_the_prototypes_are_in_the_header():
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    assert declared_args("smatrix_cf_popular") == [
        "smatrix_t* self", "const uint32_t* deny_bits", "uint64_t deny_n", "uint32_t min_total", "uint32_t n", "uint32_t* ids",
        "uint32_t* totals", "uint32_t* n_found"]
    assert declared_args("smatrix_cf_popular_dev") == [
        "smatrix_t* self", "const uint32_t* d_deny_bits", "uint64_t deny_n", "uint32_t min_total", "uint32_t n", "uint32_t* d_ids",
        "uint32_t* d_totals", "uint32_t* d_n_found", "void* hip_stream"]
    sim, fill = declared_args("smatrix_cf_recommend_sim"), declared_args("smatrix_cf_recommend_fill")
    assert fill == sim[:9] + ["const uint32_t* fill_ids", "uint64_t n_fill"] + sim[9:] + ["uint32_t* n_scored"]
    sim, fill = declared_args("smatrix_cf_recommend_sim_dev"), declared_args("smatrix_cf_recommend_fill_dev")
    assert fill == sim[:9] + ["const uint32_t* d_fill_ids", "uint64_t n_fill"] + sim[9:-1] + ["uint32_t* d_n_scored", "void* hip_stream"]
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    assert "#define SMATRIX_POPULAR_MAX 4096u" in src


def test_the_sim_call_is_declared_as_before():
    args = declared_args("smatrix_cf_recommend_sim")
    assert len(args) == 15 and args[8:12] == ["uint64_t deny_n", "int sim", "double shrink", "uint32_t k"] and args[-1] == "uint32_t* counts"
    args = declared_args("smatrix_cf_recommend_sim_dev")
    assert len(args) == 16 and args[-2:] == ["uint32_t* d_counts", "void* hip_stream"]
    assert len(declared_args("smatrix_cf_recommend_filtered")) == 13


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
    import libsmatrix_amd
    from libsmatrix_amd import SparseMatrix
    assert libsmatrix_amd.POPULAR_MAX == 4096
    p = inspect.signature(SparseMatrix.cf_popular).parameters
    assert list(p) == ["self", "n", "deny", "min_total"] and (p["deny"].default, p["min_total"].default) == (None, 1)
    p = inspect.signature(SparseMatrix.cf_popular_dev).parameters
    assert list(p) == ["self", "n", "deny_ptr", "deny_n", "min_total", "ids_ptr", "totals_ptr", "n_found_ptr", "stream"]
    assert p["stream"].default is None
    p = inspect.signature(SparseMatrix.cf_recommend_filled).parameters
    assert list(p) == ["self", "sessions", "k", "fill", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in list(p)[4:]] == [None, None, None, "cosine", 0.0] and p["fill"].default is inspect.Parameter.empty
    p = inspect.signature(SparseMatrix.cf_recommend_fill_dev).parameters
    assert list(p) == ["self", "n", "off_ptr", "items_ptr", "weights_ptr", "ex_off_ptr", "ex_items_ptr", "deny_ptr", "deny_n", "fill_ptr", "n_fill",
                       "sim", "shrink", "k", "ids_ptr", "scores_ptr", "cnt_ptr", "n_scored_ptr", "stream"]
    p = inspect.signature(SparseMatrix.cf_recommend_filtered).parameters      # the existing call keeps its signature
    assert list(p) == ["self", "sessions", "k", "weights", "exclude", "deny", "sim", "shrink"]


@pytest.mark.parametrize("n", [0, 4097, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_a_bad_n_is_refused_before_any_library_call(n):
    with pytest.raises(ValueError):
        handle_less().cf_popular(n)
    with pytest.raises(ValueError):
        handle_less().cf_popular_dev(n, None, 0, 1, 1, 1, 1)


@pytest.mark.parametrize("min_total", [-1, 1 << 32, 1.5, None, "1", True])
def test_a_bad_min_total_is_refused_before_any_library_call(min_total):
    with pytest.raises(ValueError):
        handle_less().cf_popular(10, min_total=min_total)
    with pytest.raises(ValueError):
        handle_less().cf_popular_dev(10, None, 0, min_total, 1, 1, 1)


@pytest.mark.parametrize("fill", [None, 5, "123", [1, -1], [1, 1 << 32], [1.5, 2], [1.0, 2.0], [[1, 2], [3, 4]], [True, False], ["1", "2"], [1, None]])
def test_a_bad_fill_list_is_refused_before_any_library_call(fill):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filled([[1, 2, 3]], 10, fill)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_refused(k):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filled([[1, 2, 3]], k, [4, 5])
    with pytest.raises(ValueError):
        handle_less().cf_recommend_fill_dev(1, 0, 0, None, None, None, None, 0, None, 0, "cosine", 0.0, k, 0, 0, 0, 0)


def test_the_sim_calls_checks_still_hold():
    for kw in (dict(sim="cos"), dict(shrink=-1.0), dict(weights=[[1.0, -1.0, 1.0]]), dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_filled([[1, 2, 3]], 10, [4, 5], **kw)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_fill_dev(1, 0, 0, None, None, None, None, 0, None, 0, "lift", float("nan"), 10, 0, 0, 0, 0)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for n in (1, 64, 4096, np.uint32(7)):
        for min_total in (0, 1, 0xFFFFFFFF, np.uint32(3)):
            with pytest.raises(AttributeError):
                handle_less().cf_popular(n, deny=[1, 2, 70000], min_total=min_total)
            with pytest.raises(AttributeError):
                handle_less().cf_popular_dev(n, None, 0, min_total, 1, 1, 1)
    for fill in ([], (), [0, 1, 0xFFFFFFFF], np.array([4, 5], np.uint32), np.array([4, 5], np.int64), np.zeros(0, np.float64), range(5)):
        with pytest.raises(AttributeError):
            handle_less().cf_recommend_filled([[1, 2, 3], []], 10, fill, weights=[[0.0, 1.0, 2.5], []], sim="lift", shrink=0.5)
    with pytest.raises(AttributeError):
        handle_less().cf_recommend_fill_dev(1, 0, 0, None, None, None, None, 0, None, 0, "jaccard", 1.0, 10, 0, 0, 0, 0)
