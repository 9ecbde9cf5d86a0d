"""CPU: the grouped call (include/smatrix_batch.h smatrix_cf_recommend_grouped / _dev) is declared with its exact argument list,
exported by the library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar types, and
reachable from SparseMatrix, whose argument checks come before any library call.  No compute calls."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import handle_less

NARGS = {"smatrix_cf_recommend_grouped": 18, "smatrix_cf_recommend_grouped_dev": 19}


def test_the_prototypes_and_the_constant_are_in_the_header():
    sim, grouped = declared_args("smatrix_cf_recommend_sim"), declared_args("smatrix_cf_recommend_grouped")
    assert grouped == sim[:9] + ["const uint32_t* group_of", "uint64_t group_n", "uint32_t cap"] + sim[9:]
    sim, grouped = declared_args("smatrix_cf_recommend_sim_dev"), declared_args("smatrix_cf_recommend_grouped_dev")
    assert grouped == sim[:9] + ["const uint32_t* d_group_of", "uint64_t group_n", "uint32_t cap"] + sim[9:]
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    assert "#define SMATRIX_GROUP_NONE 0xFFFFFFFFu" in src
    for word in ("a cap per group", "smatrix_cf_recommend_fill under caps", "sharded matrix"):      # what the call does not do is said there
        assert word in src, word


def test_the_sim_call_is_declared_as_before():
    assert len(declared_args("smatrix_cf_recommend_sim")) == 15 and len(declared_args("smatrix_cf_recommend_sim_dev")) == 16


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


def test_sparse_matrix_has_the_methods_and_the_package_the_constant():
    import libsmatrix_amd
    from libsmatrix_amd import SparseMatrix
    assert libsmatrix_amd.GROUP_NONE == 0xFFFFFFFF
    p = inspect.signature(SparseMatrix.cf_recommend_grouped).parameters
    assert list(p) == ["self", "sessions", "k", "group_of", "cap", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in list(p)[5:]] == [None, None, None, "cosine", 0.0]
    assert p["group_of"].default is inspect.Parameter.empty and p["cap"].default is inspect.Parameter.empty
    p = inspect.signature(SparseMatrix.cf_recommend_grouped_dev).parameters
    assert list(p) == ["self", "n", "off_ptr", "items_ptr", "weights_ptr", "ex_off_ptr", "ex_items_ptr", "deny_ptr", "deny_n", "group_ptr", "group_n",
                       "cap", "sim", "shrink", "k", "ids_ptr", "scores_ptr", "cnt_ptr", "stream"]
    assert p["stream"].default is None
    p = inspect.signature(SparseMatrix.cf_recommend_filtered).parameters      # the existing call keeps its signature
    assert list(p) == ["self", "sessions", "k", "weights", "exclude", "deny", "sim", "shrink"]


@pytest.mark.parametrize("cap", [0, 65, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_a_bad_cap_is_refused_before_any_library_call(cap):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped([[1, 2, 3]], 10, [0, 1, 2], cap)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_dev(1, 0, 0, None, None, None, None, 0, None, 0, cap, "cosine", 0.0, 10, 0, 0, 0)


@pytest.mark.parametrize("group_of", [5, "123", [1, -1], [1, 1 << 32], [1.5, 2], [[1, 2], [3, 4]], ["1", "2"], [1, None], {1: -1}, {-1: 1}, {1 << 32: 1},
                                      {1: 1 << 32}, {1.5: 2}, {1: "a"}])
def test_a_bad_map_is_refused_before_any_library_call(group_of):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped([[1, 2, 3]], 10, group_of, 2)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_and_the_sim_calls_checks(k):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped([[1, 2, 3]], k, [4, 5], 1)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_dev(1, 0, 0, None, None, None, None, 0, None, 0, 1, "cosine", 0.0, k, 0, 0, 0)
    for kw in (dict(sim="cos"), dict(shrink=-1.0), dict(weights=[[1.0, -1.0, 1.0]]), dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_grouped([[1, 2, 3]], 10, [4, 5], 1, **kw)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for group_of in (None, {}, [], [0, 1, 0xFFFFFFFF], np.array([4, 5], np.uint32), np.array([4, 5], np.int64), range(5), {7: 0, 0xFFFFFFFF >> 8: 0xFFFFFFFE},
                     {np.uint32(3): np.uint32(4)}):
        for cap in (1, 64, np.uint32(7)):
            with pytest.raises(AttributeError):
                handle_less().cf_recommend_grouped([[1, 2, 3], []], 10, group_of, cap, weights=[[0.0, 1.0, 2.5], []], sim="lift", shrink=0.5)
    with pytest.raises(AttributeError):
        handle_less().cf_recommend_grouped_dev(1, 0, 0, None, None, None, None, 0, None, 0, 64, "jaccard", 1.0, 10, 0, 0, 0)


def test_a_dict_becomes_an_array_with_group_none_in_the_gaps():
    from libsmatrix_amd.matrix import GROUP_NONE, _group_map
    got = _group_map({5: 0, 2: 0xFFFFFFFE, 3: 7})
    assert got.dtype == np.uint32 and got.tolist() == [GROUP_NONE, GROUP_NONE, 0xFFFFFFFE, 7, GROUP_NONE, 0]
