"""CPU: the grouped fill call (include/smatrix_batch.h smatrix_cf_recommend_grouped_fill / _dev) is declared with its exact argument
list, exported by the library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar types, and
reachable from SparseMatrix, whose argument checks -- the grouped call's and the fill call's -- come before any library call.  No
compute calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import handle_less

NARGS = {"smatrix_cf_recommend_grouped_fill": 21, "smatrix_cf_recommend_grouped_fill_dev": 22}
DEV_ARGS = (1, 0, 0, None, None, None, None, 0, None, 0)                  # n .. group_n of cf_recommend_grouped_fill_dev


def test_the_prototypes_are_in_the_header():
    grouped, both = declared_args("smatrix_cf_recommend_grouped"), declared_args("smatrix_cf_recommend_grouped_fill")
    assert both == grouped[:12] + ["const uint32_t* fill_ids", "uint64_t n_fill"] + grouped[12:] + ["uint32_t* n_scored"]
    grouped, both = declared_args("smatrix_cf_recommend_grouped_dev"), declared_args("smatrix_cf_recommend_grouped_fill_dev")
    assert both == grouped[:12] + ["const uint32_t* d_fill_ids", "uint64_t n_fill"] + grouped[12:-1] + ["uint32_t* d_n_scored", "void* hip_stream"]
    fill = declared_args("smatrix_cf_recommend_fill")                     # ... which is the fill call's list with the map in front of the list
    assert declared_args("smatrix_cf_recommend_grouped_fill") == fill[:9] + ["const uint32_t* group_of", "uint64_t group_n", "uint32_t cap"] + fill[9:]
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name


def test_the_header_states_the_contract_and_the_grouped_call_no_longer_names_the_gap():
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    grouped = src[src.index("/* Diverse results:"):src.index("int smatrix_cf_recommend_grouped(")]
    assert "back-fill" not in grouped and "a cap per group" in grouped and "sharded matrix" in grouped
    both = re.sub(r"\s*\n \*\s*", " ", src[src.index("smatrix_cf_recommend_fill under caps"):src.index("int smatrix_cf_recommend_grouped_fill(")])
    for word in ("candidates left behind", "a filled id is still never one of the session's candidates", "does not end the walk",
                 "refused again", "makes the call smatrix_cf_recommend_fill", "smatrix_cf_recommend_grouped's bytes and n_scored = counts",
                 "a cap per group", "a fill list per session", "sharded matrix"):
        assert word in both, word


def test_the_existing_calls_are_declared_as_before():
    assert len(declared_args("smatrix_cf_recommend_sim")) == 15 and len(declared_args("smatrix_cf_recommend_sim_dev")) == 16
    assert len(declared_args("smatrix_cf_recommend_grouped")) == 18 and len(declared_args("smatrix_cf_recommend_grouped_dev")) == 19
    assert len(declared_args("smatrix_cf_recommend_fill")) == 18 and len(declared_args("smatrix_cf_recommend_fill_dev")) == 19


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
    p = inspect.signature(SparseMatrix.cf_recommend_grouped_filled).parameters
    assert list(p) == ["self", "sessions", "k", "group_of", "cap", "fill", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in list(p)[6:]] == [None, None, None, "cosine", 0.0]
    assert all(p[a].default is inspect.Parameter.empty for a in ("group_of", "cap", "fill"))
    p = inspect.signature(SparseMatrix.cf_recommend_grouped_fill_dev).parameters
    assert list(p) == ["self", "n", "off_ptr", "items_ptr", "weights_ptr", "ex_off_ptr", "ex_items_ptr", "deny_ptr", "deny_n", "group_ptr", "group_n",
                       "cap", "fill_ptr", "n_fill", "sim", "shrink", "k", "ids_ptr", "scores_ptr", "cnt_ptr", "n_scored_ptr", "stream"]
    assert p["stream"].default is None
    p = inspect.signature(SparseMatrix.cf_recommend_grouped).parameters      # the existing calls keep their signatures
    assert list(p) == ["self", "sessions", "k", "group_of", "cap", "weights", "exclude", "deny", "sim", "shrink"]
    p = inspect.signature(SparseMatrix.cf_recommend_filled).parameters
    assert list(p) == ["self", "sessions", "k", "fill", "weights", "exclude", "deny", "sim", "shrink"]


@pytest.mark.parametrize("cap", [0, 65, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_a_bad_cap_is_refused_before_any_library_call(cap):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_filled([[1, 2, 3]], 10, [0, 1, 2], cap, [4, 5])
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_fill_dev(*DEV_ARGS, cap, None, 0, "cosine", 0.0, 10, 0, 0, 0, 0)


@pytest.mark.parametrize("group_of", [5, "123", [1, -1], [1, 1 << 32], [1.5, 2], [[1, 2], [3, 4]], ["1", "2"], [1, None], {1: -1}, {-1: 1}, {1 << 32: 1},
                                      {1: 1 << 32}, {1.5: 2}, {1: "a"}])
def test_a_bad_map_is_refused_before_any_library_call(group_of):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_filled([[1, 2, 3]], 10, group_of, 2, [4, 5])


@pytest.mark.parametrize("fill", [None, 5, "123", [1, -1], [1, 1 << 32], [1.5, 2], [1.0, 2.0], [[1, 2], [3, 4]], [True, False], ["1", "2"], [1, None]])
def test_a_bad_fill_list_is_refused_before_any_library_call(fill):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_filled([[1, 2, 3]], 10, [0, 1, 2], 2, fill)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_and_the_sim_calls_checks(k):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_filled([[1, 2, 3]], k, [4, 5], 1, [6, 7])
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_fill_dev(*DEV_ARGS, 1, None, 0, "cosine", 0.0, k, 0, 0, 0, 0)
    for kw in (dict(sim="cos"), dict(shrink=-1.0), dict(weights=[[1.0, -1.0, 1.0]]), dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_grouped_filled([[1, 2, 3]], 10, [4, 5], 1, [6, 7], **kw)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_grouped_fill_dev(*DEV_ARGS, 1, None, 0, "lift", float("nan"), 10, 0, 0, 0, 0)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for group_of in (None, {}, [], [0, 1, 0xFFFFFFFF], np.array([4, 5], np.uint32), range(5), {7: 0, 0xFFFFFFFF >> 8: 0xFFFFFFFE}):
        for fill in ([], (), [0, 1, 0xFFFFFFFF], np.array([4, 5], np.int64), np.zeros(0, np.float64), range(5)):
            for cap in (1, 64, np.uint32(7)):
                with pytest.raises(AttributeError):
                    handle_less().cf_recommend_grouped_filled([[1, 2, 3], []], 10, group_of, cap, fill, weights=[[0.0, 1.0, 2.5], []], sim="lift",
                                                              shrink=0.5)
    with pytest.raises(AttributeError):
        handle_less().cf_recommend_grouped_fill_dev(*DEV_ARGS, 64, None, 0, "jaccard", 1.0, 10, 0, 0, 0, 0)
