"""CPU: the deep call (include/smatrix_batch.h smatrix_cf_recommend_deep / _dev) is declared with the sim call's argument lists, name
for name, exported by the library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar
types, and reachable from SparseMatrix, whose argument checks come before any library call.  No compute calls."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import handle_less

NARGS = {"smatrix_cf_recommend_deep": 15, "smatrix_cf_recommend_deep_dev": 16}


def test_the_prototypes_and_the_constant_are_in_the_header():
    assert declared_args("smatrix_cf_recommend_deep") == declared_args("smatrix_cf_recommend_sim")
    assert declared_args("smatrix_cf_recommend_deep_dev") == declared_args("smatrix_cf_recommend_sim_dev")
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    assert "#define SMATRIX_DEEP_MAX 1024u" in src
    for word in ("fill lists and group quotas beyond 64", "item-neighbour calls", "sharded"):   # what the call does not do is said there
        assert word in src[src.index("SMATRIX_DEEP_MAX"):src.index("#define SMATRIX_DEEP_MAX")], word


def test_the_sim_call_is_declared_as_before():
    assert len(declared_args("smatrix_cf_recommend_sim")) == 15 and len(declared_args("smatrix_cf_recommend_sim_dev")) == 16


def test_the_symbols_are_exported(built):
    assert set(NARGS) <= exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert not set(NARGS) & in_the_shim(built)


@pytest.mark.parametrize("name", sorted(NARGS))
def test_the_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    lib = _lib.load()
    fn, args = getattr(lib, name), declared_args(name)
    assert len(fn.argtypes) == len(args) == NARGS[name]
    scalars = dict(A.SCALARS, double=C.c_double, size_t=C.c_size_t)
    for bound, arg in zip(fn.argtypes, args):
        ctype = arg.rsplit(" ", 1)[0]
        assert ctype.endswith("*") or bound is scalars[ctype], (name, arg, bound)
    assert fn.argtypes == getattr(lib, name.replace("_deep", "_sim")).argtypes


def test_sparse_matrix_has_the_methods_and_the_package_the_constant():
    import libsmatrix_amd
    from libsmatrix_amd import SparseMatrix
    assert libsmatrix_amd.DEEP_MAX == 1024
    p = inspect.signature(SparseMatrix.cf_recommend_deep).parameters
    assert list(p) == ["self", "sessions", "k", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in list(p)[3:]] == [None, None, None, "cosine", 0.0] and p["k"].default is inspect.Parameter.empty
    assert list(p) == list(inspect.signature(SparseMatrix.cf_recommend_filtered).parameters)      # the existing call keeps its signature
    assert list(inspect.signature(SparseMatrix.cf_recommend_deep_dev).parameters) == \
        list(inspect.signature(SparseMatrix.cf_recommend_sim_dev).parameters)
    assert inspect.signature(SparseMatrix.cf_recommend_deep_dev).parameters["stream"].default is None


@pytest.mark.parametrize("k", [0, 1025, -1, 1 << 32, 1.5, 65.0, None, "70", True])
def test_a_bad_k_is_refused_before_any_library_call(k):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_deep([[1, 2, 3]], k)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_deep_dev(1, 0, 0, None, None, None, None, 0, "cosine", 0.0, k, 0, 0, 0)


def test_the_sim_calls_checks_come_before_any_library_call_too():
    for kw in (dict(sim="cos"), dict(shrink=-1.0), dict(weights=[[1.0, -1.0, 1.0]]), dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_deep([[1, 2, 3]], 100, **kw)
    for kw in (dict(sim="cos"), dict(shrink=float("nan"))):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_deep_dev(1, 0, 0, None, None, None, None, 0, kw.get("sim", "lift"), kw.get("shrink", 0.0), 100, 0, 0, 0)


def test_the_existing_calls_keep_their_bound():
    for k in (65, 1024):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_filtered([[1, 2, 3]], k)
        with pytest.raises(ValueError):
            handle_less().cf_recommend_sim_dev(1, 0, 0, None, None, None, None, 0, "cosine", 0.0, k, 0, 0, 0)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for k in (1, 64, 65, 1024, np.uint32(300), np.int64(1000)):
        with pytest.raises(AttributeError):
            handle_less().cf_recommend_deep([[1, 2, 3], []], k, weights=[[0.0, 1.0, 2.5], []], exclude=[[7], []], deny=[5], sim="lift", shrink=0.5)
        with pytest.raises(AttributeError):
            handle_less().cf_recommend_deep_dev(1, 0, 0, None, None, None, None, 0, "jaccard", 1.0, k, 0, 0, 0)
