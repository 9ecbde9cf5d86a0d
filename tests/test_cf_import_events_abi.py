"""CPU: the event import (include/smatrix_batch.h smatrix_cf_import_events / _dev) is declared with its 10 / 11 arguments, exported
by the library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar types, and reachable
from SparseMatrix, whose argument checks come before any library call.  No compute calls."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import handle_less

NARGS = {"smatrix_cf_import_events": 10, "smatrix_cf_import_events_dev": 11}


def test_the_prototypes_are_in_the_header():
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    assert declared_args("smatrix_cf_import_events") == [
        "smatrix_t* self", "int op", "size_t n_sessions", "const uint64_t* offsets", "const uint32_t* ids", "const uint32_t* amounts",
        "uint32_t window", "uint32_t flags", "uint64_t max_batch", "uint64_t* n_ops"]
    assert declared_args("smatrix_cf_import_events_dev") == [
        "smatrix_t* self", "int op", "size_t n_sessions", "const uint64_t* d_offsets", "const uint32_t* d_ids", "const uint32_t* d_amounts",
        "uint32_t window", "uint32_t flags", "uint64_t max_batch", "uint64_t* n_ops", "void* hip_stream"]
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    assert "enum { SMATRIX_IMPORT_FORWARD = 1, SMATRIX_IMPORT_NO_SELF = 2 };" in src


def test_the_old_call_is_declared_as_before():
    assert declared_args("smatrix_cf_import_sessions") == ["smatrix_t* self", "size_t n_sessions", "const uint64_t* offsets", "const uint32_t* ids"]
    assert len(declared_args("smatrix_cf_import_sessions_dev")) == 7


def test_the_symbols_are_exported(built):
    assert set(NARGS) <= exported(built)


def test_the_shim_still_carries_the_reference_symbols_only(built):
    assert not set(NARGS) & in_the_shim(built)


@pytest.mark.parametrize("name", sorted(NARGS))
def test_the_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    fn, args = getattr(_lib.load(), name), declared_args(name)
    assert len(fn.argtypes) == len(args) == NARGS[name]
    scalars = dict(A.SCALARS, size_t=C.c_size_t)
    for bound, arg in zip(fn.argtypes, args):
        ctype = arg.rsplit(" ", 1)[0]
        assert ctype.endswith("*") or bound is scalars[ctype], (name, arg, bound)


def test_sparse_matrix_has_the_methods_and_their_defaults():
    import libsmatrix_amd
    from libsmatrix_amd import SparseMatrix
    assert (libsmatrix_amd.IMPORT_FORWARD, libsmatrix_amd.IMPORT_NO_SELF) == (1, 2)
    p = inspect.signature(SparseMatrix.cf_import_events).parameters
    assert list(p) == ["self", "sessions", "amounts", "window", "forward", "no_self", "forget", "max_batch"]
    assert [p[a].default for a in list(p)[2:]] == [None, 0, False, False, False, 0]
    p = inspect.signature(SparseMatrix.cf_forget_sessions).parameters
    assert list(p) == ["self", "sessions", "kw"] and p["kw"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(SparseMatrix.cf_import_events_dev).parameters
    assert list(p) == ["self", "op", "n", "off_ptr", "ids_ptr", "amounts_ptr", "window", "flags", "max_batch", "stream"]
    assert p["max_batch"].default == 0 and p["stream"].default is None


@pytest.mark.parametrize("amounts", [[[1, 2]], [[1, 2, 3], []], [], [[1, 2, 3, 4]], 5, [[[1], [2], [3]]]])
def test_a_bad_amounts_shape_is_refused_before_any_library_call(amounts):
    with pytest.raises(ValueError):
        handle_less().cf_import_events([[1, 2, 3]], amounts=amounts)
    with pytest.raises(ValueError):
        handle_less().cf_forget_sessions([[1, 2, 3]], amounts=amounts)


@pytest.mark.parametrize("amounts", [[[1, 1.5, 1]], [[1.0, 2.0, 3.0]], [[1, -1, 1]], [[1, 1 << 32, 1]], [2.5], [-1], [1 << 32], [[True, False, True]],
                                     [["1", "2", "3"]], [[1, None, 1]]])
def test_an_amount_that_is_no_uint32_is_refused_before_any_library_call(amounts):
    with pytest.raises(ValueError):
        handle_less().cf_import_events([[1, 2, 3]], amounts=amounts)


@pytest.mark.parametrize("window", [-1, 1 << 32, 1.5, None, "3", True])
def test_a_bad_window_is_refused_before_any_library_call(window):
    with pytest.raises(ValueError):
        handle_less().cf_import_events([[1, 2, 3]], window=window)
    with pytest.raises(ValueError):
        handle_less().cf_forget_sessions([[1, 2, 3]], window=window)
    with pytest.raises(ValueError):
        handle_less().cf_import_events_dev(2, 1, 0, 0, None, window, 0)


def test_an_unknown_keyword_is_refused_before_any_library_call():
    with pytest.raises(TypeError):
        handle_less().cf_import_events([[1, 2, 3]], backward=True)
    with pytest.raises(TypeError):
        handle_less().cf_forget_sessions([[1, 2, 3]], backward=True)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for amounts in (None, [[1, 0, 3], []], [2, 7], [np.array([1, 2, 3], np.uint8), np.zeros(0, np.int64)], [[0xFFFFFFFF, 0, 1], 0],
                    np.array([4, 5], np.uint32)):
        for window in (0, 1, 0xFFFFFFFF, np.uint32(7)):
            with pytest.raises(AttributeError):
                handle_less().cf_import_events([[1, 2, 3], []], amounts=amounts, window=window, forward=True, no_self=True, max_batch=64)
            with pytest.raises(AttributeError):
                handle_less().cf_forget_sessions([[1, 2, 3], []], amounts=amounts, window=window)
    with pytest.raises(AttributeError):
        handle_less().cf_import_events_dev(3, 1, 0, 0, None, 5, 3)
