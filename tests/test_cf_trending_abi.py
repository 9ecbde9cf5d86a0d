"""CPU: the trending call (include/smatrix_batch.h smatrix_cf_trending / _dev) is declared with its exact argument lists, exported by
the library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar types, and reachable from
SparseMatrix, whose argument checks come before any library call; the C entry points refuse a missing matrix before they touch a
device.  No compute calls (the refusals on real matrices, outputs untouched, are tests/test_gpu_cf_trending.py's)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import BAD_SHRINKS, handle_less

NARGS = {"smatrix_cf_trending": 16, "smatrix_cf_trending_dev": 17}
DEV_TAIL = (None, 0, 1, 1, 1, 1, 1, 1, 1)      # deny_ptr .. n_found_ptr of cf_trending_dev


def test_the_prototypes_are_in_the_header():
    assert declared_args("smatrix_cf_trending") == [
        "smatrix_t* now", "smatrix_t* base", "int measure", "uint32_t num", "uint32_t den", "double shrink", "const uint32_t* deny_bits",
        "uint64_t deny_n", "uint32_t min_total", "uint32_t min_gain", "uint32_t n", "uint32_t* ids", "double* scores", "uint32_t* totals",
        "uint32_t* expected", "uint32_t* n_found"]
    assert declared_args("smatrix_cf_trending_dev") == [
        "smatrix_t* now", "smatrix_t* base", "int measure", "uint32_t num", "uint32_t den", "double shrink", "const uint32_t* d_deny_bits",
        "uint64_t deny_n", "uint32_t min_total", "uint32_t min_gain", "uint32_t n", "uint32_t* d_ids", "double* d_scores",
        "uint32_t* d_totals", "uint32_t* d_expected", "uint32_t* d_n_found", "void* hip_stream"]
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    assert "enum { SMATRIX_TREND_GAIN = 0, SMATRIX_TREND_RATIO = 1, SMATRIX_TREND_ZSCORE = 2 };" in src
    assert len(declared_args("smatrix_cf_popular")) == 8                  # the neighbour keeps its declaration


def test_the_symbols_are_exported_by_the_library_and_not_by_the_shim(built):
    assert set(NARGS) <= exported(built)
    assert not set(NARGS) & in_the_shim(built)                            # the shim still carries the reference's symbols only


@pytest.mark.parametrize("name", sorted(NARGS))
def test_the_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    fn, args = getattr(_lib.load(), name), declared_args(name)
    assert len(fn.argtypes) == len(args) == NARGS[name]
    scalars = dict(A.SCALARS, double=C.c_double)
    for bound, arg in zip(fn.argtypes, args):
        ctype = arg.rsplit(" ", 1)[0]
        assert ctype.endswith("*") or bound is scalars[ctype], (name, arg, bound)


def test_sparse_matrix_has_the_methods_and_their_defaults():
    import libsmatrix_amd
    from libsmatrix_amd import SparseMatrix
    assert (libsmatrix_amd.TREND_GAIN, libsmatrix_amd.TREND_RATIO, libsmatrix_amd.TREND_ZSCORE) == (0, 1, 2)
    p = inspect.signature(SparseMatrix.cf_trending).parameters
    assert list(p) == ["self", "base", "n", "measure", "num", "den", "shrink", "deny", "min_total", "min_gain"]
    assert [p[a].default for a in list(p)[3:]] == ["zscore", 1, 1, 0.0, None, 1, 1]
    p = inspect.signature(SparseMatrix.cf_trending_dev).parameters
    assert list(p) == ["self", "base", "n", "measure", "num", "den", "shrink", "deny_ptr", "deny_n", "min_total", "min_gain", "ids_ptr",
                       "scores_ptr", "totals_ptr", "expected_ptr", "n_found_ptr", "stream"]
    assert p["stream"].default is None
    from libsmatrix_amd.matrix import _trend
    assert [_trend(m) for m in ("gain", "ratio", "zscore")] == [0, 1, 2]


def both(exc, n=10, measure="zscore", num=1, den=1, shrink=0.0, base=None, **kw):
    """the call raises exc in both flavours, on matrices without handles"""
    base = handle_less() if base is None else base
    with pytest.raises(exc):
        handle_less().cf_trending(base, n, measure, num, den, shrink, **kw)
    with pytest.raises(exc):
        handle_less().cf_trending_dev(base, n, measure, num, den, shrink, None, 0, kw.get("min_total", 1), kw.get("min_gain", 1), 1, 1, 1, 1, 1)


@pytest.mark.parametrize("n", [0, 4097, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_a_bad_n_is_refused_before_any_library_call(n):
    both(ValueError, n=n)
    with pytest.raises(ValueError, match="n must be an integer in 1 .. 4096"):
        handle_less().cf_trending(handle_less(), n)


@pytest.mark.parametrize("shrink", BAD_SHRINKS)
def test_a_bad_shrink_is_refused_before_any_library_call(shrink):
    both(ValueError, shrink=shrink)
    with pytest.raises(ValueError, match="shrink must be a finite number >= 0"):
        handle_less().cf_trending(handle_less(), 10, shrink=shrink)


@pytest.mark.parametrize("measure", ["z", "cosine", "", None, 0, 2, 3, True, b"gain"])
def test_an_unknown_measure_is_refused_before_any_library_call(measure):
    both(ValueError, measure=measure)


@pytest.mark.parametrize("num,den", [(0, 1), (1, 0), (0, 0), (2, 1), (8, 7), (-1, 1), (1, 1 << 32), (1.0, 2), (1, 2.0), (None, 1), ("1", 1), (True, 1)])
def test_a_bad_scale_is_refused_before_any_library_call(num, den):
    both(ValueError, num=num, den=den)


@pytest.mark.parametrize("bad", [-1, 1 << 32, 1.5, None, "1", True])
def test_a_bad_min_total_or_min_gain_is_refused_before_any_library_call(bad):
    both(ValueError, min_total=bad)
    both(ValueError, min_gain=bad)


@pytest.mark.parametrize("base", [0, 5, "m", (1, 2), object()])
def test_a_base_that_is_no_matrix_is_refused_before_any_library_call(base):
    both(ValueError, base=base)


def test_a_base_that_is_the_matrix_itself_or_missing_is_refused():
    m = handle_less()
    with pytest.raises(ValueError):
        m.cf_trending(m, 10)
    with pytest.raises(ValueError):
        m.cf_trending_dev(m, 10, "gain", 1, 1, 0.0, *DEV_TAIL)
    with pytest.raises((ValueError, TypeError)):
        handle_less().cf_trending(None, 10)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for n in (1, 64, 4096, np.uint32(7)):
        for measure, num, den, shrink in (("gain", 1, 1, 0.0), ("ratio", 1, 7, 10), ("zscore", 3, 7, 0.1), ("zscore", np.uint32(5), 0xFFFFFFFF, -0.0)):
            with pytest.raises(AttributeError, match="'_lib'"):
                handle_less().cf_trending(handle_less(), n, measure, num, den, shrink, deny=[1, 2, 70000], min_total=0, min_gain=0xFFFFFFFF)
            with pytest.raises(AttributeError, match="'_lib'"):
                handle_less().cf_trending_dev(handle_less(), n, measure, num, den, shrink, *DEV_TAIL)


def test_the_library_refuses_missing_matrices_and_outputs_before_it_touches_a_device(built):
    """on a machine without a GPU these calls return: every refusal comes before the first lock or device call"""
    from libsmatrix_amd import _lib
    lib = _lib.load()
    ids, tot, exp, nf = (np.full(8, 0xabcdef, np.uint32) for _ in range(4))
    sc = np.full(8, 7.5)
    p32, pd = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    outs = (p32(ids), pd(sc), p32(tot), p32(exp), p32(nf))
    h = _lib.Handle()                                                     # a handle without a matrix behind it: never dereferenced
    for now, base in ((None, None), (C.pointer(h), None), (None, C.pointer(h)), (C.pointer(h), C.pointer(h))):
        assert lib.smatrix_cf_trending(now, base, 2, 1, 1, 0.0, None, 0, 1, 1, 8, *outs) == -1
        assert lib.smatrix_cf_trending_dev(now, base, 2, 1, 1, 0.0, None, 0, 1, 1, 8, None, None, None, None, None, None) == -1
    for n in (0, 4097):
        assert lib.smatrix_cf_trending(None, None, 2, 1, 1, 0.0, None, 0, 1, 1, n, *outs) == -1
    assert lib.smatrix_cf_trending(None, None, 2, 1, 1, 0.0, None, 5, 1, 1, 8, *outs) == -1
    assert all((a == 0xabcdef).all() for a in (ids, tot, exp, nf)) and (sc == 7.5).all()
