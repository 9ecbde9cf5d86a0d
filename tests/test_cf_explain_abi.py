"""CPU: the explain call (include/smatrix_batch.h smatrix_cf_explain / _dev) is declared with its 11 / 14 arguments, exported by the
library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar types, and reachable from
SparseMatrix, whose argument checks come before any library call.  No compute calls."""
import ctypes as C
import inspect

import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import BAD_SHRINKS, BAD_SIMS, handle_less

NARGS = {"smatrix_cf_explain": 11, "smatrix_cf_explain_dev": 14}


def test_the_prototypes_are_in_the_header():
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    assert declared_args("smatrix_cf_explain") == [
        "smatrix_t* self", "size_t n_sessions", "const uint64_t* offsets", "const uint32_t* items", "const double* weights", "int sim",
        "double shrink", "const uint64_t* t_offsets", "const uint32_t* targets", "double* terms", "uint32_t* cc"]
    assert declared_args("smatrix_cf_explain_dev") == [
        "smatrix_t* self", "size_t n_sessions", "const uint64_t* d_offsets", "const uint32_t* d_items", "const double* d_weights", "int sim",
        "double shrink", "const uint64_t* d_t_offsets", "const uint32_t* d_targets", "const uint64_t* d_e_offsets", "uint64_t total",
        "double* d_terms", "uint32_t* d_cc", "void* hip_stream"]


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
    assert callable(libsmatrix_amd.explain_table)
    p = inspect.signature(libsmatrix_amd.explain_table).parameters
    assert list(p) == ["sessions", "targets", "terms", "cc", "e_offsets", "top"] and p["top"].default is None
    p = inspect.signature(SparseMatrix.cf_explain).parameters
    assert list(p) == ["self", "sessions", "targets", "weights", "sim", "shrink"]
    assert [p[a].default for a in ("weights", "sim", "shrink")] == [None, "cosine", 0.0]
    p = inspect.signature(SparseMatrix.cf_explain_dev).parameters
    assert list(p) == ["self", "n", "off_ptr", "items_ptr", "weights_ptr", "sim", "shrink", "t_off_ptr", "targets_ptr", "e_off_ptr", "total",
                       "terms_ptr", "cc_ptr", "stream"]
    assert p["stream"].default is None
    p = inspect.signature(SparseMatrix.cf_recommend_explained).parameters
    assert list(p) == ["self", "sessions", "k", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in ("weights", "exclude", "deny", "sim", "shrink")] == [None, None, None, "cosine", 0.0]


@pytest.mark.parametrize("shrink", BAD_SHRINKS)
def test_a_bad_shrink_is_refused_before_any_library_call(shrink):
    with pytest.raises(ValueError):
        handle_less().cf_explain([[1, 2, 3]], [[4]], sim="lift", shrink=shrink)
    with pytest.raises(ValueError):
        handle_less().cf_explain_dev(1, 0, 0, None, "lift", shrink, 0, 0, 0, 3, 0, 0)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_explained([[1, 2, 3]], 10, sim="lift", shrink=shrink)


@pytest.mark.parametrize("sim", BAD_SIMS)
def test_an_unknown_measure_is_refused_before_any_library_call(sim):
    with pytest.raises(ValueError):
        handle_less().cf_explain([[1, 2, 3]], [[4]], sim=sim)
    with pytest.raises(ValueError):
        handle_less().cf_explain_dev(1, 0, 0, None, sim, 0.0, 0, 0, 0, 3, 0, 0)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_explained([[1, 2, 3]], 10, sim=sim)


@pytest.mark.parametrize("weights", [[[1.0, 2.0]], [[1.0, 2.0, 3.0], []], [[1.0, -0.5, 1.0]], [[1.0, float("nan"), 1.0]], [[float("inf"), 1.0, 1.0]]])
def test_bad_weights_are_refused_before_any_library_call(weights):
    with pytest.raises(ValueError):
        handle_less().cf_explain([[1, 2, 3]], [[4]], weights=weights)
    with pytest.raises(ValueError):
        handle_less().cf_recommend_explained([[1, 2, 3]], 10, weights=weights)


@pytest.mark.parametrize("targets", [[], [[4], [5]]])
def test_a_target_list_per_session_or_a_value_error(targets):
    with pytest.raises(ValueError):
        handle_less().cf_explain([[1, 2, 3]], targets)


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for sim, shrink in (("cosine", 0.0), ("jaccard", 0), ("lift", -0.0), ("lift", 10)):
        with pytest.raises(AttributeError):
            handle_less().cf_explain([[1, 2, 3], []], [[], [7, 7, 0]], weights=[[0.0, -0.0, 2.5], []], sim=sim, shrink=shrink)
        with pytest.raises(AttributeError):
            handle_less().cf_explain_dev(1, 0, 0, None, sim, shrink, 0, 0, 0, 3, 0, 0)
        with pytest.raises(AttributeError):
            handle_less().cf_recommend_explained([[1, 2, 3], []], 10, weights=[[0.0, 1.0, 2.5], []], exclude=[[], [1]], deny=[5], sim=sim, shrink=shrink)
