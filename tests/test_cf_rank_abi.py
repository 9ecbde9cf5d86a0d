"""CPU: the rank call (include/smatrix_batch.h smatrix_cf_rank / _dev) is declared with its 16 / 17 arguments and SMATRIX_RANK_NONE,
exported by the library and not by the shim, bound by the ctypes layer with the declared argument counts and scalar types, and
reachable from SparseMatrix, whose argument checks come before any library call; rank_metrics on ranks written by hand.  No compute
calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import ROOT, built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import BAD_SHRINKS, BAD_SIMS, handle_less

NARGS = {"smatrix_cf_rank": 16, "smatrix_cf_rank_dev": 17}


def test_the_prototypes_are_in_the_header():
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    args = declared_args("smatrix_cf_rank")
    assert args[:11] == declared_args("smatrix_cf_recommend_sim")[:11]               # up to shrink: the sim call's, and no k
    assert args[11:] == ["const uint64_t* t_offsets", "const uint32_t* targets", "uint32_t* ranks", "double* scores", "uint32_t* n_candidates"]
    assert declared_args("smatrix_cf_rank_dev")[-1] == "void* hip_stream"
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    assert re.search(r"^#define\s+SMATRIX_RANK_NONE\s+0xFFFFFFFFu\s*$", src, flags=re.M)


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
    assert libsmatrix_amd.RANK_NONE == 0xFFFFFFFF and callable(libsmatrix_amd.rank_metrics)
    p = inspect.signature(SparseMatrix.cf_rank).parameters
    assert list(p) == ["self", "sessions", "targets", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in ("weights", "exclude", "deny", "sim", "shrink")] == [None, None, None, "cosine", 0.0]
    p = inspect.signature(SparseMatrix.cf_rank_dev).parameters
    assert list(p) == ["self", "n", "off_ptr", "items_ptr", "weights_ptr", "ex_off_ptr", "ex_items_ptr", "deny_ptr", "deny_n", "sim", "shrink",
                       "t_off_ptr", "targets_ptr", "ranks_ptr", "scores_ptr", "ncand_ptr", "stream"]
    assert p["stream"].default is None
    p = inspect.signature(SparseMatrix.cf_evaluate).parameters
    assert p["ks"].default == (1, 10, 100) and "flatter" in SparseMatrix.cf_evaluate.__doc__


@pytest.mark.parametrize("shrink", BAD_SHRINKS)
def test_a_bad_shrink_is_refused_before_any_library_call(shrink):
    with pytest.raises(ValueError):
        handle_less().cf_rank([[1, 2, 3]], [[4]], sim="lift", shrink=shrink)
    with pytest.raises(ValueError):
        handle_less().cf_rank_dev(1, 0, 0, None, None, None, None, 0, "lift", shrink, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        handle_less().cf_evaluate([[1, 2, 3]], sim="lift", shrink=shrink)


@pytest.mark.parametrize("sim", BAD_SIMS)
def test_an_unknown_measure_is_refused_before_any_library_call(sim):
    with pytest.raises(ValueError):
        handle_less().cf_rank([[1, 2, 3]], [[4]], sim=sim)
    with pytest.raises(ValueError):
        handle_less().cf_rank_dev(1, 0, 0, None, None, None, None, 0, sim, 0.0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        handle_less().cf_evaluate([[1, 2, 3]], sim=sim)


@pytest.mark.parametrize("weights", [[[1.0, 2.0]], [[1.0, 2.0, 3.0], []], [[1.0, -0.5, 1.0]], [[1.0, float("nan"), 1.0]], [[float("inf"), 1.0, 1.0]]])
def test_bad_weights_are_refused_before_any_library_call(weights):
    with pytest.raises(ValueError):
        handle_less().cf_rank([[1, 2, 3]], [[4]], weights=weights)


@pytest.mark.parametrize("targets", [[], [[4], [5]]])
def test_a_target_list_per_session_or_a_value_error(targets):
    with pytest.raises(ValueError):
        handle_less().cf_rank([[1, 2, 3]], targets)
    with pytest.raises(ValueError):
        handle_less().cf_rank([[1, 2, 3]], [[4]], exclude=[[1], [2]])


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for sim, shrink in (("cosine", 0.0), ("jaccard", 0), ("lift", -0.0), ("lift", 10)):
        with pytest.raises(AttributeError):
            handle_less().cf_rank([[1, 2, 3], []], [[], [7, 7, 0]], weights=[[0.0, 1.0, 2.5], []], exclude=[[], [1]], deny=[5], sim=sim, shrink=shrink)
        with pytest.raises(AttributeError):
            handle_less().cf_evaluate([[1, 2, 3], [4], [5, 5]], sim=sim, shrink=shrink)


# ---- rank_metrics ------------------------------------------------------------------------------------------------------------------
def test_rank_metrics_on_ranks_written_by_hand():
    from libsmatrix_amd import RANK_NONE, rank_metrics
    ranks = np.array([0, 9, 10, RANK_NONE, 99, 100, 3, RANK_NONE], np.uint32)       # rank k - 1 is a hit at k, rank k is none
    got = rank_metrics(ranks)
    assert got["n"] == 8 and got["found"] == 6
    assert got["hit_rate"] == {1: 1 / 8, 10: 3 / 8, 100: 5 / 8}
    assert got["mrr"] == (1 / 1 + 1 / 10 + 1 / 11 + 0.0 + 1 / 100 + 1 / 101 + 1 / 4 + 0.0) / 8
    got = rank_metrics([4, 5], ks=(5, 6))
    assert got["hit_rate"] == {5: 0.5, 6: 1.0} and got["found"] == 2
    got = rank_metrics(np.array([RANK_NONE, RANK_NONE], np.uint32), ks=(1, 1 << 40))
    assert got == {"n": 2, "found": 0, "hit_rate": {1: 0.0, 1 << 40: 0.0}, "mrr": 0.0}  # no rank is no hit, at any k
    assert rank_metrics(np.zeros(0, np.uint32)) == {"n": 0, "found": 0, "hit_rate": {1: 0.0, 10: 0.0, 100: 0.0}, "mrr": 0.0}
