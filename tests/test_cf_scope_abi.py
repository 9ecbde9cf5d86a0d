"""CPU: the scoped call (include/smatrix_batch.h smatrix_cf_recommend_scoped / _dev) is declared as smatrix_cf_recommend_grouped_fill
with its five arguments behind deny_n, exported by the library and not by the shim, bound by the ctypes layer with the declared
argument counts and scalar types, and reachable from SparseMatrix, whose argument checks come before any library call; every refusal
of the C call returns -1 without a handle.  No compute calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import merge_abi_helpers as A
from tests.merge_abi_helpers import built, declared_args, exported, in_the_shim  # noqa: F401
from tests.test_cf_sim_abi import handle_less

NARGS = {"smatrix_cf_recommend_scoped": 26, "smatrix_cf_recommend_scoped_dev": 27}
FIVE = ["const uint32_t* scope_of", "uint64_t scope_n", "const uint64_t* sc_offsets", "const uint32_t* sc_groups", "int scope_mode"]
GOOD = dict(sessions=[[1, 2, 3], []], k=10, scope_of=[0, 1, 2, 3], scope=[[1], None])


def test_the_prototypes_are_grouped_fills_with_five_arguments_behind_deny_n():
    base, new = declared_args("smatrix_cf_recommend_grouped_fill"), declared_args("smatrix_cf_recommend_scoped")
    assert base[8] == "uint64_t deny_n" and new == base[:9] + FIVE + base[9:]
    base, new = declared_args("smatrix_cf_recommend_grouped_fill_dev"), declared_args("smatrix_cf_recommend_scoped_dev")
    dev = [a.replace("* s", "* d_s") if "*" in a else a for a in FIVE]
    assert new == base[:9] + dev + base[9:] and new[-1] == "void* hip_stream"
    for name, n in NARGS.items():
        assert len(declared_args(name)) == n, name
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    assert re.search(r"#define SMATRIX_SCOPE_MAX 64\b", src) and "enum { SMATRIX_SCOPE_ONLY = 0, SMATRIX_SCOPE_EXCEPT = 1 };" in src


def test_the_header_states_the_contract_and_what_is_not_here():
    src = open(os.path.join(A.ROOT, "include", "smatrix_batch.h")).read()
    text = re.sub(r"\s*\n \*\s*", " ", src[src.index("Recommendations from these categories only"):src.index("#define SMATRIX_SCOPE_MAX")])
    for word in ("exactly as an id on the session's exclusion list", "unscoped in both modes", "matches nothing", "repeats allowed",
                 "extended by every id that is not allowed for s", "through that call's own launches", "an ungrouped id is never given",
                 "ungrouped ids pass", "its row is scanned and its weight counts", "Deterministic", "a list longer than SMATRIX_SCOPE_MAX"):
        assert word in text, word
    not_here = text[text.index("Not here:"):]
    for word in ("k > 64", "smatrix_cf_rank", "smatrix_cf_explain", "a mode per session", "sharded matrix"):
        assert word in not_here, word


def test_the_existing_calls_are_declared_as_before():
    assert len(declared_args("smatrix_cf_recommend_grouped_fill")) == 21 and len(declared_args("smatrix_cf_recommend_grouped_fill_dev")) == 22
    assert len(declared_args("smatrix_cf_recommend_sim")) == 15 and len(declared_args("smatrix_cf_recommend_fill")) == 18


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
    assert (libsmatrix_amd.SCOPE_MAX, libsmatrix_amd.SCOPE_ONLY, libsmatrix_amd.SCOPE_EXCEPT) == (64, 0, 1)
    p = inspect.signature(SparseMatrix.cf_recommend_scoped).parameters
    assert list(p) == ["self", "sessions", "k", "scope_of", "scope", "mode", "group_of", "cap", "fill", "weights", "exclude", "deny", "sim", "shrink"]
    assert [p[a].default for a in list(p)[5:]] == ["only", None, None, None, None, None, None, "cosine", 0.0]
    assert all(p[a].default is inspect.Parameter.empty for a in ("sessions", "k", "scope_of", "scope"))
    p = inspect.signature(SparseMatrix.cf_recommend_scoped_dev).parameters
    assert list(p) == ["self", "n", "off_ptr", "items_ptr", "weights_ptr", "ex_off_ptr", "ex_items_ptr", "deny_ptr", "deny_n", "scope_ptr", "scope_n",
                       "sc_off_ptr", "sc_groups_ptr", "mode", "group_ptr", "group_n", "cap", "fill_ptr", "n_fill", "sim", "shrink", "k", "ids_ptr",
                       "scores_ptr", "cnt_ptr", "n_scored_ptr", "stream"]
    assert p["stream"].default is None
    p = inspect.signature(SparseMatrix.cf_recommend_grouped_filled).parameters      # the existing call keeps its signature
    assert list(p) == ["self", "sessions", "k", "group_of", "cap", "fill", "weights", "exclude", "deny", "sim", "shrink"]


@pytest.mark.parametrize("scope", [None, [[1]], [[1], [2], [3]], 5, "ab", [[1], 5], [[1], "7"]])
def test_a_scope_of_another_shape_is_refused_before_any_library_call(scope):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_scoped(**dict(GOOD, scope=scope))


def test_a_list_longer_than_64_is_refused_before_any_library_call():
    with pytest.raises(ValueError):
        handle_less().cf_recommend_scoped(**dict(GOOD, scope=[list(range(65)), []]))
    with pytest.raises(AttributeError):                                   # 64 pass the checks: the call gets as far as the library
        handle_less().cf_recommend_scoped(**dict(GOOD, scope=[list(range(64)), []]))


@pytest.mark.parametrize("entry", [-1, 1 << 32, 1.5, "3", None, [1]])
def test_a_non_uint32_entry_is_refused_before_any_library_call(entry):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_scoped(**dict(GOOD, scope=[[1, entry], []]))


@pytest.mark.parametrize("mode", ["ONLY", "not", "", None, 0, 1, 2, True])
def test_an_unknown_mode_is_refused_before_any_library_call(mode):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_scoped(**dict(GOOD, mode=mode))
    with pytest.raises(ValueError):
        handle_less().cf_recommend_scoped_dev(1, 0, 0, None, None, None, None, 0, None, 0, None, None, mode, None, 0, 1, None, 0, "cosine", 0.0, 10,
                                              0, 0, 0, 0)


def test_the_grouped_fill_calls_checks_are_kept():
    for kw in (dict(k=0), dict(k=65), dict(cap=0, group_of=[1, 2]), dict(cap=65), dict(group_of=[1, 2]), dict(group_of=[1, -1], cap=1), dict(fill=5),
               dict(fill=[1.5]), dict(sim="cos"), dict(shrink=-1.0), dict(weights=[[1.0, -1.0, 1.0], []]), dict(exclude=[[1]]), dict(scope_of="abc"),
               dict(scope_of={1: -1})):
        with pytest.raises(ValueError):
            handle_less().cf_recommend_scoped(**dict(GOOD, **kw))


def test_good_arguments_pass_the_checks():
    """the checks refuse nothing that is allowed: the call gets as far as the library, which a handle-less object does not have"""
    for scope_of in (None, {}, [0, 1, 0xFFFFFFFF], np.array([4, 5], np.uint32), {7: 0, 99: 0xFFFFFFFE}):
        for scope in ([None, None], [[], ()], [[0xFFFFFFFF, 0, 0], np.array([3], np.int64)], [range(3), None]):
            for mode in ("only", "except"):
                with pytest.raises(AttributeError):
                    handle_less().cf_recommend_scoped([[1, 2, 3], []], 10, scope_of, scope, mode, group_of={5: 1}, cap=2, fill=[4, 5],
                                                      weights=[[0.0, 1.0, 2.5], []], sim="lift", shrink=0.5)
    with pytest.raises(AttributeError):
        handle_less().cf_recommend_scoped(**GOOD)


def test_every_refusal_returns_minus_one_without_a_handle(built):
    """the refusals stand before the handle is touched: a NULL handle, and pointers that are never followed"""
    from libsmatrix_amd import _lib
    lib = _lib.load()
    off = np.zeros(2, np.uint64)
    u = np.zeros(4, np.uint32)
    d = np.zeros(4, np.float64)
    p64, p32 = (lambda a: a.ctypes.data_as(_lib.u64p)), (lambda a: a.ctypes.data_as(_lib.u32p))
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                # noqa: E731

    def host(scope_of=True, scope_n=4, sc_off=True, sc_gr=True, mode=0, grp=True, group_n=4, cap=1, fill=True, n_fill=4, sim=0, shrink=0.0, k=4,
             nsc=True, deny_n=0, ex_off=None, n=1):
        return lib.smatrix_cf_recommend_scoped(None, n, p64(off), p32(u), None, ex_off, None, None, deny_n, p32(u) if scope_of else None, scope_n,
                                               p64(off) if sc_off else None, p32(u) if sc_gr else None, mode, p32(u) if grp else None, group_n, cap,
                                               p32(u) if fill else None, n_fill, sim, shrink, k, p32(u), pd(d), p32(u), p32(u) if nsc else None)

    def dev(scope_of=True, scope_n=4, sc_off=True, sc_gr=True, mode=0, grp=True, group_n=4, cap=1, fill=True, n_fill=4, sim=0, shrink=0.0, k=4,
            nsc=True, deny_n=0, ex_off=None, n=1):
        a = 4096                                                          # a pointer value that is never followed
        return lib.smatrix_cf_recommend_scoped_dev(None, n, a, a, None, a if ex_off is not None else None, None, None, deny_n, a if scope_of else None,
                                                   scope_n, a if sc_off else None, a if sc_gr else None, mode, a if grp else None, group_n, cap,
                                                   a if fill else None, n_fill, sim, shrink, k, a, a, a, a if nsc else None, None)

    bad = [dict(mode=2), dict(mode=-1), dict(scope_n=(1 << 32) + 1), dict(scope_of=False), dict(sc_off=False), dict(sc_gr=False),       # the scope's
           dict(sc_off=False, sc_gr=False), dict(sc_off=False, sc_gr=False, scope_of=False, scope_n=1),                                  # a map without lists
           dict(cap=0), dict(cap=65), dict(group_n=(1 << 32) + 1), dict(grp=False),                                                     # the grouped call's
           dict(nsc=False), dict(fill=False), dict(n_fill=1 << 32),                                                                     # the fill call's
           dict(sim=3), dict(shrink=-1.0), dict(shrink=float("nan")), dict(k=0), dict(k=65), dict(deny_n=5), dict(ex_off=p64(off)),     # the sim call's
           dict(n=1 << 32)]
    for case in bad:
        assert host(**case) == -1, ("host", case)
        assert dev(**case) == -1, ("dev", case)
    assert host(n=0) == 0 and dev(n=0) == 0                               # ... and nothing to do is no refusal
    assert host(n=0, sc_off=False, sc_gr=False, scope_of=False, scope_n=0) == 0
