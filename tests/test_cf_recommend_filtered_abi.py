"""CPU: filtered session recommendations (include/smatrix_batch.h smatrix_cf_recommend_filtered / _dev) are exported by the
library, bound by the ctypes layer with the declared argument counts, and reachable from SparseMatrix, whose argument checks
come before any library call.  No compute calls."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libsmatrix_amd", "lib")
NARGS = {"smatrix_cf_recommend_filtered": 13, "smatrix_cf_recommend_filtered_dev": 14}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LIBDIR, "smatrix.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    return LIBDIR


def declared_args(name):
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_filtered_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(built, "smatrix.so")], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NARGS) <= syms


@pytest.mark.parametrize("name", sorted(NARGS))
def test_filtered_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(declared_args(name)) == NARGS[name]


def test_sparse_matrix_has_the_filtered_methods():
    from libsmatrix_amd import SparseMatrix
    for meth in ("cf_recommend_filtered", "cf_recommend_filtered_dev"):
        assert callable(getattr(SparseMatrix, meth, None)), meth


def handle_less():
    from libsmatrix_amd import SparseMatrix
    return SparseMatrix.__new__(SparseMatrix)       # no handle, no library: only the argument checks can run


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_refused_before_any_library_call(k):
    m = handle_less()
    with pytest.raises(ValueError):
        m.cf_recommend_filtered([[1, 2, 3]], k)
    with pytest.raises(ValueError):
        m.cf_recommend_filtered_dev(1, 0, 0, None, None, None, None, 0, k, 0, 0, 0)


@pytest.mark.parametrize("weights", [
    [[1.0, 1.0]],                       # a session's weights shorter than the session
    [[1.0, 1.0, 1.0, 1.0]],             # ... longer
    [[1.0, 1.0, 1.0], [1.0]],           # a weight sequence too many
    [],                                 # ... too few
    [[1.0, -0.5, 1.0]],                 # negative
    [[1.0, float("nan"), 1.0]],
    [[float("inf"), 1.0, 1.0]],
    [[1.0, 1.0, float("-inf")]],
])
def test_bad_weights_are_refused_before_any_library_call(weights):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filtered([[1, 2, 3]], 10, weights=weights)


@pytest.mark.parametrize("exclude", [[], [[4], [5]]])
def test_exclude_of_another_length_is_refused_before_any_library_call(exclude):
    with pytest.raises(ValueError):
        handle_less().cf_recommend_filtered([[1, 2, 3]], 10, exclude=exclude)


def test_good_arguments_pass_the_checks():
    """the checks above refuse nothing that is allowed (-0.0 and 0.0 among the weights): the call gets as far as the library,
    which a handle-less object does not have"""
    with pytest.raises(AttributeError):
        handle_less().cf_recommend_filtered([[1, 2, 3], []], 10, weights=[[0.0, -0.0, 2.5], []], exclude=[[7, 7, 0], []], deny=[3, 40])


def test_the_deny_bitmap():
    from libsmatrix_amd.matrix import _deny_bitmap
    assert _deny_bitmap([]) == (None, 0)
    bits, n = _deny_bitmap([0, 33, 33, 70])
    assert n == 71 and bits.tolist() == [1, 2, 1 << 6]
