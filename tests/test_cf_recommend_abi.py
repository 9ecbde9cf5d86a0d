"""CPU: session recommendations (include/smatrix_batch.h smatrix_cf_recommend_batch / _dev) are exported by the library,
bound by the ctypes layer with the declared argument counts, and reachable from SparseMatrix, whose k check comes before any
library call.  No compute calls."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libsmatrix_amd", "lib")
NAMES = ("smatrix_cf_recommend_batch", "smatrix_cf_recommend_batch_dev")


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


def test_recommend_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(built, "smatrix.so")], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NAMES) <= syms


@pytest.mark.parametrize("name", NAMES)
def test_recommend_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(declared_args(name)) == (8 if name == "smatrix_cf_recommend_batch" else 9)


def test_sparse_matrix_has_the_recommend_methods():
    from libsmatrix_amd import SparseMatrix
    for meth in ("cf_recommend_batch", "cf_recommend_batch_dev"):
        assert callable(getattr(SparseMatrix, meth, None)), meth


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_refused_before_any_library_call(k):
    from libsmatrix_amd import SparseMatrix
    m = SparseMatrix.__new__(SparseMatrix)          # no handle, no library: only the k check can run
    with pytest.raises(ValueError):
        m.cf_recommend_batch([[1, 2, 3]], k)
    with pytest.raises(ValueError):
        m.cf_recommend_batch_dev(1, 0, 0, k, 0, 0, 0)
