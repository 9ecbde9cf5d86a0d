"""CPU: smatrix_merge / smatrix_import_csr / smatrix_import_csr_dev (include/smatrix_batch.h) are declared in the header, exported
by the library, bound by the ctypes layer with the declared argument counts, and reachable from SparseMatrix.  No compute calls."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libsmatrix_amd", "lib")
CALLS = {"smatrix_merge": 5, "smatrix_import_csr": 8, "smatrix_import_csr_dev": 9}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LIBDIR, "smatrix.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    return LIBDIR


def declared_args(name):
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/smatrix_batch.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_merge_prototypes_are_in_the_header(name):
    assert len(declared_args(name)) == CALLS[name]


def test_merge_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(built, "smatrix.so")], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(CALLS) <= syms


def test_the_shim_still_carries_the_reference_symbols_only(built):
    out = subprocess.run(["nm", "--defined-only", os.path.join(built, "smatrix.o")], check=True, capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not (set(CALLS) & syms)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_merge_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(declared_args(name)) == CALLS[name]


def test_sparse_matrix_has_the_merge_methods():
    from libsmatrix_amd import SparseMatrix
    for meth in ("merge", "__iadd__", "__isub__", "import_csr", "import_csr_dev", "from_sparse_coo"):
        assert callable(getattr(SparseMatrix, meth, None)), meth


@pytest.mark.parametrize("op", ["get", "add", "", None, 0, 4, True])
def test_unknown_op_is_refused_before_any_device_call(op):
    import numpy as np
    from libsmatrix_amd import SparseMatrix
    a = SparseMatrix.__new__(SparseMatrix)          # no handles: the op is checked first
    b = SparseMatrix.__new__(SparseMatrix)
    with pytest.raises(ValueError):
        a.merge(b, op)
    with pytest.raises(ValueError):
        a.import_csr(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros((0, 2), np.uint32), op)
    with pytest.raises(ValueError):
        a.import_csr_dev(0, 0, 0, op, n_rows=0)
    with pytest.raises(ValueError):
        a.from_sparse_coo(None, op)


def test_iadd_of_something_else_is_a_type_error():
    from libsmatrix_amd import SparseMatrix
    a = SparseMatrix.__new__(SparseMatrix)
    with pytest.raises(TypeError):
        a += 3
    with pytest.raises(TypeError):
        a.merge([1, 2, 3])
