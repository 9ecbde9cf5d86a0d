"""CPU: the whole-matrix export (include/smatrix_batch.h smatrix_export / smatrix_export_dev) is exported by the library,
bound by the ctypes layer with the declared argument counts, and reachable from SparseMatrix.  No compute calls."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libsmatrix_amd", "lib")


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


def test_export_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(built, "smatrix.so")], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"smatrix_export", "smatrix_export_dev"} <= syms


def test_export_orders_are_declared():
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    assert re.search(r"SMATRIX_EXPORT_TABLE\s*=\s*0", src) and re.search(r"SMATRIX_EXPORT_SORTED\s*=\s*1", src)
    from libsmatrix_amd.matrix import EXPORT_SORTED, EXPORT_TABLE
    assert (EXPORT_TABLE, EXPORT_SORTED) == (0, 1)


@pytest.mark.parametrize("name", ["smatrix_export", "smatrix_export_dev"])
def test_export_binding_matches_the_header(built, name):
    from libsmatrix_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(declared_args(name)) == (9 if name == "smatrix_export" else 10)


def test_sparse_matrix_has_the_export_methods():
    from libsmatrix_amd import SparseMatrix
    for meth in ("export", "export_dev", "to_sparse_coo"):
        assert callable(getattr(SparseMatrix, meth, None)), meth


def test_unknown_order_is_refused_before_any_device_call():
    from libsmatrix_amd import SparseMatrix
    m = SparseMatrix.__new__(SparseMatrix)          # no handle: the order is checked first
    with pytest.raises(ValueError):
        m.export("by_value")
    with pytest.raises(ValueError):
        m.export_dev("columns")
