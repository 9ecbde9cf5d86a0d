"""CPU: smatrix_merge_topk (include/smatrix_batch.h) is declared in the header with its 8 arguments, exported by the library and
not by the shim, bound by the ctypes layer with the declared argument count, and reachable from SparseMatrix as merge_topk and
truncated, whose argument checks fire before any handle is touched.  No compute calls."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libsmatrix_amd", "lib")
NAME, NARGS = "smatrix_merge_topk", 8


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LIBDIR, "smatrix.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    return LIBDIR


def declared_args():
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert m, "%s is not declared in include/smatrix_batch.h" % NAME
    return [a.strip() for a in m.group(1).split(",")]


def test_the_prototype_is_in_the_header():
    args = declared_args()
    assert len(args) == NARGS, args
    assert [a.split()[-1].lstrip("*") for a in args] == ["dst", "src", "op", "m", "min_value", "max_batch", "n_ops", "n_dropped"]
    assert [" ".join(a.split()[:-1]) for a in args] == ["smatrix_t*", "smatrix_t*", "int", "uint32_t", "uint32_t", "uint64_t", "uint64_t*", "uint64_t*"]


def test_the_symbol_is_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(built, "smatrix.so")], check=True,
                         capture_output=True, text=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_the_shim_still_carries_the_reference_symbols_only(built):
    out = subprocess.run(["nm", "--defined-only", os.path.join(built, "smatrix.o")], check=True, capture_output=True, text=True).stdout
    assert NAME not in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_the_binding_matches_the_header(built):
    import ctypes as C
    from libsmatrix_amd import _lib
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == len(declared_args()) == NARGS
    assert fn.argtypes[2:6] == [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64]


def test_sparse_matrix_has_the_methods():
    from libsmatrix_amd import SparseMatrix
    for meth in ("merge_topk", "truncated"):
        assert callable(getattr(SparseMatrix, meth, None)), meth


def handleless():
    from libsmatrix_amd import SparseMatrix
    return SparseMatrix.__new__(SparseMatrix), SparseMatrix.__new__(SparseMatrix)      # no handles: the arguments are checked first


@pytest.mark.parametrize("op", ["get", "add", "", None, 0, 4, True])
def test_unknown_op_is_refused_before_any_device_call(op):
    a, b = handleless()
    with pytest.raises(ValueError):
        a.merge_topk(b, 5, op)


@pytest.mark.parametrize("m", [0, -1, 1 << 32, 1.5, 2.0, None, "3", True])
def test_bad_m_is_refused_before_any_device_call(m):
    a, b = handleless()
    with pytest.raises(ValueError):
        a.merge_topk(b, m)
    with pytest.raises(ValueError):
        a.truncated(m)


@pytest.mark.parametrize("min_value", [-1, 1 << 32, 1.5, None])
def test_bad_min_value_is_refused_before_any_device_call(min_value):
    a, b = handleless()
    with pytest.raises(ValueError):
        a.merge_topk(b, 5, "set", min_value)
    with pytest.raises(ValueError):
        a.truncated(5, min_value)


def test_something_else_than_a_matrix_is_a_type_error():
    a, _ = handleless()
    with pytest.raises(TypeError):
        a.merge_topk([1, 2, 3], 5)
    with pytest.raises(TypeError):
        a.merge_topk(3, 5, "set", 1)
