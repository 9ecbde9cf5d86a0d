"""What tests/test_merge_abi.py, test_merge_scaled_abi.py and test_merge_topk_abi.py share (a plain module, no tests of its own):
the header's declaration of a symbol, the symbol tables of the library and of the shim, the ctypes binding, and calls on
handle-less matrices, whose argument checks must fire before any handle is touched.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libsmatrix_amd", "lib")
SCALARS = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
BAD_OPS = ["get", "add", "", None, 0, 4, True]
BAD_MIN_VALUES = [-1, 1 << 32, 1.5, None]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LIBDIR, "smatrix.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    return LIBDIR


def declared_args(name):
    """the arguments of `name` as include/smatrix_batch.h declares them: ["type name", ...]"""
    src = open(os.path.join(ROOT, "include", "smatrix_batch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/smatrix_batch.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def text_symbols(path, *nm_flags):
    out = subprocess.run(["nm", *nm_flags, "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def exported(built):
    return text_symbols(os.path.join(built, "smatrix.so"), "-D")


def in_the_shim(built):
    return text_symbols(os.path.join(built, "smatrix.o"))


def assert_binding_matches_the_header(name, nargs):
    """the declared argument count, and the declared type of every scalar argument"""
    from libsmatrix_amd import _lib
    fn, args = getattr(_lib.load(), name), declared_args(name)
    assert len(fn.argtypes) == len(args) == nargs
    for bound, arg in zip(fn.argtypes, args):
        ctype = arg.rsplit(" ", 1)[0]
        assert ctype.endswith("*") or bound is SCALARS[ctype], (name, arg, bound)


def assert_methods(*methods):
    from libsmatrix_amd import SparseMatrix
    for meth in methods:
        assert callable(getattr(SparseMatrix, meth, None)), meth


def handleless():
    from libsmatrix_amd import SparseMatrix
    return SparseMatrix.__new__(SparseMatrix), SparseMatrix.__new__(SparseMatrix)      # no handles: the arguments are checked first


def assert_raises(exc, *calls):
    """every call(a, b) on two handle-less matrices raises exc"""
    for call in calls:
        a, b = handleless()
        with pytest.raises(exc):
            call(a, b)
