"""tv_guard_check (csrc/tv_alloc.cpp), the parts that need no GPU: the symbol is
exported and bound, null arguments are refused, and with no guarded allocation
live the call reports zeros without making a HIP call (so without initialising
the GPU).  What the red zones find is tests/test_guard_bands.py's subject."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fem-glass-tempering_amd")


@pytest.fixture(scope="module")
def lib():
    from tvfem import _native as N
    return N.load_library()


def test_symbol_exported_and_bound(lib):
    from tvfem import _native as N
    assert "tv_guard_check" in N.EXPORTS
    fn = lib.tv_guard_check
    assert fn.restype is C.c_int and len(fn.argtypes) == 3
    assert all(t is C.POINTER(C.c_int64) for t in fn.argtypes)
    header = open(os.path.join(ROOT, "include", "tvfem.h")).read()
    assert "int tv_guard_check(int64_t* n_guarded, int64_t* n_damaged, int64_t* guard_bytes);" in header
    assert lib.tv_abi_version() == 8  # an additive change


def test_null_arguments_refused(lib):
    from tvfem import _native as N
    a, b, c = C.c_int64(5), C.c_int64(5), C.c_int64(5)
    for args in ((None, C.byref(b), C.byref(c)), (C.byref(a), None, C.byref(c)), (C.byref(a), C.byref(b), None),
                 (None, None, None)):
        assert lib.tv_guard_check(*args) == N.TV_ERR_ARG
        assert b"tv_guard_check" in lib.tv_last_error(None)
    assert (a.value, b.value, c.value) == (5, 5, 5)  # nothing written on a refusal


_FRESH = r"""
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
from tvfem import _native as N
os.environ["TVFEM_ALLOC_GUARD"] = "64"   # the mode on, but nothing allocated
lib = N.load_library()
a, b, c = C.c_int64(7), C.c_int64(7), C.c_int64(7)
rc = lib.tv_guard_check(C.byref(a), C.byref(b), C.byref(c))
kfd = [t for t in (os.readlink(os.path.join("/proc/self/fd", f)) for f in os.listdir("/proc/self/fd")
                   if os.path.islink(os.path.join("/proc/self/fd", f))) if t.startswith("/dev/kfd") or t.startswith("/dev/dri")]
print("RESULT", rc, a.value, b.value, c.value, len(kfd))
"""


def test_nothing_allocated_reports_zeros_without_the_gpu():
    """In a fresh process: zeros, and the GPU driver's device files were never opened
    (the HIP runtime opens them at its first call)."""
    out = subprocess.run([sys.executable, "-c", _FRESH, PKG], capture_output=True, text=True, timeout=120)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, out.stdout[-2000:] + out.stderr[-2000:]
    assert line[0].split()[1:] == ["0", "0", "0", "0", "0"], line[0]
