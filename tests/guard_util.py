"""Red zones for the GPU tests (tests/test_guard_bands.py).

Two instruments, neither of which touches memory that is not mapped:

  * the library's own allocations: ``guard_env`` sets TVFEM_ALLOC_GUARD, so every
    device allocation of a context created afterwards lies between two filled
    guards (csrc/tv_alloc.cpp), and ``assert_guards_intact`` has tv_guard_check
    compare them with their fill;
  * the caller's vectors: ``guarded`` places a vector inside a larger torch
    tensor filled with NaN bit patterns, so that a kernel reading past either
    end of a caller pointer poisons its result and one writing there is seen.
"""
import ctypes as C

import numpy as np

ARENA_GUARD = 8192  # NaN doubles on each side of a guarded caller vector (64 KiB)
_FILL = -1          # all-ones bits: as a double a NaN, the fill of the library's guards of doubles


def guarded(values, lead=0):
    """(view, data_ptr, check): `values` as a float64 device vector inside a larger
    tensor filled with NaN bit patterns.  The vector's first element sits `lead`
    doubles after a 512-byte boundary (lead = 1: an 8-byte aligned, not 16-byte
    aligned pointer), its last element is the last one before the trailing NaNs,
    and at least ARENA_GUARD NaN doubles lie on each side.  check() asserts that
    every guard element still holds the fill, bit for bit."""
    import torch
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    n = v.size
    arena = torch.empty(2 * ARENA_GUARD + n + 128 + lead, dtype=torch.int64, device="cuda")
    arena.fill_(_FILL)
    first = ARENA_GUARD
    while (arena.data_ptr() + 8 * first) % 512:
        first += 1
    first += lead
    assert arena.numel() - (first + n) >= ARENA_GUARD
    view = arena.view(torch.float64)[first:first + n]
    view.copy_(torch.from_numpy(v))
    torch.cuda.synchronize()
    assert view.data_ptr() % 512 == 8 * lead

    def check():
        torch.cuda.synchronize()
        front, back = arena[:first], arena[first + n:]
        bad_f = torch.nonzero(front != _FILL).flatten()
        bad_b = torch.nonzero(back != _FILL).flatten()
        assert bad_f.numel() == 0, f"caller arena: {bad_f.numel()} guard doubles changed before the vector " \
                                   f"(nearest {first - int(bad_f.max())} before its first element)"
        assert bad_b.numel() == 0, f"caller arena: {bad_b.numel()} guard doubles changed behind the vector " \
                                   f"(nearest at offset {int(bad_b.min())} past its last element)"

    return view, view.data_ptr(), check


def guard_env(monkeypatch, kib=64):
    """Contexts created from here on guard their device allocations with `kib` KiB on each side."""
    monkeypatch.setenv("TVFEM_ALLOC_GUARD", str(kib))


def plain_env(monkeypatch):
    monkeypatch.delenv("TVFEM_ALLOC_GUARD", raising=False)


def guard_check(lib):
    """(n_guarded, n_damaged, guard_bytes) of tv_guard_check"""
    ng, nd, gb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.tv_guard_check(C.byref(ng), C.byref(nd), C.byref(gb))
    assert rc == 0, lib.tv_last_error(None)
    return ng.value, nd.value, gb.value


def assert_guards_intact(lib, kib=64):
    """The red-zone mode was on (so the test did not pass vacuously), with guards
    of at least `kib` KiB, and no guard byte of a live allocation has changed."""
    ng, nd, gb = guard_check(lib)
    assert ng > 0, "no guarded allocation is live: TVFEM_ALLOC_GUARD was not in force when the context was created"
    assert gb >= kib * 1024, (gb, kib)
    if nd:
        print("[guard]", lib.tv_last_error(None).decode())
    assert nd == 0, (nd, lib.tv_last_error(None).decode())
