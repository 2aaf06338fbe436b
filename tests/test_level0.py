"""Multigrid level 0 AS THE SOLVE RUNS IT, for every kind of level-0 smoother
and cycle below it (tools/bitcmp_step.CASES): the first KSPCG iterate of one
linear solve against the device's own PCApply.

In a solve x0 = omega0 B^-1 r comes from the init form of the update launch
(level0_update), in tv_precond_apply from the smooth launch (level0_smooth);
both then run the same cycle.  tests/test_krylov.py pins the in-solve path
against a reference for the CG and DG boxes; the numpy restatements pin
tv_precond_apply for every case (cg-box: tests/gmg_reference.py, dg-box:
tests/dg_gmg_reference.py, um-amg*: oracle/amg.py, umdg-aux:
tests/dg_aux_reference.py).  This ties the two entry points together:
with F = tv_residual(T), z = tv_precond_apply(F) and w = tv_jacobian_apply(z),
the iterate after one KSPCG iteration is dx = alpha z, alpha = (F.z) / (z.w).

Both sides are the device's own cycle, so nothing but rounding separates them:
1e-12, the project's "rounding only" tolerance (test_krylov.TOL["jacobi"]).
Measured (relative L2, MI355X, the same on the parent commit's library):
cg-box 1.5e-16, dg-box 2.8e-16, um-amg 9.9e-17, um-amg-structured 1.8e-16,
umdg-aux 2.6e-16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_krylov import GRIDS, TOL, bitwise, one_linear_solve, relerr
from oracle import tv_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(lib, ptr, n):
    """n doubles at a device address"""
    out = np.empty(n)
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemcpy.restype = C.c_int
    assert lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 8 * n, 2) == 0  # device to host
    return out


def _field_ptr(p, name):
    from tvfem._native import FIELD_ID
    ptr, stride = C.c_void_p(), C.c_int64()
    assert p._lib.tv_field_device_ptr(p._ctx, FIELD_ID[name], C.byref(ptr), C.byref(stride)) == 0
    return ptr.value


@pytest.mark.parametrize("case", ["cg-box", "dg-box", "um-amg", "um-amg-structured", "umdg-aux"])
def test_first_iterate_is_the_pcapply(case):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bitcmp_step as B
    kw = dict(box=GRIDS["3d"], part_axis=2) if case == "cg-box" else {}
    p = B.problem(case, model_parameters=O.MAIN_MODEL_PARAMS, ksp_fixed_its=1, **kw)
    try:
        p.setup()
        one_linear_solve(p)
        lib, ctx = p._lib, p._ctx
        X = p.functionSpaces["T"].tabulate_dof_coordinates()
        rng = np.random.default_rng(0)
        T = 700.0 + 100.0 * np.cos(X[:, 0] / 3.0) + rng.uniform(-5, 5, X.shape[0])
        p.set_field("T", T)
        p.set_field("T_prev", T + rng.uniform(-3, 3, X.shape[0]))
        p._flush()
        n = T.size
        # everything below in device layout; tv_jacobian_apply uses the context's T, which the solve moves
        T0 = _read(lib, _field_ptr(p, "T"), n)
        F, z, w = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3))
        assert lib.tv_residual(ctx, _field_ptr(p, "T"), F.data_ptr()) == 0, lib.tv_last_error(ctx)
        assert lib.tv_precond_apply(ctx, F.data_ptr(), z.data_ptr()) == 0, lib.tv_last_error(ctx)
        assert lib.tv_jacobian_apply(ctx, z.data_ptr(), w.data_ptr()) == 0, lib.tv_last_error(ctx)
        Fh, zh, wh = (v.cpu().numpy().astype(np.longdouble) for v in (F, z, w))
        alpha = (Fh @ zh) / (zh @ wh)
        assert p.solver.solve() == (1, False)
        k = p.last_krylov_iterations
        dx = _read(lib, _field_ptr(p, "dx"), n)
        T1 = _read(lib, _field_ptr(p, "T"), n)
    finally:
        p.close()
    e = relerr(dx, alpha * zh)
    print(f"[level0] {case}: n {n}, alpha {float(alpha):.6e}, first iterate vs alpha * PCApply(F) {e:.2e}")
    assert k == 1, k
    assert bitwise(T1, T0 - dx), "T_after != T_before - dx"
    assert e < TOL["jacobi"], e
