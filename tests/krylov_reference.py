"""Test infrastructure (never imported by the product path): PETSc's
KSPSolve_CG with KSPConvergedDefault restated in numpy, for
tests/test_krylov_reference.py (which pins it) and tests/test_krylov.py (which
holds the five device solves against it).

    kspcg(A, b, B, rtol, atol, dtol, max_it, dtype) -> KspResult

The preconditioned norm (KSP_NORM_PRECONDITIONED, dp = ||B r||), a zero
initial guess, the symmetric inner products.  It is oracle.tv_oracle.pcg_jacobi
with any preconditioner (``B`` a callable r -> z), every iterate and the norm
history returned, a reason name instead of an exception, and PETSc's own order
of tests:

    before the first iteration   dp_0 NaN / Inf, then dp_0 <= ttol with
                                 ttol = max(rtol dp_0, atol)
    pass i (0-based)             beta == 0, then (i > 0) beta betaold < 0,
                                 p, w = A p, dpi = (p, w): NaN / Inf, then
                                 dpi == 0 or (i > 0) a sign change against the
                                 previous dpi; the update; dp NaN / Inf, then
                                 dp <= ttol, then dp >= dtol dp_0; beta = (z, r):
                                 NaN / Inf; then i + 1 >= max_it

so a solve whose norm passes ttol at iteration max_it is converged, and the
tests on beta run only if another pass follows.  The divergence test starts at
iteration 1: at iteration 0 PETSc's dp_0 >= dtol dp_0 can fire only for
dtol <= 1, which KSPSetTolerances does not take as a divergence tolerance.
``its`` is PETSc's ksp->its:
the number of updates, except for the four ends inside a pass before its
update (beta == 0, the two indefinite ones, a NaN dpi), where it is one more
than the updates applied (ksp->its = i + 1 is set at the top of the pass);
``len(x) - 1`` is always the number of updates.

dtype: np.longdouble is the reference, np.float64 the same arithmetic at the
device's precision (the rounding floor of a comparison).  A may be anything
with ``A @ p`` (a float64 scipy CSR matrix or ndarray takes long-double
vectors and returns them).
"""
from collections import namedtuple

import numpy as np

KspResult = namedtuple("KspResult", "x dp its reason")

REASONS = ("CONVERGED_RTOL", "CONVERGED_ATOL", "DIVERGED_ITS", "DIVERGED_DTOL", "DIVERGED_NANORINF",
           "DIVERGED_INDEFINITE_MAT", "DIVERGED_INDEFINITE_PC")


def _converged(dp, dp0, ttol, atol, dtol):
    """KSPConvergedDefault on the norm dp (None: go on)"""
    if not np.isfinite(dp):
        return "DIVERGED_NANORINF"
    if dp <= ttol:
        return "CONVERGED_ATOL" if dp < atol else "CONVERGED_RTOL"
    if dp >= dtol * dp0:
        return "DIVERGED_DTOL"
    return None


def kspcg(A, b, B, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000, dtype=np.longdouble):
    """x: the iterates x_0 = 0, x_1, ... (a list; the last one is the solve's
    result), dp: dp_j = ||B r_j|| for the same j, its, reason."""
    fl = dtype
    rtol, atol, dtol = fl(rtol), fl(atol), fl(dtol)
    r = np.array(b, dtype=fl)
    x = np.zeros_like(r)
    xs, dps = [x.copy()], []

    def pc(v):
        return np.asarray(B(v), dtype=fl)

    def norm(v):
        return np.sqrt(v @ v)

    z = pc(r)
    dp = dp0 = norm(z)
    dps.append(dp)
    ttol = max(rtol * dp0, atol)
    reason = _converged(dp, dp0, ttol, atol, fl(np.inf))  # no divergence test against itself
    if reason:
        return KspResult(xs, dps, 0, reason)
    beta = z @ r
    if not np.isfinite(beta):
        return KspResult(xs, dps, 0, "DIVERGED_NANORINF")
    betaold = dpi = dpiold = fl(0)
    p = None
    i = 0
    while True:
        if beta == 0:
            return KspResult(xs, dps, i + 1, "CONVERGED_ATOL")
        if i > 0 and beta * betaold < 0:
            return KspResult(xs, dps, i + 1, "DIVERGED_INDEFINITE_PC")
        p = z.copy() if i == 0 else z + (beta / betaold) * p
        dpiold = dpi
        w = np.asarray(A @ p, dtype=fl)
        dpi = p @ w
        if not np.isfinite(dpi):
            return KspResult(xs, dps, i + 1, "DIVERGED_NANORINF")
        betaold = beta
        if dpi == 0 or (i > 0 and (dpi >= 0) != (dpiold >= 0)):
            return KspResult(xs, dps, i + 1, "DIVERGED_INDEFINITE_MAT")
        a = beta / dpi
        x = x + a * p
        r = r - a * w
        z = pc(r)
        dp = norm(z)
        xs.append(x.copy())
        dps.append(dp)
        reason = _converged(dp, dp0, ttol, atol, dtol)
        if reason:
            return KspResult(xs, dps, i + 1, reason)
        beta = z @ r
        if not np.isfinite(beta):
            return KspResult(xs, dps, i + 1, "DIVERGED_NANORINF")
        i += 1
        if i >= max_it:
            return KspResult(xs, dps, i, "DIVERGED_ITS")
