"""tests/krylov_reference.kspcg (PETSc KSPSolve_CG + KSPConvergedDefault in
numpy, the reference of tests/test_krylov.py) pinned on the CPU: against the
oracle's own pcg_jacobi, against a direct solve, and every one of its seven end
reasons with the iteration at which it is reached."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from krylov_reference import kspcg
from oracle import tv_oracle as O


@pytest.fixture(scope="module")
def system():
    """J(T), F(T, T_prev) of a small graded 3D grid at a non-uniform state"""
    axes = [np.array([0.0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.0]), np.linspace(0.0, 1.5, 5), np.array([0.0, 0.2, 0.5, 1.0])]
    sp = O.Space(O.rectilinear_mesh(axes), "CG", 1)
    form = O.HeatForm(sp, 0.1, O.ThermalParams.from_dict(O.MAIN_MODEL_PARAMS))
    rng = np.random.default_rng(0)
    X = sp.dof_coordinates()
    T = 700.0 + 100.0 * np.cos(X[:, 0] / 3.0) + rng.uniform(-5, 5, sp.n)
    Tp = T + rng.uniform(-3, 3, sp.n)
    J = form.jacobian(T).tocsr()
    return J, form.residual(T, Tp), J.diagonal()


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.sqrt(((a - b) @ (a - b)) / (b @ b)))


def test_matches_oracle_pcg_jacobi(system):
    J, F, d = system
    x_o, k_o = O.pcg_jacobi(J, F)
    for dtype in (np.float64, np.longdouble):
        res = kspcg(J, F, lambda r: r / d, dtype=dtype)
        assert res.x[-1].dtype == dtype and res.dp[-1].dtype == dtype
        assert (res.its, res.reason) == (k_o, "CONVERGED_RTOL")
        assert len(res.x) == len(res.dp) == k_o + 1
        assert relerr(res.x[-1], x_o) < 1e-14
    assert k_o > 5


def test_tight_rtol_matches_direct_solve(system):
    J, F, d = system
    res = kspcg(J, F, lambda r: r / d, rtol=1e-13)
    assert res.reason == "CONVERGED_RTOL"
    assert relerr(res.x[-1], spla.spsolve(J.tocsc(), F)) < 1e-10


def test_history_is_the_preconditioned_residual_norm(system):
    """dp_j = ||B (b - A x_j)|| for every returned iterate (1e-12 of dp_0: the
    recurrence residual against the true one), x_0 = 0, and a solve with other
    tolerances walks the same iterates."""
    J, F, d = system
    res = kspcg(J, F, lambda r: r / d)
    assert not res.x[0].any()
    for x, dp in zip(res.x, res.dp):
        z = (F - J @ x) / d
        assert abs(np.sqrt(z @ z) - dp) < 1e-12 * res.dp[0]
    short = kspcg(J, F, lambda r: r / d, max_it=3)
    assert all(np.array_equal(a, b) for a, b in zip(short.x, res.x[:4]))


# ---- the seven reasons --------------------------------------------------------
SPD = np.diag([1.0, 2.0, 3.0, 4.0])
ONES = np.ones(4)
IDENT = lambda r: r  # noqa: E731


def _history():
    return kspcg(SPD, ONES, IDENT, rtol=1e-14)


def test_reason_converged_rtol():
    """four distinct eigenvalues: CG ends at iteration 4 (dp_4 is rounding)"""
    res = _history()
    assert (res.its, res.reason) == (4, "CONVERGED_RTOL")
    assert relerr(res.x[-1], 1.0 / np.diag(SPD)) < 1e-15


def test_reason_converged_atol():
    h = _history()
    res = kspcg(SPD, ONES, IDENT, atol=float(np.sqrt(h.dp[2] * h.dp[1])))
    assert (res.its, res.reason) == (2, "CONVERGED_ATOL")
    res = kspcg(SPD, ONES, IDENT, atol=1e300)  # before the first iteration
    assert (res.its, res.reason, len(res.x)) == (0, "CONVERGED_ATOL", 1) and not res.x[0].any()
    res = kspcg(SPD, np.zeros(4), IDENT)  # b = 0: dp_0 = 0 < atol
    assert (res.its, res.reason) == (0, "CONVERGED_ATOL")


def test_reason_diverged_its_and_convergence_at_max_it():
    """the norm test comes before the max_it test: a solve that reaches ttol at
    iteration max_it is converged, one iteration less is DIVERGED_ITS"""
    rtol = 1e-14
    assert (lambda r: (r.its, r.reason))(kspcg(SPD, ONES, IDENT, rtol=rtol, max_it=4)) == (4, "CONVERGED_RTOL")
    res = kspcg(SPD, ONES, IDENT, rtol=rtol, max_it=3)
    assert (res.its, res.reason, len(res.x)) == (3, "DIVERGED_ITS", 4)
    res = kspcg(SPD, ONES, IDENT, rtol=rtol, max_it=1)
    assert (res.its, res.reason) == (1, "DIVERGED_ITS")


def test_reason_diverged_dtol():
    h = _history()
    ratio = float(h.dp[1] / h.dp[0])
    assert 1e-5 < ratio < 1.0
    res = kspcg(SPD, ONES, IDENT, dtol=0.5 * ratio)
    assert (res.its, res.reason) == (1, "DIVERGED_DTOL")
    # the convergence test comes first: with both satisfied the solve converged
    res = kspcg(SPD, ONES, IDENT, dtol=0.5 * ratio, atol=2.0 * float(h.dp[1]))
    assert (res.its, res.reason) == (1, "CONVERGED_ATOL")


def test_reason_diverged_nanorinf():
    b = ONES.copy()
    b[2] = np.nan
    res = kspcg(SPD, b, IDENT)
    assert (res.its, res.reason) == (0, "DIVERGED_NANORINF")
    # a NaN that appears in the operator: dpi of the first pass
    A = SPD.copy()
    A[1, 1] = np.inf
    res = kspcg(A, ONES, IDENT)
    assert (res.its, res.reason, len(res.x)) == (1, "DIVERGED_NANORINF", 1)


def test_reason_diverged_indefinite_mat():
    """PETSc's test: dpi == 0, or a sign change against the previous dpi from
    the second pass on -- not dpi <= 0.  diag(1, 2, -0.5), b = 1: dpi_0 = 2.5,
    a = 1.2, r_1 = (-0.2, -1.4, 1.6), beta_1 / beta_0 = 1.52,
    p_1 = (1.32, 0.12, 3.12), dpi_1 = 1.7424 + 0.0288 - 4.8672 < 0."""
    res = kspcg(np.diag([1.0, 2.0, -0.5]), np.ones(3), IDENT)
    assert (res.its, res.reason, len(res.x)) == (2, "DIVERGED_INDEFINITE_MAT", 2)
    assert relerr(res.x[1], 1.2 * np.ones(3)) < 1e-15
    # dpi_0 = 1 + 2 - 3 = 0 in the first pass
    res = kspcg(np.diag([1.0, 2.0, -3.0]), np.ones(3), IDENT)
    assert (res.its, res.reason, len(res.x)) == (1, "DIVERGED_INDEFINITE_MAT", 1)
    # a negative definite operator keeps its sign: no indefinite end, CG solves it
    res = kspcg(-SPD, ONES, IDENT, rtol=1e-14)
    assert (res.its, res.reason) == (4, "CONVERGED_RTOL")
    assert relerr(res.x[-1], -1.0 / np.diag(SPD)) < 1e-15


def test_reason_diverged_indefinite_pc():
    """B = diag(1, 1, -1) on diag(1, 2, 3), b = 1: beta_0 = 1, a = 1/6,
    r_1 = (5, 4, 9) / 6, beta_1 = (25 + 16 - 81) / 36 < 0, found at the top of the
    second pass (dp_1 / dp_0 = 1.06: no other test fires first)."""
    w = np.array([1.0, 1.0, -1.0])
    res = kspcg(np.diag([1.0, 2.0, 3.0]), np.ones(3), lambda r: w * r)
    assert (res.its, res.reason, len(res.x)) == (2, "DIVERGED_INDEFINITE_PC", 2)
    assert relerr(res.x[1], w / 6.0) < 1e-15
    # ... and not at max_it = 1: the max_it test comes before the tests on beta
    res = kspcg(np.diag([1.0, 2.0, 3.0]), np.ones(3), lambda r: w * r, max_it=1)
    assert (res.its, res.reason) == (1, "DIVERGED_ITS")
