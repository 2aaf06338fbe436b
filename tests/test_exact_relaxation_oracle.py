"""tests/exact_relaxation.py: the helper that gives the unchanged CPU oracle the exact
exponential relaxation, the reference of the exact cells of tests/ensemble_cases.py.  No GPU.

The helper's object against numpy on x from 1e-300 to 1e3, against the Taylor polynomial
inside its remainder bound, the restore of the oracle's own function, and what the
relaxation does to the model: under the patch all ten BARS of tests/ensemble_cases.py, CG1 /
CG1 and DG1 / CG1 at 16 cells, are finite in every compared field after every one of 500
steps (measured surface sigma 0.024-0.21, 3.9e-5 on the equilibrium bar 4), while without
it bar 5 (873 K) has a non-finite sigma within 100 steps (measured: step 48, CG).
"""
import numpy as np
import pytest

from ensemble_cases import CELL, oracle_run
from exact_relaxation import ExactE, exact_exponential, exact_relaxation
from oracle import tv_oracle as O


def test_object_is_exp_and_expm1():
    x = np.concatenate([np.logspace(-300, 3, 607), [1e-300, 1e-16, 1.0, 1e3]])
    lam = 0.37
    E = exact_exponential(x * lam, lam)
    assert isinstance(E, ExactE) and E.__array_ufunc__ is None
    xq = (x * lam) / lam  # the quotient the object holds
    assert np.array_equal(E.x, xq)
    om = 1.0 - E
    assert isinstance(om, np.ndarray) and np.array_equal(om, -np.expm1(-xq))
    a = np.linspace(-2.0, 3.0, x.size)
    prod = a * E
    assert isinstance(prod, np.ndarray) and np.array_equal(prod, a * np.exp(-xq))
    # the two forms in which the oracle uses it: (1.0 - E)[:, None, None] and array * E[:, None, None]
    assert np.array_equal((1.0 - E)[:, None, None], (-np.expm1(-xq))[:, None, None])
    a3 = np.arange(x.size * 4, dtype=float).reshape(x.size, 2, 2)
    assert np.array_equal(a3 * E[:, None, None], a3 * np.exp(-xq)[:, None, None])
    # E in (0, 1] (0 only by underflow), 1 - E in [0, 1], and no digits lost where Taylor's 1 - E is 0
    e = 1.0 * E
    assert np.all(e >= 0.0) and np.all(e <= 1.0) and np.all(e[xq < 700.0] > 0.0)
    assert np.all(om > 0.0) and np.all(om <= 1.0)
    small = xq < 1e-16
    assert small.any() and np.all(1.0 - O.taylor_exponential(xq[small], 1.0) == 0.0)
    assert np.allclose(om[small], xq[small], rtol=1e-15, atol=0.0)


def test_taylor_polynomial_lies_within_its_remainder():
    """|exact - taylor_exponential| <= x^3 / 6 (1 + x) on [1e-6, 1e-2].

    The bound is the polynomial's remainder, 1.7e-19 at x = 1e-6, while both values are
    close to 1, where binary64 resolves 1.1e-16: the inequality cannot be decided on
    binary64 values below x ~ 5e-3 (measured here: |difference| up to 1.1e-16 from x = 1e-6
    on, pure rounding).  So it is asserted twice.  (a) As stated, without any allowance, at
    50 digits: the oracle's own taylor_exponential evaluated on mpmath numbers against
    mpmath's exp, at the same 401 binary64 abscissae.  (b) On the binary64 values the
    oracle and the helper actually produce, with the roundings of the two sides added and
    nothing else: exp(-x) <= 1 correctly rounded to within one ulp (2 u, u = 2^-53) and the
    polynomial's three roundings of values <= 1 (3 u).  test_object_is_exp_and_expm1 ties
    the helper's object to numpy's exp bit for bit."""
    import mpmath
    x = np.logspace(-6, -2, 401)
    with mpmath.workdps(50):
        for xv in x:
            xm = mpmath.mpf(float(xv))
            taylor = O.taylor_exponential(xm, 1.0)
            assert isinstance(taylor, mpmath.mpf)
            assert abs(mpmath.exp(-xm) - taylor) <= xm ** 3 / 6 * (1 + xm), xv
    exact = 1.0 * exact_exponential(x, 1.0)
    taylor = O.taylor_exponential(x, 1.0)
    u = 2.0 ** -53
    err = np.abs(exact - taylor)
    print(f"[exact oracle] binary64 |exact - taylor|: max over x < 1e-4 {err[x < 1e-4].max():.2e}")
    assert np.all(err <= x ** 3 / 6.0 * (1.0 + x) + 5.0 * u)


def test_original_function_is_restored():
    original = O.taylor_exponential
    with exact_relaxation():
        assert O.taylor_exponential is exact_exponential
        assert isinstance(O.taylor_exponential(np.array([0.1]), 2.0), ExactE)
    assert O.taylor_exponential is original
    with pytest.raises(RuntimeError, match="inside"):
        with exact_relaxation():
            assert O.taylor_exponential is exact_exponential
            raise RuntimeError("inside")
    assert O.taylor_exponential is original
    assert O.taylor_exponential(0.5, 1.0) == (1.0 - 0.5) + 0.125


@pytest.mark.parametrize("fam", ["cg", "dg"])
def test_all_ten_bars_stay_finite_over_500_steps(fam):
    original = O.taylor_exponential
    for bar in range(10):
        ref = oracle_run(CELL[fam + "-exact"], bar, 16, 500)
        assert ref["first_nonfinite"] is None, (fam, bar, ref["first_nonfinite"])
        for name, v in ref["end"].items():
            assert np.all(np.isfinite(v)), (fam, bar, name)
        s = ref["end"]["sigma"]
        print(f"[exact oracle] {fam} bar {bar}: sigma surface {s[0]:.4e} / {s[-1]:.4e}  max {np.abs(s).max():.4e}")
        assert np.abs(s).max() <= 1.0  # measured: at most 0.211 (bar 6)
    assert O.taylor_exponential is original


def test_taylor_bar_5_overflows_within_100_steps():
    ref = oracle_run(CELL["cg-paper"], 5, 16, 100, finite=False)
    assert ref["first_nonfinite"] is not None and ref["first_nonfinite"] <= 100
    assert not np.all(np.isfinite(ref["end"]["sigma"]))
    # and the exact relaxation keeps the same bar finite over the same steps
    assert oracle_run(CELL["cg-exact"], 5, 16, 100)["first_nonfinite"] is None
