"""The CPU oracle with the exact exponential relaxation, without touching oracle/.

OracleProblem.visco_update calls the module-level oracle.tv_oracle.taylor_exponential(xi, lam)
and uses the result in two ways only: ``(1.0 - E)[...]`` (Eq. 15 + 20) and ``array * E[...]``
(Eq. 16).  ``exact_relaxation()`` replaces that function, for the length of a ``with`` block,
by one that returns an object holding x = xi / lam which answers those two uses with the
operations the kernel performs (csrc/tv_visco_point.h, EXACT): ``1.0 - E`` is -expm1(-x) and
``a * E`` is a * exp(-x); everything else of the expression keeps the oracle's association.
The original function is put back on exit, also when the block raises: tests/ensemble_cases.py
caches runs of the unpatched oracle beside the patched ones.
"""
import contextlib

import numpy as np

from oracle import tv_oracle as O


class ExactE:
    """exp(-x) as the oracle uses it, x = xi / lam."""
    __array_ufunc__ = None  # ndarray * ExactE and 1.0 - ExactE come here, not to numpy's broadcasting

    def __init__(self, x):
        self.x = x

    def __getitem__(self, idx):
        return ExactE(self.x[idx])

    def __rsub__(self, one):
        assert one == 1.0  # the only subtraction the oracle forms
        return -np.expm1(-self.x)

    def __rmul__(self, a):
        return a * np.exp(-self.x)


def exact_exponential(xi, lam):
    return ExactE(np.asarray(xi, dtype=np.float64) / lam)


@contextlib.contextmanager
def exact_relaxation():
    saved = O.taylor_exponential
    O.taylor_exponential = exact_exponential
    try:
        yield
    finally:
        O.taylor_exponential = saved
