"""The CPU oracle with the exact exponential relaxation, without touching oracle/.

OracleProblem.visco_update calls the module-level oracle.tv_oracle.taylor_exponential(xi, lam)
and uses the result in two ways only: ``(1.0 - E)[...]`` (Eq. 15 + 20) and ``array * E[...]``
(Eq. 16).  ``exact_relaxation()`` replaces that function, for the length of a ``with`` block,
by one that returns an object holding x = xi / lam which answers those two uses with the
operations the kernel performs (csrc/tv_visco_point.h, EXACT): ``1.0 - E`` is -expm1(-x) and
``a * E`` is a * exp(-x); everything else of the expression keeps the oracle's association.
The original function is put back on exit, also when the block raises: other test modules
cache runs of the unpatched oracle.
"""
import contextlib
import functools

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


def compared_state(ref):
    """The fields of a paper oracle that the ensemble tests compare (tests/test_ensemble_paper._oracle_end,
    without its assertion), as float64 copies."""
    fc, fn, f = ref.functions_current, ref.functions_next, ref.functions
    end = {"T": fc["T"], "Tf": fc["Tf"], "Tf_partial": fc["Tf_partial"], "phi": f["phi"], "xi": f["xi"],
           "sigma": fn["sigma"], "s_partial": fc["s_partial"], "sigma_partial": fc["sigma_partial"],
           "s_tilde_partial": fc["s_tilde_partial"], "sigma_tilde_partial": fc["sigma_tilde_partial"]}
    return {k: np.array(v, dtype=np.float64) for k, v in end.items()}


@functools.lru_cache(maxsize=None)
def oracle_run(fam, bar, n_cells, n_steps, keep_every_step=False, exact=True):
    """One of the ten BARS of tests/test_ensemble.py through the paper oracle, with the exact relaxation
    unless exact=False; once per session (the record is shared: leave it unchanged).  "first_nonfinite" is
    the first step (1-based) after which a compared field is not finite, or None."""
    from test_ensemble import _coords, _params
    from test_ensemble_paper import CFGS, DT, _src
    ref = O.OracleProblem(O.rectilinear_mesh([_coords(bar, n_cells)]), (0.0, 50.0), DT, CFGS[fam], _params(bar),
                          linear="direct", model_mode="paper")
    ref.setup()
    assert np.array_equal(ref._maps[("S", "T")], _src(fam, n_cells))
    Ts, T_before, first_nonfinite = [], None, None
    with exact_relaxation() if exact else contextlib.nullcontext():
        with np.errstate(all="ignore"):
            for step in range(1, n_steps + 1):
                T_before = ref.functions_current["T"].copy()
                ref.solve_timestep()
                if keep_every_step:
                    Ts.append(ref.functions_current["T"].copy())
                if first_nonfinite is None and not all(np.all(np.isfinite(v)) for v in compared_state(ref).values()):
                    first_nonfinite = step
    return {"Ts": Ts, "T_before": T_before, "end": compared_state(ref), "first_nonfinite": first_nonfinite}
