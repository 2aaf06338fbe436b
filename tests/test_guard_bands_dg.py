"""Red zones around the DG1-temperature ensemble kernel (csrc/tv_ensemble_dg.hip):
the scheme of tests/test_guard_bands.py (its Run and _twice, imported), the
bars of tests/test_ensemble_dg.py.

Each case runs the same calls twice, with TVFEM_ALLOC_GUARD (every allocation
of the library between two NaN-filled guards) and plain, and asserts that the
guards are intact (no out-of-bounds write), that every state field, history
record and statistic has the same bits in both runs (a difference is an
out-of-bounds read) and that the guarded T agrees with the oracle (1e-10).
n_cells = 1 is where the clamped chunk indices of the two sweeps are most
likely to stray; 65 and 130 bars put tail lanes, a second wave and a second
workgroup next to the guards.
"""
import numpy as np
import pytest

from parity_util import relerr
from test_guard_bands import Run, _twice  # noqa: F401  (Run is what _twice hands to the case)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_cells", [1, 3, 16])
@pytest.mark.parametrize("n_bars", [1, 65, 130])
def test_ensemble_dg(n_bars, n_cells, monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_ensemble_dg import STATE, _ensemble, _oracle_run, _scheduled

    def run(R):
        out = {}
        ens = _ensemble([b % 10 for b in range(n_bars)], n_cells)
        ens.solve(20)
        for f in STATE:
            out["plain/" + f] = ens.get_field(f)
        out["plain/its"] = np.asarray(ens.newton_iterations)
        out["plain/total"] = np.asarray(ens.newton_total)
        out["plain/failed"] = np.asarray(ens.failed_step)
        R.finish(ens._lib)
        ens.close()
        ens = _scheduled([b % 6 for b in range(n_bars)], n_cells, history=dict(nodes=[0, n_cells], every=5))
        ens.solve(20)
        for f in STATE:
            out["sched/" + f] = ens.get_field(f)
        h = ens.get_history()
        for k in ("step", "T", "Tf", "sigma"):
            out["hist/" + k] = np.asarray(h[k])
        out["sched/total"] = np.asarray(ens.newton_total)
        out["sched/failed"] = np.asarray(ens.failed_step)
        R.finish(ens._lib)
        ens.close()
        return out

    got = _twice(monkeypatch, run)
    assert got["plain/T"].shape == (n_bars, 2 * n_cells) and got["plain/sigma"].shape == (n_bars, n_cells + 1)
    assert got["hist/T"].shape == (4, n_bars, 2)
    assert not got["plain/failed"].any() and not got["sched/failed"].any()
    ref = _oracle_run(0, n_cells, 20, False)
    assert relerr(got["plain/T"][0], ref["end"]["T"]) <= 1e-10
