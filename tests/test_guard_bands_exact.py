"""Red zones around the exact-relaxation ensemble kernels (the kModel = 2 instantiations
of csrc/tv_ensemble.hip and csrc/tv_ensemble_dg.hip, plain and scheduled): the scheme of
tests/test_guard_bands.py (its Run and _twice, imported), the cases of
tests/test_guard_bands_paper.py, both families.

Each case runs the same calls twice, with TVFEM_ALLOC_GUARD (every allocation of the
library between two NaN-filled guards) and plain, and asserts that the guards are intact
(no out-of-bounds write), that every one of the eleven state fields, every history record
and statistic has the same bits in both runs (a difference is an out-of-bounds read) and
that the guarded T agrees with the oracle (1e-10).  The kernels are new code objects with
the addressing of the paper ones; n_cells = 1 is where the clamped chunk indices of the two
sweeps are most likely to stray; 65 and 130 bars put tail lanes, a second wave and a second
workgroup next to the guards.
"""
import numpy as np
import pytest

from parity_util import relerr
from test_guard_bands import Run, _twice  # noqa: F401  (Run is what _twice hands to the case)

pytestmark = pytest.mark.gpu

N_STEPS = 8


@pytest.mark.parametrize("n_cells", [1, 3, 16])
@pytest.mark.parametrize("n_bars", [1, 65, 130])
@pytest.mark.parametrize("fam", ["cg", "dg"])
def test_ensemble_exact(fam, n_bars, n_cells, monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from exact_relaxation import oracle_run
    from test_ensemble_paper import STATE, _ensemble, _scheduled

    def run(R):
        out = {}
        ens = _ensemble(fam, [b % 10 for b in range(n_bars)], n_cells, relaxation="exact")
        ens.solve(N_STEPS)
        for f in STATE:
            out["plain/" + f] = ens.get_field(f)
        out["plain/its"] = np.asarray(ens.newton_iterations)
        out["plain/total"] = np.asarray(ens.newton_total)
        out["plain/failed"] = np.asarray(ens.failed_step)
        R.finish(ens._lib)
        ens.close()
        ens = _scheduled(fam, [b % 6 for b in range(n_bars)], n_cells, history=dict(nodes=[0, n_cells], every=2),
                         relaxation="exact")
        ens.solve(N_STEPS)
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
    nT = 2 * n_cells if fam == "dg" else n_cells + 1
    assert got["plain/T"].shape == (n_bars, nT) and got["plain/sigma"].shape == (n_bars, n_cells + 1)
    assert got["plain/s_partial"].shape == got["plain/sigma_partial"].shape == (n_bars, 6 * (n_cells + 1))
    assert got["hist/T"].shape == (4, n_bars, 2)
    assert not got["plain/failed"].any() and not got["sched/failed"].any()
    for k, v in got.items():
        assert np.all(np.isfinite(v)), k  # no NaN to hide a poisoned read behind
    ref = oracle_run(fam, 0, n_cells, N_STEPS)
    assert relerr(got["plain/T"][0], ref["end"]["T"]) <= 1e-10
