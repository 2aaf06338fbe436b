"""Process schedules and probe histories of ThermoViscoEnsemble
(csrc/tv_ensemble.hip, the kExt instantiation): against the CPU oracle, whose
ThermalParams object is set to the step's stage before each solve_timestep();
against the unscheduled kernel (a schedule that changes nothing, a stage
change as a restart); against itself (splits, independence of the bars); and
the records against get_field of a twin ensemble.

Tolerances: T rel. L2 <= 1e-10 per bar at every compared step (the project's
step tolerance); phi / Tf / xi / sigma through parity_util.check_field with
its tolerances.  Of the six scheduled bars every dof is well-conditioned by
cond_mask after step 8 and the two surface nodes after every step (run through
the oracle at 1, 2, 3 and 16 cells), so min_frac applies to the end state and
to the surface probes; an interior node may move less than 1e-6 K in the first
steps, so interior records are compared in T only.  Everything else is bitwise.
"""
import functools

import numpy as np
import pytest

from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr

pytestmark = pytest.mark.gpu

CFG = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
DT = 0.1
N_STEPS = 8
STATE = ["T", "T_prev", "Tf", "Tf_partial", "phi", "xi", "sigma", "s_tilde_partial", "sigma_tilde_partial"]
# T_0, epsilon, L, graded, stages (last step, htc, T_ambient); the last stage never ends
SBARS = [
    (800.0, 0.93, 50.0, False, [(3, 280.1, 600.0), (5, 1000.0, 293.0), (None, 50.0, 293.0)]),
    (900.0, 0.9, 4.0, True, [(2, 50.0, 300.0), (2, 999.0, 999.0), (None, 600.0, 350.0)]),  # empty middle stage
    (850.0, 0.8, 6.0, False, [(0, 1.0, 1.0), (4, 1000.0, 293.0), (None, 0.0, 293.0)]),  # empty first stage
    (873.0, 0.5, 10.0, True, [(1, 120.0, 350.0), (7, 800.0, 293.0), (None, 120.0, 500.0)]),
    (920.0, 0.93, 3.0, False, [(6, 800.0, 293.0), (7, 400.0, 700.0), (None, 10.0, 293.0)]),  # a reheating stage
    (800.0, 0.93, 8.0, True, [(100, 280.1, 600.0), (200, 1.0, 1.0), (None, 1.0, 1.0)]),  # never leaves stage 0
]
# the ten bars of test_ensemble.py: htc, T_0, T_ambient, epsilon, L (odd bars graded)
BARS = [
    (280.1, 800.0, 600.0, 0.93, 50.0),
    (50.0, 900.0, 300.0, 0.9, 4.0),
    (1000.0, 850.0, 293.0, 0.8, 6.0),
    (0.0, 800.0, 600.0, 0.93, 50.0),
    (400.0, 600.0, 600.0, 0.93, 10.0),
    (120.0, 873.0, 350.0, 0.5, 19.0),
    (800.0, 920.0, 293.0, 0.93, 3.0),
    (280.1, 800.0, 600.0, 0.0, 8.0),
    (280.1, 780.0, 500.0, 0.93, 12.0),
    (600.0, 890.0, 293.0, 0.85, 5.0),
]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _graded(L, graded, n_cells):
    g = 0.5 if graded else 0.0
    s = np.linspace(0.0, 1.0, n_cells + 1)
    return L * (g * (1.0 - np.cos(np.pi * s)) / 2.0 + (1.0 - g) * s)


def _stage_of(stages, step):
    """Index of the stage that holds the 1-based step: the first whose end is not before it."""
    for j, (end, _, _) in enumerate(stages):
        if end is None or step <= end:
            return j
    raise AssertionError


# ---- the six scheduled bars ---------------------------------------------------------------
def _scheduled(rows, n_cells, schedule=True, **kw):
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    bars = [SBARS[r] for r in rows]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=np.array([b[0] for b in bars]), epsilon=np.array([b[1] for b in bars]))
    sched = None
    if schedule:
        sched = []
        for j in range(3):
            st = dict(htc=np.array([b[4][j][1] for b in bars]), T_ambient=np.array([b[4][j][2] for b in bars]))
            if j < 2:
                st["until_step"] = np.array([b[4][j][0] for b in bars])
            sched.append(st)
    meshes = [RectilinearMesh([_graded(b[2], b[3], n_cells)]) for b in bars]
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFG, mp, schedule=sched, **kw)
    ens.setup()
    return ens


@functools.lru_cache(maxsize=None)
def _oracle_run(row, n_cells):
    """Bar `row` of SBARS through the oracle, once per session: T, Tf, sigma after
    every step, T before every step, and the state after the last one."""
    T0, eps, L, graded, stages = SBARS[row]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=T0, epsilon=eps, htc=stages[0][1], T_ambient=stages[0][2])
    ref = O.OracleProblem(O.rectilinear_mesh([_graded(L, graded, n_cells)]), (0.0, 50.0), DT, CFG, mp,
                          linear="direct")
    ref.setup()
    out = {"T": [], "Tf": [], "sigma": [], "T_before": []}
    for step in range(1, N_STEPS + 1):
        _, htc, Ta = stages[_stage_of(stages, step)]
        ref.tp.htc, ref.tp.T_ambient, ref.tp.epsilon = htc, Ta, eps
        out["T_before"].append(ref.functions_current["T"].copy())
        ref.solve_timestep()
        out["T"].append(ref.functions_current["T"].copy())
        out["Tf"].append(ref.functions_current["Tf"].copy())
        out["sigma"].append(ref.functions_next["sigma"].copy())
    out["end"] = {"phi": ref.functions["phi"].copy(), "Tf": ref.functions_current["Tf"].copy(),
                  "xi": ref.functions["xi"].copy(), "sigma": ref.functions_next["sigma"].copy()}
    return out


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
def test_parity_with_oracle(n_cells):
    _torch()
    rows = list(range(6))
    refs = [_oracle_run(r, n_cells) for r in rows]
    ens = _scheduled(rows, n_cells)
    for s in range(N_STEPS):
        ens.solve_timestep()
        T = ens.get_field("T")
        for r in rows:
            e = relerr(T[r], refs[r]["T"][s])
            print(f"[schedule] n_cells {n_cells} step {s + 1} bar {r}: T rel {e:.2e}")
            assert e <= 1e-10, (n_cells, s, r, e)
    assert not ens.failed_step.any()
    for r in rows:
        mT, _ = cond_mask(refs[r]["T"][-1], refs[r]["T_before"][-1])
        for name in ("phi", "Tf", "xi", "sigma"):
            check_field(f"n_cells {n_cells} bar {r} {name}", ens.get_field(name)[r], refs[r]["end"][name], mT, 1,
                        min_frac=0.9)
    ens.close()


# ---- the ten unscheduled bars -------------------------------------------------------------
def _ten(n_cells, values=None, **kw):
    """The ten bars of BARS; `values` replaces (htc, T_ambient, epsilon) of creation."""
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    htc, Ta, eps = values if values is not None else _own()
    mp = dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=np.array([b[1] for b in BARS]), T_ambient=Ta, epsilon=eps)
    meshes = [RectilinearMesh([_graded(b[4], i % 2 == 1, n_cells)]) for i, b in enumerate(BARS)]
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFG, mp, **kw)
    ens.setup()
    return ens


def _own():
    return (np.array([b[0] for b in BARS]), np.array([b[2] for b in BARS]), np.array([b[3] for b in BARS]))


def _state(ens):
    return {f: ens.get_field(f) for f in STATE}


def _same(got, want, tag):
    for f in STATE:
        assert np.array_equal(got[f], want[f], equal_nan=True), (tag, f)


def test_schedule_that_changes_nothing_changes_no_bit():
    _torch()
    n_cells = 16
    plain = _ten(n_cells)
    plain.solve(N_STEPS)
    want = _state(plain)
    plain.close()
    htc, Ta, eps = _own()
    one = [dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    three = [dict(until_step=np.arange(10) % 4, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(until_step=np.arange(10) % 4 + np.arange(10) % 3 * 2, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    for tag, sched in (("one stage", one), ("three equal stages", three)):
        ens = _ten(n_cells, schedule=sched)
        ens.solve(N_STEPS)
        _same(_state(ens), want, tag)
        ens.close()


@pytest.mark.parametrize("n_cells", [3, 16])
def test_stage_change_is_a_restart(n_cells):
    """Two stages with the shared end k = 3 against two unscheduled ensembles: the
    first with the stage-1 values for k steps, the second with the stage-2 values
    started from the first one's nine state fields for the other 8 - k."""
    _torch()
    k = 3
    htc, Ta, eps = _own()
    htc2, Ta2, eps2 = htc[::-1].copy(), Ta - 40.0, np.clip(eps + 0.05, 0.0, 1.0)[::-1].copy()
    sch = _ten(n_cells, schedule=[dict(until_step=k, htc=htc, T_ambient=Ta, epsilon=eps),
                                  dict(htc=htc2, T_ambient=Ta2, epsilon=eps2)])
    sch.solve(N_STEPS)
    got = _state(sch)
    sch.close()
    first = _ten(n_cells)
    first.solve(k)
    mid = _state(first)
    first.close()
    second = _ten(n_cells, values=(htc2, Ta2, eps2))
    for f in STATE:
        second.set_field(f, mid[f])
    second.solve(N_STEPS - k)
    _same(got, _state(second), f"n_cells {n_cells}")
    second.close()


def test_independence_and_splits():
    """Stage ends that differ from lane to lane: solve(8) = solve(3) + solve(5), and
    every bar the same bits alone and repeated into tail lanes (65 bars), a second
    wave and a second workgroup (130)."""
    _torch()
    n_cells = 16
    rows = list(range(6))
    six = _scheduled(rows, n_cells)
    six.solve(N_STEPS)
    want = _state(six)
    six.close()
    split = _scheduled(rows, n_cells)
    split.solve(3)
    split.solve(5)
    _same(_state(split), want, "split")
    split.close()
    for r in rows:
        one = _scheduled([r], n_cells)
        one.solve(N_STEPS)
        got = _state(one)
        for f in STATE:
            assert np.array_equal(got[f][0], want[f][r], equal_nan=True), (r, f)
        one.close()
    for n_bars in (65, 130):
        idx = [i % 6 for i in range(n_bars)]
        rep = _scheduled(idx, n_cells)
        rep.solve(N_STEPS)
        got = _state(rep)
        for f in STATE:
            assert np.array_equal(got[f], want[f][idx], equal_nan=True), (n_bars, f)
        rep.close()


# ---- probe histories ----------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 16])
def test_history(n_cells):
    _torch()
    rows = list(range(6))
    probes = [0, n_cells // 2, n_cells]
    ens = _scheduled(rows, n_cells, history=dict(nodes=probes, every=2))
    ens.solve(N_STEPS)
    h = ens.get_history()
    assert np.array_equal(h["step"], [2, 4, 6, 8]) and np.allclose(h["t"], [0.2, 0.4, 0.6, 0.8])
    assert h["T"].shape == h["Tf"].shape == h["sigma"].shape == (4, 6, 3)
    twin = _scheduled(rows, n_cells)
    for rec in range(4):
        twin.solve(2)
        for name in ("T", "Tf", "sigma"):
            assert np.array_equal(h[name][rec], twin.get_field(name)[:, probes], equal_nan=True), (rec, name)
    _same(_state(ens), _state(twin), "with / without a history")  # recording changes no state bit
    twin.close()
    ens.close()
    surface = [0, 2]  # the probes at the two ends
    for r in rows:
        ref = _oracle_run(r, n_cells)
        for rec in range(4):
            s = 2 * rec + 1  # index of step 2 (rec + 1)
            e = relerr(h["T"][rec, r], ref["T"][s][probes])
            print(f"[history] n_cells {n_cells} bar {r} record {rec}: T rel {e:.2e}")
            assert e <= 1e-10, (n_cells, r, rec, e)
            mT, _ = cond_mask(ref["T"][s], ref["T_before"][s])
            check_field(f"n_cells {n_cells} bar {r} record {rec} surface sigma", h["sigma"][rec, r][surface],
                        ref["sigma"][s][probes][surface], mT[probes][surface], 1, min_frac=1.0)


def test_history_and_a_failed_bar():
    """Bar 1's T becomes NaN after step 4: its Newton loop runs to newton_max_it, the
    bar is restored and frozen at step 5 (the failure contract) and writes no record."""
    _torch()
    n_cells = 16
    rows = [0, 1, 2]
    hist = dict(nodes=[0, n_cells // 2, n_cells], every=2)
    good = _scheduled(rows, n_cells, history=hist)
    good.solve(N_STEPS)
    want, want_state = good.get_history(), _state(good)
    good.close()
    ens = _scheduled(rows, n_cells, history=hist, error_on_nonconvergence=False)
    ens.solve(4)
    T = ens.get_field("T")
    T[1] = np.nan
    ens.set_field("T", T)
    ens.solve(4)
    h = ens.get_history()
    assert np.array_equal(ens.failed_step, [0, 5, 0])
    for name in ("T", "Tf", "sigma"):
        assert h[name].shape == (4, 3, 3)
        assert np.all(np.isfinite(h[name][:2, 1])), name
        assert np.all(np.isnan(h[name][2:, 1])), name
        assert np.array_equal(h[name][:, [0, 2]], want[name][:, [0, 2]], equal_nan=True), name
    got = _state(ens)
    for f in STATE:
        assert np.array_equal(got[f][[0, 2]], want_state[f][[0, 2]], equal_nan=True), f
    ens.close()


def test_history_capacity():
    _torch()
    from tvfem import NativeError
    from tvfem import _native as N
    ens = _scheduled([0, 1, 2], 16, history=dict(nodes=[0, 16], every=2, max_records=2))
    T0 = ens.get_field("T")
    with pytest.raises(NativeError) as exc:
        ens.solve(5)
    assert exc.value.code == N.TV_ERR_STATE
    assert np.array_equal(ens.get_field("T"), T0)  # refused before any launch: no bar has advanced
    assert ens.get_history()["T"].shape == (0, 3, 2)
    ens.solve(4)
    h = ens.get_history()
    assert h["T"].shape == (2, 3, 2) and np.all(np.isfinite(h["T"]))
    ens.close()
