"""ThermoViscoEnsemble(model_mode="paper", relaxation="exact"): the exact exponential
relaxation of the paper-mode bar kernels (the kModel = 2 instantiations of
csrc/tv_ensemble_step.h; EXACT in s_part of csrc/tv_visco_point.h), CG1 / CG1 and DG1 /
CG1: against the CPU oracle with the same relaxation (tests/exact_relaxation.py, the
oracle itself unchanged) bar by bar over 6 and over 500 steps, against the
relaxation="taylor" ensemble (everything but the stress is the same bits), against itself
(independence of the bars, padding lanes, splits), and the contracts of a paper ensemble
under it: failure, thermal-only steps, schedules, histories.

Tolerances and comparator are those of tests/test_ensemble_paper.py (its _check_state,
imported): T <= 1e-10 after every step; Tf and Tf_partial <= 1e-10; phi and xi <= 1e-9;
sigma and the four partial-stress fields through parity_util.check_field at 1e-6 with the
oracle's mask through the source map, the deviatoric partials measured on the volumetric
scale; every compared oracle array asserted finite.  The mask depends on the oracle's T
alone and T does not see the relaxation, so the compared fractions are those recorded
there (min_frac 0.9 CG / 0.6 DG on every bar but the equilibrium bar 4).

The 500-step case takes all ten bars (the Taylor form overflows on the five hot ones:
tests/test_ensemble_paper.py leaves them out).  Several bars sit at ambient by then and
their masked fraction is 0, so no min_frac is passed and check_field's absolute bound
carries them; in addition the unmasked relative L2 error of sigma and of sigma_partial is
<= 1e-6 per bar: in exact mode the stress is an accumulated sum and an increment's
rounding error is absolute and tiny against it.
"""
import functools

import numpy as np
import pytest

from exact_relaxation import compared_state, exact_relaxation, oracle_run
from oracle import tv_oracle as O
from parity_util import relerr
from test_ensemble import BARS
from test_ensemble_paper import (CFGS, DT, FAMS, MIN_FRAC, STATE, VISCO, _check_state, _ensemble, _own, _same,
                                 _scheduled, _src, _state, _ten, _torch)
from test_ensemble_schedule import N_STEPS, SBARS, _graded, _stage_of

pytestmark = pytest.mark.gpu

EXACT = dict(relaxation="exact")
# what the relaxation cannot touch: the T family, and the statistics
UNTOUCHED = ["T", "T_prev", "Tf", "Tf_partial", "phi", "xi"]
HOT = [b for b in range(10) if BARS[b][1] >= 850.0]  # outside the Taylor limit


def _finite_end(ref):
    for k, v in ref["end"].items():
        assert np.all(np.isfinite(v)), f"the oracle's {k} is not finite"
    return ref


# ---- 1. the patched oracle, 6 steps ----------------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_parity_with_oracle(fam, n_cells):
    _torch()
    n_steps = 6
    bars = list(range(10))
    refs = [_finite_end(oracle_run(fam, b, n_cells, n_steps, True)) for b in bars]
    ens = _ensemble(fam, bars, n_cells, **EXACT)
    assert ens.relaxation == "exact" and ens.model_mode == "paper"
    for s in range(n_steps):
        ens.solve_timestep()
        T = ens.get_field("T")
        for b in bars:
            e = relerr(T[b], refs[b]["Ts"][s])
            assert e <= 1e-10, (fam, n_cells, s, b, e)
    assert not ens.failed_step.any()
    got = _state(ens)
    ens.close()
    assert np.all(np.isfinite(got["sigma"]))
    for b in bars:
        recs = _check_state(f"exact {fam} n_cells {n_cells} bar {b}", fam, n_cells, got, b, refs[b],
                            None if b == 4 else MIN_FRAC[fam])
        if b == 4:
            assert all(r["frac"] == 0.0 for r in recs)


# ---- 2. the patched oracle, 500 steps, all ten bars; solve(250) twice ------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_long_horizon_all_ten_bars(fam):
    _torch()
    n_cells, n_steps = 16, 500
    bars = list(range(10))
    ens = _ensemble(fam, bars, n_cells, **EXACT)
    ens.solve(n_steps)
    assert abs(ens.t - 50.0) < 1e-9
    assert not ens.failed_step.any()
    got = _state(ens)
    total = ens.newton_total
    ens.close()
    assert np.all(np.isfinite(got["sigma"]))
    worst = {}
    for b in bars:
        ref = _finite_end(oracle_run(fam, b, n_cells, n_steps))
        assert ref["first_nonfinite"] is None
        assert np.abs(ref["end"]["sigma"]).max() <= 1.0  # as measured: at most 0.211 (bar 6)
        _check_state(f"exact {fam} 500 steps bar {b}", fam, n_cells, got, b, ref, None)
        for name in ("sigma", "sigma_partial"):
            e = relerr(got[name][b], ref["end"][name])
            print(f"[ensemble exact] {fam} 500 steps bar {b}: unmasked {name} rel {e:.2e}")
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1e-6, (fam, b, name, e)
    print(f"[ensemble exact] {fam} 500 steps: worst unmasked rel L2 sigma {worst['sigma']:.2e}, "
          f"sigma_partial {worst['sigma_partial']:.2e}")
    two = _ensemble(fam, bars, n_cells, **EXACT)
    two.solve(250)
    two.solve(250)
    _same(_state(two), got, "250 + 250")
    assert np.array_equal(two.newton_total, total)
    two.close()


# ---- 3. what the relaxation does not touch ---------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_only_the_stress_sees_the_relaxation(fam):
    _torch()
    n_cells = 16
    ex = _ensemble(fam, list(range(10)), n_cells, **EXACT)
    ta = _ensemble(fam, list(range(10)), n_cells, relaxation="taylor")
    assert ta.relaxation == "taylor"
    for s in range(6):
        ex.solve_timestep()
        ta.solve_timestep()
        for f in UNTOUCHED:
            assert np.array_equal(ex.get_field(f), ta.get_field(f)), (fam, s, f)
        assert np.array_equal(ex.newton_iterations, ta.newton_iterations), (fam, s)
        assert np.array_equal(ex.newton_total, ta.newton_total), (fam, s)
        assert np.array_equal(ex.failed_step, ta.failed_step), (fam, s)
    se, st = ex.get_field("sigma"), ta.get_field("sigma")
    ex.close()
    ta.close()
    assert np.all(np.isfinite(se))
    for b in HOT:
        assert not np.array_equal(se[b], st[b]), b


# ---- 4. bitwise self-consistency -------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_independence_padding_and_split(fam):
    """A bar computes the same bits alone, among ten, and repeated into tail lanes (65 bars),
    a second wave and a second workgroup (130); solve(3) + solve(5) = solve(8)."""
    _torch()
    n_cells, n_steps = 16, 8
    ten = _ensemble(fam, list(range(10)), n_cells, **EXACT)
    ten.solve(n_steps)
    want = _state(ten)
    its, total = ten.newton_iterations, ten.newton_total
    assert not ten.failed_step.any()
    ten.close()
    assert np.abs(want["sigma_partial"]).max() > 0.0 and np.abs(want["sigma_tilde_partial"]).max() > 0.0
    split = _ensemble(fam, list(range(10)), n_cells, **EXACT)
    split.solve(3)
    split.solve(5)
    _same(_state(split), want, "split")
    assert np.array_equal(split.newton_total, total)
    split.close()
    for b in range(10):
        one = _ensemble(fam, [b], n_cells, **EXACT)
        one.solve(n_steps)
        got = _state(one)
        for f in STATE:
            assert np.array_equal(got[f][0], want[f][b], equal_nan=True), (b, f)
        assert one.newton_iterations[0] == its[b] and one.newton_total[0] == total[b]
        one.close()
    for n_bars in (65, 130):
        idx = [i % 10 for i in range(n_bars)]
        rep = _ensemble(fam, idx, n_cells, **EXACT)
        rep.solve(n_steps)
        got = _state(rep)
        for f in STATE:
            assert np.array_equal(got[f], want[f][idx], equal_nan=True), (n_bars, f)
        assert np.array_equal(rep.newton_iterations, its[idx])
        assert np.array_equal(rep.newton_total, total[idx])
        rep.close()


# ---- 5. the contracts of a paper ensemble under the exact relaxation -------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_failure_semantics(fam):
    """newton_max_it = 1: every bar fails its first step, is restored and frozen, the stress
    memory stays zero.  Then two bars failed through a NaN state: the others advance bitwise."""
    _torch()
    from tvfem import NativeError
    from tvfem import _native as N
    n_cells = 16
    ens = _ensemble(fam, list(range(10)), n_cells, newton_max_it=1, **EXACT)
    init = _state(ens)
    with pytest.raises(NativeError) as exc:
        ens.solve(3)
    assert exc.value.code == N.TV_ERR_NOT_CONVERGED
    assert "bar 0" in str(exc.value) and "step 1" in str(exc.value)
    assert np.array_equal(ens.failed_step, np.ones(10, dtype=int))
    assert np.array_equal(ens.newton_iterations, np.ones(10, dtype=int))
    got = _state(ens)
    ens.close()
    assert np.array_equal(got["T"], got["T_prev"])
    for f in STATE:
        if f != "T":
            assert np.array_equal(got[f], init[f], equal_nan=True), f
    assert np.all(got["s_partial"] == 0.0) and np.all(got["sigma_partial"] == 0.0)
    good = _ensemble(fam, list(range(10)), n_cells, **EXACT)
    good.solve(3)
    want = _state(good)
    good.close()
    ens = _ensemble(fam, list(range(10)), n_cells, error_on_nonconvergence=False, **EXACT)
    T = ens.get_field("T")
    T[[2, 7]] = np.nan
    ens.set_field("T", T)
    before = _state(ens)
    ens.solve(3)
    failed = np.zeros(10, dtype=int)
    failed[[2, 7]] = 1
    assert np.array_equal(ens.failed_step, failed)
    ok = failed == 0
    got = _state(ens)
    ens.close()
    for f in STATE:
        assert np.array_equal(got[f][ok], want[f][ok], equal_nan=True), f
        if f != "T":
            assert np.array_equal(got[f][~ok], before[f][~ok], equal_nan=True), f
    assert np.array_equal(got["T"][~ok], before["T_prev"][~ok])


@pytest.mark.parametrize("fam", FAMS)
def test_thermal_only(fam):
    _torch()
    n_cells = 16
    ens = _ensemble(fam, list(range(10)), n_cells, **EXACT)
    init = _state(ens)
    ens.solve(3, thermal_only=True)
    got = _state(ens)
    assert not ens.failed_step.any()
    ens.close()
    _same(got, init, "thermal_only", VISCO)  # all nine visco fields untouched
    assert np.array_equal(got["T_prev"], got["T"])
    full = _ensemble(fam, list(range(10)), n_cells, **EXACT)
    full.solve(3)
    assert np.array_equal(full.get_field("T"), got["T"])
    full.close()


@functools.lru_cache(maxsize=None)
def _scheduled_oracle(fam, row, n_cells):
    """Bar `row` of SBARS through the patched paper oracle, its ThermalParams set to the step's stage."""
    T0, eps, L, graded, stages = SBARS[row]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=T0, epsilon=eps, htc=stages[0][1], T_ambient=stages[0][2])
    ref = O.OracleProblem(O.rectilinear_mesh([_graded(L, graded, n_cells)]), (0.0, 50.0), DT, CFGS[fam], mp,
                          linear="direct", model_mode="paper")
    ref.setup()
    Ts, T_before = [], None
    with exact_relaxation(), np.errstate(all="ignore"):
        for step in range(1, N_STEPS + 1):
            _, htc, Ta = stages[_stage_of(stages, step)]
            ref.tp.htc, ref.tp.T_ambient, ref.tp.epsilon = htc, Ta, eps
            T_before = ref.functions_current["T"].copy()
            ref.solve_timestep()
            Ts.append(ref.functions_current["T"].copy())
    return _finite_end({"Ts": Ts, "T_before": T_before, "end": compared_state(ref)})


@pytest.mark.parametrize("n_cells", [1, 3, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_schedule_parity_with_oracle(fam, n_cells):
    """The six SBARS; the mask is the oracle's T, so MIN_FRAC applies to all six as in
    tests/test_ensemble_paper.py."""
    _torch()
    rows = list(range(6))
    refs = [_scheduled_oracle(fam, r, n_cells) for r in rows]
    ens = _scheduled(fam, rows, n_cells, **EXACT)
    for s in range(N_STEPS):
        ens.solve_timestep()
        T = ens.get_field("T")
        for r in rows:
            e = relerr(T[r], refs[r]["Ts"][s])
            assert e <= 1e-10, (fam, n_cells, s, r, e)
    assert not ens.failed_step.any()
    got = _state(ens)
    ens.close()
    for r in rows:
        _check_state(f"exact {fam} scheduled n_cells {n_cells} bar {r}", fam, n_cells, got, r, refs[r], MIN_FRAC[fam])


@pytest.mark.parametrize("fam", FAMS)
def test_schedule_that_changes_nothing_changes_no_bit(fam):
    _torch()
    n_cells = 16
    plain = _ten(fam, n_cells, **EXACT)
    plain.solve(N_STEPS)
    want = _state(plain)
    plain.close()
    htc, Ta, eps = _own()
    one = [dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    three = [dict(until_step=np.arange(10) % 4, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(until_step=np.arange(10) % 4 + np.arange(10) % 3 * 2, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    for tag, sched in (("one stage", one), ("three equal stages", three)):
        ens = _ten(fam, n_cells, schedule=sched, **EXACT)
        ens.solve(N_STEPS)
        _same(_state(ens), want, tag)
        ens.close()


@pytest.mark.parametrize("n_cells", [3, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_stage_change_is_a_restart(fam, n_cells):
    """Two stages with the shared end k = 3 against two unscheduled ensembles, the second
    started from the first one's eleven state fields through get_field / set_field."""
    _torch()
    k = 3
    htc, Ta, eps = _own()
    htc2, Ta2, eps2 = htc[::-1].copy(), Ta - 40.0, np.clip(eps + 0.05, 0.0, 1.0)[::-1].copy()
    sch = _ten(fam, n_cells, schedule=[dict(until_step=k, htc=htc, T_ambient=Ta, epsilon=eps),
                                       dict(htc=htc2, T_ambient=Ta2, epsilon=eps2)], **EXACT)
    sch.solve(N_STEPS)
    got = _state(sch)
    sch.close()
    first = _ten(fam, n_cells, **EXACT)
    first.solve(k)
    mid = _state(first)
    first.close()
    assert np.abs(mid["sigma_partial"]).max() > 0.0
    second = _ten(fam, n_cells, values=(htc2, Ta2, eps2), **EXACT)
    for f in STATE:
        second.set_field(f, mid[f])
    _same(_state(second), mid, "set_field / get_field round trip")
    second.solve(N_STEPS - k)
    _same(got, _state(second), f"n_cells {n_cells}")
    second.close()


@pytest.mark.parametrize("n_cells", [1, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_history(fam, n_cells):
    """Records bitwise equal to get_field of a twin stepped `every` steps at a time; recording
    changes no state bit."""
    _torch()
    rows = list(range(6))
    probes = [0, n_cells // 2, n_cells]
    src = _src(fam, n_cells)[probes]
    ens = _scheduled(fam, rows, n_cells, history=dict(nodes=probes, every=2), **EXACT)
    ens.solve(N_STEPS)
    h = ens.get_history()
    assert np.array_equal(h["step"], [2, 4, 6, 8])
    assert h["T"].shape == h["Tf"].shape == h["sigma"].shape == (4, 6, 3)
    for name in ("T", "Tf", "sigma"):
        assert np.all(np.isfinite(h[name])), name
    twin = _scheduled(fam, rows, n_cells, **EXACT)
    for rec in range(4):
        twin.solve(2)
        assert np.array_equal(h["T"][rec], twin.get_field("T")[:, src]), rec
        assert np.array_equal(h["Tf"][rec], twin.get_field("Tf")[:, src]), rec
        assert np.array_equal(h["sigma"][rec], twin.get_field("sigma")[:, probes]), rec
    _same(_state(ens), _state(twin), "with / without a history")
    twin.close()
    ens.close()
