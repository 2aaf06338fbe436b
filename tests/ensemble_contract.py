"""The contract of the shared ensemble step driver (ensemble_bar<Fam, kExt, kModel> of
csrc/tv_ensemble_step.h) as checks over a Cell of tests/ensemble_cases.py, which the test
modules of the six (family, model) cells call under their own test names.  A support module
(pytest does not collect it).  The checks: independence of the bars, padding lanes and launch splits, plain
and scheduled; a schedule that changes nothing; a stage change as a restart; thermal-only
steps; the failure contract; probe histories (against a twin, against the oracle, with a
failed bar, at capacity); and the shapes of the two field families.

Everything here is bitwise except the oracle parts of test_thermal_only and test_history
(T rel. L2 <= 1e-10, surface sigma through parity_util.check_field with min_frac 1.0).  An
assertion that holds in some cells only is conditioned on the Cell record: a paper handle
has a finite stress everywhere and a stress memory, a reference handle a NaN stress on the
equilibrium bar 4 and sigma = 0 until the first full step.
"""
import numpy as np
import pytest

from ensemble_cases import (BARS, N_STEPS, PAPER_ONLY, VISCO, coords, ensemble, gpu, oracle, own, params, same,
                            scheduled, scheduled_oracle_run, src, state, ten)
from parity_util import check_field, cond_mask, relerr

# ---- independence, padding, splits -----------------------------------------------------------
def independence_padding_and_split(cell):
    """A bar computes the same bits alone, among ten, and repeated into tail lanes (65
    bars), a second wave and a second workgroup (130); solve(3) + solve(5) = solve(8)."""
    gpu()
    n_cells, n_steps = 16, 8
    tenb = ensemble(cell, list(range(10)), n_cells)
    tenb.solve(n_steps)
    want = state(tenb)
    assert tuple(want) == cell.state
    its, total = tenb.newton_iterations, tenb.newton_total
    assert not tenb.failed_step.any()
    tenb.close()
    if cell.paper:  # the stress has a memory (in 1D the deviatoric strain, and with it s_partial, is exactly zero)
        assert np.abs(want["sigma_partial"]).max() > 0.0 and np.abs(want["sigma_tilde_partial"]).max() > 0.0
        assert np.all(np.isfinite(want["sigma"]))
    else:
        assert np.isnan(want["sigma"][4]).all()
    split = ensemble(cell, list(range(10)), n_cells)
    split.solve(3)
    split.solve(5)
    same(state(split), want, "split")
    assert np.array_equal(split.newton_total, total)
    split.close()
    for b in range(10):
        one = ensemble(cell, [b], n_cells)
        one.solve(n_steps)
        got = state(one)
        for f in cell.state:
            assert np.array_equal(got[f][0], want[f][b], equal_nan=True), (b, f)
        assert one.newton_iterations[0] == its[b] and one.newton_total[0] == total[b]
        one.close()
    for n_bars in (65, 130):
        idx = [i % 10 for i in range(n_bars)]
        rep = ensemble(cell, idx, n_cells)
        rep.solve(n_steps)
        got = state(rep)
        for f in cell.state:
            assert np.array_equal(got[f], want[f][idx], equal_nan=True), (n_bars, f)
        assert np.array_equal(rep.newton_iterations, its[idx])
        assert np.array_equal(rep.newton_total, total[idx])
        assert not rep.failed_step.any()
        rep.close()


def scheduled_independence_and_splits(cell):
    """Stage ends that differ from lane to lane: solve(8) = solve(3) + solve(5), and
    every bar the same bits alone and repeated into tail lanes (65 bars), a second
    wave and a second workgroup (130)."""
    gpu()
    n_cells = 16
    rows = list(range(6))
    six = scheduled(cell, rows, n_cells)
    six.solve(N_STEPS)
    want, total = state(six), six.newton_total
    six.close()
    split = scheduled(cell, rows, n_cells)
    split.solve(3)
    split.solve(5)
    same(state(split), want, "split")
    assert np.array_equal(split.newton_total, total)
    split.close()
    for r in rows:
        one = scheduled(cell, [r], n_cells)
        one.solve(N_STEPS)
        got = state(one)
        for f in cell.state:
            assert np.array_equal(got[f][0], want[f][r], equal_nan=True), (r, f)
        one.close()
    for n_bars in (65, 130):
        idx = [i % 6 for i in range(n_bars)]
        rep = scheduled(cell, idx, n_cells)
        rep.solve(N_STEPS)
        got = state(rep)
        for f in cell.state:
            assert np.array_equal(got[f], want[f][idx], equal_nan=True), (n_bars, f)
        rep.close()


# ---- schedules against the unscheduled kernel ------------------------------------------------
def schedule_that_changes_nothing_changes_no_bit(cell):
    gpu()
    n_cells = 16
    plain = ten(cell, n_cells)
    plain.solve(N_STEPS)
    want = state(plain)
    plain.close()
    htc, Ta, eps = own()
    one = [dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    three = [dict(until_step=np.arange(10) % 4, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(until_step=np.arange(10) % 4 + np.arange(10) % 3 * 2, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    for tag, sched in (("one stage", one), ("three equal stages", three)):
        ens = ten(cell, n_cells, schedule=sched)
        ens.solve(N_STEPS)
        same(state(ens), want, tag)
        ens.close()


def stage_change_is_a_restart(cell, n_cells):
    """Two stages with the shared end k = 3 against two unscheduled ensembles: the first
    with the stage-1 values for k steps, the second with the stage-2 values started from
    the first one's state fields (get_field / set_field) for the other 8 - k."""
    gpu()
    k = 3
    htc, Ta, eps = own()
    htc2, Ta2, eps2 = htc[::-1].copy(), Ta - 40.0, np.clip(eps + 0.05, 0.0, 1.0)[::-1].copy()
    sch = ten(cell, n_cells, schedule=[dict(until_step=k, htc=htc, T_ambient=Ta, epsilon=eps),
                                       dict(htc=htc2, T_ambient=Ta2, epsilon=eps2)])
    sch.solve(N_STEPS)
    got = state(sch)
    sch.close()
    first = ten(cell, n_cells)
    first.solve(k)
    mid = state(first)
    first.close()
    if cell.paper:
        # (s_partial is exactly zero in 1D, no deviatoric strain: its set_field is shown to move values in
        # test_partial_stress_fields_exist_only_on_a_paper_handle)
        assert np.abs(mid["sigma_partial"]).max() > 0.0
    second = ten(cell, n_cells, values=(htc2, Ta2, eps2))
    for f in cell.state:
        second.set_field(f, mid[f])
    same(state(second), mid, "set_field / get_field round trip")
    second.solve(N_STEPS - k)
    same(got, state(second), f"n_cells {n_cells}")
    second.close()


# ---- thermal-only steps ----------------------------------------------------------------------
def thermal_only(cell):
    gpu()
    n_cells = 16
    ens = ensemble(cell, list(range(10)), n_cells)
    init = state(ens)
    ens.solve(3, thermal_only=True)
    got = state(ens)
    assert not ens.failed_step.any()
    ens.close()
    same(got, init, "thermal_only", VISCO + (PAPER_ONLY if cell.paper else []))  # every visco field untouched
    assert np.array_equal(got["T_prev"], got["T"])
    if not cell.paper:
        assert np.all(got["sigma"] == 0.0)
    full = ensemble(cell, list(range(10)), n_cells)
    full.solve(3)
    assert np.array_equal(full.get_field("T"), got["T"])
    full.close()
    if not cell.paper:  # the oracle's own thermal-only steps (T does not see the model: the reference cells' part)
        for b in range(10):
            ref = oracle(cell, coords(b, n_cells), params(b), n_cells)
            ref.solve(3, thermal_only=True)
            e = relerr(got["T"][b], ref.functions_current["T"])
            assert e <= 1e-10, (b, e)


# ---- the failure contract --------------------------------------------------------------------
def failure_semantics(cell, error_on_nonconvergence):
    """newton_max_it = 1: the incremental criterion cannot converge at iteration 1, so every
    bar fails its first step, is restored and frozen: a failed step writes only T <- T_prev.
    Then two bars failed through a NaN state: the others advance bitwise as without them."""
    gpu()
    from tvfem import NativeError
    from tvfem import _native as N
    n_cells = 16
    ens = ensemble(cell, list(range(10)), n_cells, newton_max_it=1, error_on_nonconvergence=error_on_nonconvergence)
    init = state(ens)
    if error_on_nonconvergence:
        with pytest.raises(NativeError) as exc:
            ens.solve(3)
        assert exc.value.code == N.TV_ERR_NOT_CONVERGED
        assert "bar 0" in str(exc.value) and "step 1" in str(exc.value)
    else:
        ens.solve(3)
    assert np.array_equal(ens.failed_step, np.ones(10, dtype=int))
    assert np.array_equal(ens.newton_iterations, np.ones(10, dtype=int))
    got = state(ens)
    ens.close()
    assert np.array_equal(got["T"], got["T_prev"])  # T <- T_prev
    for f in cell.state:
        if f != "T":  # the visco state and T_prev are untouched, bit for bit
            assert np.array_equal(got[f], init[f], equal_nan=True), f
    assert np.all(got["Tf"] == np.array([b[1] for b in BARS])[:, None])  # Tf stays T_0
    if cell.paper:
        assert np.all(got["s_partial"] == 0.0) and np.all(got["sigma_partial"] == 0.0)
    # bar 4: zero residual, zero increment -- T too is still the initial condition
    assert np.array_equal(got["T"][4], init["T"][4])
    assert np.all(init["T"][4] == BARS[4][1]) and np.all(init["T_prev"][4] == BARS[4][1])
    # bars 2 and 7 fail at step 1 (NaN never converges), the others advance as if alone with them
    good = ensemble(cell, list(range(10)), n_cells)
    good.solve(3)
    want = state(good)
    good.close()
    ens = ensemble(cell, list(range(10)), n_cells, error_on_nonconvergence=error_on_nonconvergence)
    T = ens.get_field("T")
    T[[2, 7]] = np.nan
    ens.set_field("T", T)
    before = state(ens)
    if error_on_nonconvergence:
        with pytest.raises(NativeError) as exc:
            ens.solve(3)
        assert exc.value.code == N.TV_ERR_NOT_CONVERGED and "bar 2" in str(exc.value)
    else:
        ens.solve(3)
    failed = np.zeros(10, dtype=int)
    failed[[2, 7]] = 1
    assert np.array_equal(ens.failed_step, failed)
    ok = failed == 0
    got = state(ens)
    ens.close()
    for f in cell.state:
        assert np.array_equal(got[f][ok], want[f][ok], equal_nan=True), f
        if f != "T":
            assert np.array_equal(got[f][~ok], before[f][~ok], equal_nan=True), f
    assert np.array_equal(got["T"][~ok], before["T_prev"][~ok])


# ---- probe histories -------------------------------------------------------------------------
def history(cell, n_cells):
    """Records bitwise equal to get_field of a twin stepped `every` steps at a time: T and
    Tf at the probe node's source dof, sigma at the node; recording changes no state bit;
    and the recorded T is the oracle's."""
    gpu()
    rows = list(range(6))
    probes = [0, n_cells // 2, n_cells]
    sdof = src(cell.fam, n_cells)[probes]
    ens = scheduled(cell, rows, n_cells, history=dict(nodes=probes, every=2))
    ens.solve(N_STEPS)
    h = ens.get_history()
    assert np.array_equal(h["step"], [2, 4, 6, 8]) and np.allclose(h["t"], [0.2, 0.4, 0.6, 0.8])
    assert h["T"].shape == h["Tf"].shape == h["sigma"].shape == (4, 6, 3)
    for name in ("T", "Tf") + (("sigma",) if cell.finite_sigma else ()):
        assert np.all(np.isfinite(h[name])), name
    twin = scheduled(cell, rows, n_cells)
    for rec in range(4):
        twin.solve(2)
        assert np.array_equal(h["T"][rec], twin.get_field("T")[:, sdof]), rec
        assert np.array_equal(h["Tf"][rec], twin.get_field("Tf")[:, sdof]), rec
        assert np.array_equal(h["sigma"][rec], twin.get_field("sigma")[:, probes], equal_nan=not cell.finite_sigma), rec
    same(state(ens), state(twin), "with / without a history")  # recording changes no state bit
    twin.close()
    ens.close()
    surface = [0, 2]  # the probes at the two ends
    for r in rows:
        ref = scheduled_oracle_run(cell, r, n_cells)
        for rec in range(4):
            s = 2 * rec + 1  # index of step 2 (rec + 1)
            e = relerr(h["T"][rec, r], ref["Ts"][s][sdof])
            print(f"[history {cell.id}] n_cells {n_cells} bar {r} record {rec}: T rel {e:.2e}")
            assert e <= 1e-10, (n_cells, r, rec, e)
            if cell.history_surface_sigma:
                mT, _ = cond_mask(ref["Ts"][s], ref["T_befores"][s])
                check_field(f"n_cells {n_cells} bar {r} record {rec} surface sigma", h["sigma"][rec, r][surface],
                            ref["sigmas"][s][probes][surface], mT[sdof][surface], 1, min_frac=1.0)


def history_and_a_failed_bar(cell):
    """Bar 1's T becomes NaN after step 4: its Newton loop runs to newton_max_it, the
    bar is restored and frozen at step 5 (the failure contract) and writes no record."""
    gpu()
    n_cells = 16
    rows = [0, 1, 2]
    hist = dict(nodes=[0, n_cells // 2, n_cells], every=2)
    good = scheduled(cell, rows, n_cells, history=hist)
    good.solve(N_STEPS)
    want, want_state = good.get_history(), state(good)
    good.close()
    ens = scheduled(cell, rows, n_cells, history=hist, error_on_nonconvergence=False)
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
    got = state(ens)
    for f in cell.state:
        assert np.array_equal(got[f][[0, 2]], want_state[f][[0, 2]], equal_nan=True), f
    ens.close()


def history_capacity(cell):
    gpu()
    from tvfem import NativeError
    from tvfem import _native as N
    ens = scheduled(cell, [0, 1, 2], 16, history=dict(nodes=[0, 16], every=2, max_records=2))
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


# ---- field shapes ----------------------------------------------------------------------------
def field_shapes(cell, n_cells):
    gpu()
    from tvfem import NativeError
    from tvfem import _native as N
    nT, nS = cell.n_T(n_cells), n_cells + 1
    other = {"cg": 2 * n_cells, "dg": n_cells + 1}[cell.fam]  # the other family's T dofs
    ens = ensemble(cell, [0, 1, 2], n_cells)
    assert ens.n_dofs_T == ens.n_dofs == nT and ens.n_dofs_sigma == nS
    for name in ("T", "T_prev", "Tf", "phi", "xi"):
        assert ens.get_field(name).shape == (3, nT), name
    assert ens.get_field("Tf_partial").shape == (3, 6 * nT)
    assert ens.get_field("sigma").shape == (3, nS)
    for name in ["s_tilde_partial", "sigma_tilde_partial"] + (PAPER_ONLY if cell.paper else []):
        assert ens.get_field(name).shape == (3, 6 * nS), name
    # the initial condition reaches every T dof, and set_field / get_field round-trip in the family's layout
    assert np.all(ens.get_field("T") == np.array([BARS[b][1] for b in (0, 1, 2)])[:, None])
    assert np.all(ens.get_field("Tf_partial") == np.array([BARS[b][1] for b in (0, 1, 2)])[:, None])
    for name, n in (("T", nT), ("Tf_partial", 6 * nT), ("sigma", nS), ("sigma_tilde_partial", 6 * nS)):
        v = np.arange(3 * n, dtype=float).reshape(3, n) + 0.25
        ens.set_field(name, v)
        assert np.array_equal(ens.get_field(name), v), name
    wrong = [("T", nT + 1), ("sigma", n_cells), ("Tf_partial", 6 * nT - 6)]
    if n_cells > 1:  # the other family's count (at one cell both families have two dofs)
        wrong += [("T", other), ("sigma", 2 * n_cells), ("Tf_partial", 6 * other)]
    for name, n in wrong:
        with pytest.raises(NativeError) as exc:
            ens.set_field(name, np.zeros((3, n)))
        assert exc.value.code == N.TV_ERR_ARG, (name, n)
    ens.close()
