"""ThermoViscoEnsemble (csrc/tv_ensemble.hip, csrc/tv_ensemble_dg.hip): what is specific to a
family or a model, as checks over a Cell of tests/ensemble_cases.py, which the test modules of
the six (family, model) cells call under their own test names.  A support module (pytest does
not collect it).  The contract of the shared step driver is tests/ensemble_contract.py.

Every cell against its CPU oracle bar by bar: the ten BARS over 6 steps, the six scheduled
SBARS over 8 (the oracle's ThermalParams set to the step's stage before each step), and 500
steps in one solve().  The exact cells' oracle is the unchanged oracle inside
tests/exact_relaxation.py.  Then the single-bar device path (ThermoViscoProblem, which has no
exact relaxation), the golden DG / CG fixture (10:1 jumps in h, where the '+' side of the
SIPG penalty matters), and what separates the models: the thermal problem does not see the
mode, only the stress sees the relaxation, and the two partial-stress fields exist on a paper
handle only.

Tolerances, min_frac and the Newton-count rule: the docstring of tests/ensemble_cases.py.
The 500-step case takes, per cell, the bars that can be compared there.  Reference: bars whose
every dof still moves more than 1e-6 K per step at the end (min_frac 0.9).  Paper: the bars
with T_0 <= 800 K, inside the Taylor limit, where the oracle stays finite (sigma at most 5.8e-2
CG, 3.3 DG, as measured).  Exact: all ten; several sit at ambient by then and their masked
fraction is 0, so no min_frac is passed and check_field's absolute bound carries them; in
addition the unmasked relative L2 error of sigma and of sigma_partial is <= 1e-6 per bar (in
exact mode the stress is an accumulated sum and an increment's rounding error is absolute and
tiny against it; measured sigma at most 0.211, bar 6).
"""
import json
import os

import numpy as np
import pytest

from ensemble_cases import (CELL, DT, HOT, N_STEPS, STRESS, THERMAL, ensemble, gpu, oracle_run, same, scheduled,
                            scheduled_oracle_run, src, state)
from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1d_dg_cg.npz")


# ---- 1. the oracle, six steps ----------------------------------------------------------------
def parity_with_oracle(cell, n_cells):
    gpu()
    n_steps = 6
    bars = list(range(10))
    refs = [oracle_run(cell, b, n_cells, n_steps, True) for b in bars]
    ens = ensemble(cell, bars, n_cells)
    assert (ens.model_mode, ens.relaxation) == ("paper" if cell.paper else "reference",
                                                "exact" if cell.model == "exact" else "taylor")
    strict = total = 0
    worst = 0.0
    for s in range(n_steps):
        ens.solve_timestep()
        T = ens.get_field("T")
        its = ens.newton_iterations
        for b in bars:
            e = relerr(T[b], refs[b]["Ts"][s])
            worst = max(worst, e)
            assert e <= 1e-10, (cell.id, n_cells, s, b, e)
            if cell.paper:  # T does not see the model: the counts are compared in the reference cells
                continue
            want, margin = refs[b]["hist"][s]
            total += 1
            if margin >= 1.0:
                strict += 1
                assert its[b] == want, (n_cells, s, b, int(its[b]), want, margin)
            else:
                assert abs(int(its[b]) - want) <= 1, (n_cells, s, b, int(its[b]), want, margin)
    print(f"[ensemble {cell.id}] n_cells {n_cells}: worst T rel {worst:.2e}; {strict}/{total} solves in the strict "
          f"Newton-count group; counts {sorted({h[0] for r in refs for h in r['hist']})}")
    assert strict >= 0.6 * total, (strict, total)
    assert not ens.failed_step.any()
    got = state(ens)
    ens.close()
    if cell.finite_sigma:  # reference mode: NaN wherever T has not moved, the equilibrium bar 4 above all
        assert np.all(np.isfinite(got["sigma"]))
    for b in bars:
        recs = cell.check_end(cell, f"n_cells {n_cells} bar {b}", got, b, n_cells, refs[b], cell.min_frac(b, n_cells))
        if b == 4 and cell.paper:
            assert all(r["frac"] == 0.0 for r in recs)


# ---- 2. the oracle, scheduled, eight steps ---------------------------------------------------
def schedule_parity_with_oracle(cell, n_cells):
    """The six SBARS as they are (the paper oracle stays finite on all of them over the 8
    steps, at most 1.1e75: asserted).  By the oracle's T every node of these bars is
    well-conditioned in step 8 except the core of bar 0 with DG at 16 cells (compared fraction
    0.71), so the cell's sched_min_frac applies to all six; in the DG reference cell T alone is
    compared."""
    gpu()
    rows = list(range(6))
    refs = [scheduled_oracle_run(cell, r, n_cells) for r in rows]
    ens = scheduled(cell, rows, n_cells)
    for s in range(N_STEPS):
        ens.solve_timestep()
        T = ens.get_field("T")
        for r in rows:
            e = relerr(T[r], refs[r]["Ts"][s])
            print(f"[schedule {cell.id}] n_cells {n_cells} step {s + 1} bar {r}: T rel {e:.2e}")
            assert e <= 1e-10, (cell.id, n_cells, s, r, e)
    assert not ens.failed_step.any()
    got = state(ens)
    ens.close()
    if cell.sched_min_frac is not None:
        for r in rows:
            cell.check_end(cell, f"scheduled n_cells {n_cells} bar {r}", got, r, n_cells, refs[r], cell.sched_min_frac)


# ---- 3. long horizon (module docstring) ------------------------------------------------------
LONG = {"cg-reference": dict(bars=[0, 9], frac=0.9),
        "dg-reference": dict(bars=[0, 5, 9], frac=0.9),
        "cg-paper": dict(bars=[0, 3, 4, 7, 8], frac=0.9, sigma_max=10.0),
        "dg-paper": dict(bars=[0, 3, 4, 7, 8], frac=0.6, sigma_max=10.0),
        "cg-exact": dict(bars=list(range(10)), frac=None, sigma_max=1.0, unmasked=1e-6),
        "dg-exact": dict(bars=list(range(10)), frac=None, sigma_max=1.0, unmasked=1e-6)}


def long_horizon(cell):
    """500 steps in one solve() against the oracle; solve(250) twice is the same bits."""
    gpu()
    n_cells, n_steps = 16, 500
    case = LONG[cell.id]
    bars = case["bars"]
    ens = ensemble(cell, bars, n_cells)
    ens.solve(n_steps)
    assert abs(ens.t - 50.0) < 1e-9
    assert not ens.failed_step.any()
    got = state(ens)
    total = ens.newton_total
    ens.close()
    if cell.finite_sigma:
        assert np.all(np.isfinite(got["sigma"]))
    for row, b in enumerate(bars):
        ref = oracle_run(cell, b, n_cells, n_steps)
        if cell.paper:
            assert ref["first_nonfinite"] is None
            assert np.abs(ref["end"]["sigma"]).max() <= case["sigma_max"]
        cell.check_end(cell, f"500 steps bar {b}", got, row, n_cells, ref, None if b == 4 else case["frac"])
        if "unmasked" in case:
            for name in ("sigma", "sigma_partial"):
                e = relerr(got[name][row], ref["end"][name])
                print(f"[ensemble {cell.id}] 500 steps bar {b}: unmasked {name} rel {e:.2e}")
                assert e <= case["unmasked"], (cell.id, b, name, e)
    two = ensemble(cell, bars, n_cells)
    two.solve(250)
    two.solve(250)
    same(state(two), got, "250 + 250")
    assert np.array_equal(two.newton_total, total)
    two.close()


# ---- 4. the single-bar device path -----------------------------------------------------------
def against_single_bar_path(cell):
    """The geometry.create_mesh graded bar, 20 steps: an ensemble over three parameter sets
    against three ThermoViscoProblem runs of the same config and model mode (Jacobi-PCG Newton,
    launch per operation).  Paper mode stays at main.py's T_0 = 800 K, inside the Taylor limit."""
    gpu()
    from geometry import graded_bar
    from tvfem import ThermoViscoEnsemble
    from tvfem.problem import ThermoViscoProblem
    T0s = [800.0, 873.0, 920.0] if cell.id == "dg-reference" else [O.MAIN_MODEL_PARAMS["T_0"]] * 3
    sets = list(zip([100.0, 280.1, 700.0], T0s))  # htc, T_0
    mesh = graded_bar()
    n_cells = mesh.n_cells[0]
    ens = ThermoViscoEnsemble(mesh, (0.0, 2.0), DT, cell.cfg,
                              dict(O.MAIN_MODEL_PARAMS, htc=np.array([s[0] for s in sets]),
                                   T_0=np.array([s[1] for s in sets])), **cell.ens_kw)
    ens.setup()
    assert ens.n_steps == 20 and ens.n_dofs_T == cell.n_T(n_cells)
    ens.solve(19)
    T_before = ens.get_field("T")
    ens.solve(1)
    got = state(ens)
    ens.close()
    for row, (htc, T0) in enumerate(sets):
        dev = ThermoViscoProblem(mesh, (0.0, 2.0), DT, cell.cfg, dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=T0),
                                 verbose=False, write_output=False, **(dict(model_mode="paper") if cell.paper else {}))
        dev.setup()
        dev.solve(19)
        Tb = np.array(dev.functions_current["T"].x.array)
        dev.solve(1)
        Td = np.array(dev.functions_current["T"].x.array)
        e = relerr(got["T"][row], Td)
        print(f"[ensemble {cell.id}] single-bar path htc {htc}: T rel {e:.2e}")
        assert e <= 1e-10, (htc, e)
        assert relerr(T_before[row], Tb) <= 1e-10
        _, mS = cond_mask(Td, Tb, src_map=src(cell.fam, n_cells))
        want = {"sigma": np.array(dev.functions_next["sigma"].x.array)}
        if not cell.paper:
            check_field(f"htc {htc} sigma", got["sigma"][row], want["sigma"], mS, 1)
        else:
            for k in STRESS[1:]:
                want[k] = np.array(dev.functions_current[k].x.array)
            vol = float(np.linalg.norm(want["sigma_partial"]))
            for k in STRESS:
                assert np.all(np.isfinite(want[k])), k
                check_field(f"htc {htc} {k}", got[k][row], want[k], mS, 1 if k == "sigma" else 6,
                            scale=vol if k.startswith("s_") else None)
        dev.close()


# ---- 5. the golden fixture -------------------------------------------------------------------
def golden_fixture(copies):
    gpu()
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    assert meta["config"] == CELL["dg-reference"].cfg
    ens = ThermoViscoEnsemble(RectilinearMesh([z["axis0"]]), (0.0, meta["steps"] * meta["dt"]), meta["dt"],
                              meta["config"], meta["model_parameters"], n_bars=copies)
    ens.setup()
    assert meta["steps"] == len(z["newton_its"])
    for s in range(meta["steps"]):
        ens.solve_timestep()
        its = ens.newton_iterations
        assert np.all(np.abs(its - int(z["newton_its"][s])) <= 1), (s, its, z["newton_its"][s])
    for row in range(copies):
        e = relerr(ens.get_field("T")[row], z["T"])
        print(f"[ensemble dg] golden row {row}: T rel {e:.2e}")
        assert e <= 1e-10, (row, e)
        for name, bs in (("Tf", 1), ("Tf_partial", 6), ("phi", 1), ("xi", 1)):
            check_field(f"golden row {row} {name}", ens.get_field(name)[row], z[name], z["mask_T"], bs)
        check_field(f"golden row {row} sigma", ens.get_field("sigma")[row], z["sigma"], z["mask_S"], 1)
    ens.close()


# ---- 6. what separates the models ------------------------------------------------------------
def thermal_problem_does_not_see_the_mode(cell):
    gpu()
    n_cells = 16
    pap = ensemble(cell, list(range(10)), n_cells)
    ref = ensemble(CELL[cell.fam + "-reference"], list(range(10)), n_cells)
    for s in range(6):
        pap.solve_timestep()
        ref.solve_timestep()
        for f in THERMAL:
            assert np.array_equal(pap.get_field(f), ref.get_field(f)), (cell.id, s, f)
        assert np.array_equal(pap.newton_iterations, ref.newton_iterations), (cell.id, s)
        assert np.array_equal(pap.newton_total, ref.newton_total), (cell.id, s)
    # and the stress is where they differ: NaN on the equilibrium bar in reference mode only
    assert np.isnan(ref.get_field("sigma")[4]).all() and np.isfinite(pap.get_field("sigma")).all()
    pap.close()
    ref.close()


def only_the_stress_sees_the_relaxation(fam):
    """Exact against Taylor: the T family and the statistics are the same bits."""
    gpu()
    n_cells = 16
    ex = ensemble(CELL[fam + "-exact"], list(range(10)), n_cells)
    ta = ensemble(CELL[fam + "-paper"], list(range(10)), n_cells, relaxation="taylor")
    assert ta.relaxation == "taylor"
    for s in range(6):
        ex.solve_timestep()
        ta.solve_timestep()
        for f in ("T", "T_prev", "Tf", "Tf_partial", "phi", "xi"):
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


def partial_stress_fields_exist_only_on_a_paper_handle(cell):
    gpu()
    from tvfem import NativeError
    from tvfem import _native as N
    n_cells = 5
    ref = ensemble(CELL[cell.fam + "-reference"], [0, 1, 2], n_cells)
    for name in ("s_partial", "sigma_partial"):
        with pytest.raises(NativeError) as exc:
            ref.get_field(name)
        assert exc.value.code == N.TV_ERR_STATE, name
        with pytest.raises(NativeError) as exc:
            ref.set_field(name, np.zeros((3, 6 * (n_cells + 1))))
        assert exc.value.code == N.TV_ERR_STATE, name
    ref.close()
    pap = ensemble(cell, [0, 1, 2], n_cells)
    for name in ("s_partial", "sigma_partial"):
        assert pap.get_field(name).shape == (3, 6 * (n_cells + 1)), name
        assert np.all(pap.get_field(name) == 0.0), name
        v = np.arange(3 * 6 * (n_cells + 1), dtype=float).reshape(3, -1) + 0.25
        pap.set_field(name, v)
        assert np.array_equal(pap.get_field(name), v), name
        with pytest.raises(NativeError) as exc:
            pap.set_field(name, np.zeros((3, 6 * n_cells)))
        assert exc.value.code == N.TV_ERR_ARG, name
    pap.setup()  # the initial condition takes the stress memory back to zero
    for name in ("s_partial", "sigma_partial"):
        assert np.all(pap.get_field(name) == 0.0), name
    pap.close()
