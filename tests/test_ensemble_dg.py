"""ThermoViscoEnsemble with DG1 temperature and CG1 stress (csrc/tv_ensemble_dg.hip,
main.py's own fe_config): against the CPU oracle bar by bar, against the golden
DG / CG fixture (10:1 jumps in h, where the '+' side of the SIPG penalty
matters), against itself (independence of the bars, padding lanes, splits),
against the single-bar device path, the failure contract, schedules and
histories, and the shapes of the two field families.

Tolerances: T rel. L2 <= 1e-10 per bar at every compared step (the project's
ensemble tolerance); phi / Tf / xi on T dofs and sigma on mesh nodes through
parity_util.check_field with its tolerances, the well-conditioned nodes being
those whose source dof (the oracle's sigma <- T map) moved; Newton counts equal
wherever the oracle's own decision was at least a decade from flipping, within
one elsewhere.  min_frac is 0.9 in general, None for the equilibrium bar 4, and
0.5 for bars 0 and 3 at 16 cells: their cores have not moved 1e-6 K after six
steps (the oracle's own well-conditioned share there is 0.62-0.71 on T dofs and
0.65-0.71 on nodes, 1.0 everywhere else).  Everything else is bitwise.
"""
import functools
import json
import os

import numpy as np
import pytest

from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr
from test_ensemble import BARS, _coords, _newton_margin, _params
from test_ensemble_schedule import N_STEPS, SBARS, _graded, _stage_of

pytestmark = pytest.mark.gpu

CFG = {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
DT = 0.1
STATE = ["T", "T_prev", "Tf", "Tf_partial", "phi", "xi", "sigma", "s_tilde_partial", "sigma_tilde_partial"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1d_dg_cg.npz")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _src(n_cells):
    """sigma node -> T dof: 2 i, and 2 n_cells - 1 for the last node (the last cell in cell order wins)."""
    return np.append(2 * np.arange(n_cells), 2 * n_cells - 1)


def _ensemble(bars, n_cells, **kw):
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    mp = dict(O.MAIN_MODEL_PARAMS)
    for k, col in (("htc", 0), ("T_0", 1), ("T_ambient", 2), ("epsilon", 3)):
        mp[k] = np.array([BARS[b][col] for b in bars])
    meshes = [RectilinearMesh([_coords(b, n_cells)]) for b in bars]
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFG, mp, **kw)
    ens.setup()
    return ens


def _oracle(bar, n_cells):
    ref = O.OracleProblem(O.rectilinear_mesh([_coords(bar, n_cells)]), (0.0, 50.0), DT, CFG, _params(bar),
                          linear="direct")
    ref.setup()
    assert np.array_equal(ref._maps[("S", "T")], _src(n_cells))
    return ref


@functools.lru_cache(maxsize=None)
def _oracle_run(bar, n_cells, n_steps, keep_every_step):
    """One bar through the oracle, once per session: T after every step (or only
    the last), the end state, T before the last step, per step (Newton count, margin)."""
    ref = _oracle(bar, n_cells)
    Ts, hist = [], []
    T_before = None
    for s in range(n_steps):
        if keep_every_step:
            it, margin = _newton_margin(ref.form, ref.functions_current["T"], ref.functions_previous["T"])
        T_before = ref.functions_current["T"].copy()
        ref.solve_timestep()
        if keep_every_step:
            assert ref.newton_history[-1][0] == it  # the helper restates the oracle's loop
            hist.append((it, margin))
            Ts.append(ref.functions_current["T"].copy())
    end = {"T": ref.functions_current["T"].copy(), "phi": ref.functions["phi"].copy(),
           "Tf": ref.functions_current["Tf"].copy(), "xi": ref.functions["xi"].copy(),
           "sigma": ref.functions_next["sigma"].copy()}
    return {"Ts": Ts, "hist": hist, "T_before": T_before, "end": end}


def _min_frac(bar, n_cells):
    """After six steps (module docstring)."""
    if bar == 4:
        return None
    return 0.5 if (n_cells == 16 and bar in (0, 3)) else 0.9


def _check_end(tag, ens, row, bar, n_cells, ref, min_frac):
    e = relerr(ens.get_field("T")[row], ref["end"]["T"])
    print(f"[ensemble dg] {tag} bar {bar}: T rel {e:.2e}")
    assert e <= 1e-10, (tag, bar, e)
    mT, mS = cond_mask(ref["end"]["T"], ref["T_before"], src_map=_src(n_cells))
    for name in ("phi", "Tf", "xi", "sigma"):
        check_field(f"{tag} bar {bar} {name}", ens.get_field(name)[row], ref["end"][name],
                    mS if name == "sigma" else mT, 1, min_frac=min_frac)


# ---- 1. the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
def test_parity_with_oracle(n_cells):
    _torch()
    n_steps = 6
    bars = list(range(10))
    refs = [_oracle_run(b, n_cells, n_steps, True) for b in bars]
    ens = _ensemble(bars, n_cells)
    strict = total = 0
    worst = 0.0
    for s in range(n_steps):
        ens.solve_timestep()
        T = ens.get_field("T")
        its = ens.newton_iterations
        for b in bars:
            e = relerr(T[b], refs[b]["Ts"][s])
            worst = max(worst, e)
            assert e <= 1e-10, (n_cells, s, b, e)
            want, margin = refs[b]["hist"][s]
            total += 1
            if margin >= 1.0:
                strict += 1
                assert its[b] == want, (n_cells, s, b, int(its[b]), want, margin)
            else:
                assert abs(int(its[b]) - want) <= 1, (n_cells, s, b, int(its[b]), want, margin)
    print(f"[ensemble dg] n_cells {n_cells}: worst T rel {worst:.2e}; {strict}/{total} solves in the strict "
          f"Newton-count group; counts {sorted({h[0] for r in refs for h in r['hist']})}")
    assert strict >= 0.6 * total, (strict, total)
    assert not ens.failed_step.any()
    for b in bars:
        _check_end(f"n_cells {n_cells}", ens, b, b, n_cells, refs[b], _min_frac(b, n_cells))
    ens.close()


# ---- 2. the golden fixture -------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, 3])
def test_golden_fixture(copies):
    _torch()
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    assert meta["config"] == CFG
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


# ---- 3. independence and padding -------------------------------------------------------------
def test_independence_and_padding():
    """A bar computes the same bits alone, in the ten-bar ensemble, and repeated
    into tail lanes (65 bars), a second wave and a second workgroup (130)."""
    _torch()
    n_cells, n_steps = 16, 6
    ten = _ensemble(list(range(10)), n_cells)
    ten.solve(n_steps)
    want = {f: ten.get_field(f) for f in STATE}
    its, total = ten.newton_iterations, ten.newton_total
    assert not ten.failed_step.any()
    ten.close()
    for b in range(10):
        one = _ensemble([b], n_cells)
        one.solve(n_steps)
        for f in STATE:
            assert np.array_equal(one.get_field(f)[0], want[f][b], equal_nan=True), (b, f)
        assert one.newton_iterations[0] == its[b] and one.newton_total[0] == total[b]
        one.close()
    for n_bars in (65, 130):
        idx = [i % 10 for i in range(n_bars)]
        rep = _ensemble(idx, n_cells)
        rep.solve(n_steps)
        for f in STATE:
            assert np.array_equal(rep.get_field(f), want[f][idx], equal_nan=True), (n_bars, f)
        assert np.array_equal(rep.newton_iterations, its[idx])
        assert np.array_equal(rep.newton_total, total[idx])
        assert not rep.failed_step.any()
        rep.close()


# ---- 4. long horizon -------------------------------------------------------------------------
def test_long_horizon():
    """500 steps in one solve() against the oracle; solve(250) twice is the same bits."""
    _torch()
    n_cells, n_steps = 16, 500
    bars = [0, 5, 9]  # every dof of these still moves more than 1e-6 K per step at the end
    ens = _ensemble(bars, n_cells)
    ens.solve(n_steps)
    assert abs(ens.t - 50.0) < 1e-9
    for row, b in enumerate(bars):
        _check_end("500 steps", ens, row, b, n_cells, _oracle_run(b, n_cells, n_steps, False), 0.9)
    two = _ensemble(bars, n_cells)
    two.solve(250)
    two.solve(250)
    for f in STATE:
        assert np.array_equal(two.get_field(f), ens.get_field(f), equal_nan=True), f
    assert np.array_equal(two.newton_total, ens.newton_total)
    ens.close()
    two.close()


# ---- 5. the single-bar device path -----------------------------------------------------------
def test_against_single_bar_path():
    """The geometry.create_mesh graded bar, 20 steps: an ensemble over three parameter
    sets against three ThermoViscoProblem runs with the same DG / CG config."""
    _torch()
    from geometry import graded_bar
    from tvfem import ThermoViscoEnsemble
    from tvfem.problem import ThermoViscoProblem
    sets = [(100.0, 800.0), (280.1, 873.0), (700.0, 920.0)]  # htc, T_0
    mesh = graded_bar()
    n_cells = mesh.n_cells[0]
    ens = ThermoViscoEnsemble(mesh, (0.0, 2.0), DT, CFG,
                              dict(O.MAIN_MODEL_PARAMS, htc=np.array([s[0] for s in sets]),
                                   T_0=np.array([s[1] for s in sets])))
    ens.setup()
    assert ens.n_steps == 20 and ens.n_dofs_T == 2 * n_cells
    ens.solve(19)
    T_before = ens.get_field("T")
    ens.solve(1)
    T, sigma = ens.get_field("T"), ens.get_field("sigma")
    ens.close()
    for row, (htc, T0) in enumerate(sets):
        dev = ThermoViscoProblem(mesh, (0.0, 2.0), DT, CFG, dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=T0),
                                 verbose=False, write_output=False)
        dev.setup()
        dev.solve(19)
        Tb = np.array(dev.functions_current["T"].x.array)
        dev.solve(1)
        Td = np.array(dev.functions_current["T"].x.array)
        e = relerr(T[row], Td)
        print(f"[ensemble dg] single-bar path htc {htc}: T rel {e:.2e}")
        assert e <= 1e-10, (htc, e)
        assert relerr(T_before[row], Tb) <= 1e-10
        _, mS = cond_mask(Td, Tb, src_map=_src(n_cells))
        check_field(f"htc {htc} sigma", sigma[row], np.array(dev.functions_next["sigma"].x.array), mS, 1)
        dev.close()


# ---- 6. the failure contract -----------------------------------------------------------------
@pytest.mark.parametrize("error_on_nonconvergence", [True, False])
def test_failure_semantics(error_on_nonconvergence):
    """newton_max_it = 1: the incremental criterion cannot converge at iteration 1,
    so every bar fails its first step, is restored and frozen.  A second ensemble
    in which only some bars fail (NaN temperatures) shows the others advancing."""
    _torch()
    from tvfem import NativeError
    from tvfem import _native as N
    n_cells = 16
    ens = _ensemble(list(range(10)), n_cells, newton_max_it=1, error_on_nonconvergence=error_on_nonconvergence)
    init = {f: ens.get_field(f) for f in STATE}
    if error_on_nonconvergence:
        with pytest.raises(NativeError) as exc:
            ens.solve(3)
        assert exc.value.code == N.TV_ERR_NOT_CONVERGED
        assert "bar 0" in str(exc.value) and "step 1" in str(exc.value)
    else:
        ens.solve(3)
    assert np.array_equal(ens.failed_step, np.ones(10, dtype=int))
    assert np.array_equal(ens.newton_iterations, np.ones(10, dtype=int))
    got = {f: ens.get_field(f) for f in STATE}
    assert np.array_equal(got["T"], got["T_prev"])  # T <- T_prev
    for f in STATE:
        if f != "T":  # the visco state and T_prev are untouched, bit for bit
            assert np.array_equal(got[f], init[f], equal_nan=True), f
    # bar 4: zero residual, zero increment -- T too is still the initial condition
    assert np.array_equal(got["T"][4], init["T"][4]) and np.all(init["T"][4] == BARS[4][1])
    ens.close()
    # bars 2 and 7 fail at step 1 (NaN never converges), the others advance as if alone with them
    good = _ensemble(list(range(10)), n_cells)
    good.solve(3)
    want = {f: good.get_field(f) for f in STATE}
    good.close()
    ens = _ensemble(list(range(10)), n_cells, error_on_nonconvergence=error_on_nonconvergence)
    T = ens.get_field("T")
    T[[2, 7]] = np.nan
    ens.set_field("T", T)
    before = {f: ens.get_field(f) for f in STATE}
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
    for f in STATE:
        g = ens.get_field(f)
        assert np.array_equal(g[ok], want[f][ok], equal_nan=True), f
        if f != "T":
            assert np.array_equal(g[~ok], before[f][~ok], equal_nan=True), f
    assert np.array_equal(ens.get_field("T")[~ok], before["T_prev"][~ok])
    ens.close()


# ---- 7. thermal-only steps -------------------------------------------------------------------
def test_thermal_only():
    _torch()
    n_cells = 16
    ens = _ensemble(list(range(10)), n_cells)
    ens.solve(3, thermal_only=True)
    T, sigma = ens.get_field("T"), ens.get_field("sigma")
    assert not ens.failed_step.any()
    assert np.array_equal(ens.get_field("T_prev"), T)
    ens.close()
    assert np.all(sigma == 0.0)
    for b in range(10):
        ref = _oracle(b, n_cells)
        ref.solve(3, thermal_only=True)
        e = relerr(T[b], ref.functions_current["T"])
        assert e <= 1e-10, (b, e)


# ---- 8. schedules and histories --------------------------------------------------------------
def _scheduled(rows, n_cells, schedule=True, **kw):
    """test_ensemble_schedule._scheduled with the DG / CG config."""
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
def _scheduled_oracle(row, n_cells):
    """T of bar `row` of SBARS after every step, the oracle's ThermalParams set to the step's stage."""
    T0, eps, L, graded, stages = SBARS[row]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=T0, epsilon=eps, htc=stages[0][1], T_ambient=stages[0][2])
    ref = O.OracleProblem(O.rectilinear_mesh([_graded(L, graded, n_cells)]), (0.0, 50.0), DT, CFG, mp,
                          linear="direct")
    ref.setup()
    out = []
    for step in range(1, N_STEPS + 1):
        _, htc, Ta = stages[_stage_of(stages, step)]
        ref.tp.htc, ref.tp.T_ambient, ref.tp.epsilon = htc, Ta, eps
        ref.solve_timestep()
        out.append(ref.functions_current["T"].copy())
    return out


@pytest.mark.parametrize("n_cells", [1, 3, 16])
def test_schedule_parity_with_oracle(n_cells):
    _torch()
    rows = list(range(6))
    refs = [_scheduled_oracle(r, n_cells) for r in rows]
    ens = _scheduled(rows, n_cells)
    for s in range(N_STEPS):
        ens.solve_timestep()
        T = ens.get_field("T")
        for r in rows:
            e = relerr(T[r], refs[r][s])
            print(f"[schedule dg] n_cells {n_cells} step {s + 1} bar {r}: T rel {e:.2e}")
            assert e <= 1e-10, (n_cells, s, r, e)
    assert not ens.failed_step.any()
    ens.close()


def _ten(n_cells, **kw):
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    mp = dict(O.MAIN_MODEL_PARAMS, htc=np.array([b[0] for b in BARS]), T_0=np.array([b[1] for b in BARS]),
              T_ambient=np.array([b[2] for b in BARS]), epsilon=np.array([b[3] for b in BARS]))
    meshes = [RectilinearMesh([_coords(i, n_cells)]) for i in range(10)]
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFG, mp, **kw)
    ens.setup()
    return ens


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
    htc, Ta, eps = (np.array([b[c] for b in BARS]) for c in (0, 2, 3))
    one = [dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    three = [dict(until_step=np.arange(10) % 4, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(until_step=np.arange(10) % 4 + np.arange(10) % 3 * 2, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    for tag, sched in (("one stage", one), ("three equal stages", three)):
        ens = _ten(n_cells, schedule=sched)
        ens.solve(N_STEPS)
        _same(_state(ens), want, tag)
        ens.close()


def test_scheduled_split():
    """Stage ends that differ from lane to lane: solve(8) = solve(3) + solve(5)."""
    _torch()
    rows = list(range(6))
    whole = _scheduled(rows, 16)
    whole.solve(N_STEPS)
    split = _scheduled(rows, 16)
    split.solve(3)
    split.solve(5)
    _same(_state(split), _state(whole), "split")
    assert np.array_equal(split.newton_total, whole.newton_total)
    whole.close()
    split.close()


@pytest.mark.parametrize("n_cells", [1, 16])
def test_history(n_cells):
    """Records bitwise equal to get_field of a twin stepped `every` steps at a time:
    T and Tf at the probe node's source dof, sigma at the node."""
    _torch()
    rows = list(range(6))
    probes = [0, n_cells // 2, n_cells]
    src = _src(n_cells)[probes]
    ens = _scheduled(rows, n_cells, history=dict(nodes=probes, every=2))
    ens.solve(N_STEPS)
    h = ens.get_history()
    assert np.array_equal(h["step"], [2, 4, 6, 8]) and np.allclose(h["t"], [0.2, 0.4, 0.6, 0.8])
    assert h["T"].shape == h["Tf"].shape == h["sigma"].shape == (4, 6, 3)
    assert np.all(np.isfinite(h["T"])) and np.all(np.isfinite(h["Tf"]))
    twin = _scheduled(rows, n_cells)
    for rec in range(4):
        twin.solve(2)
        assert np.array_equal(h["T"][rec], twin.get_field("T")[:, src]), rec
        assert np.array_equal(h["Tf"][rec], twin.get_field("Tf")[:, src]), rec
        assert np.array_equal(h["sigma"][rec], twin.get_field("sigma")[:, probes], equal_nan=True), rec
    _same(_state(ens), _state(twin), "with / without a history")  # recording changes no state bit
    twin.close()
    ens.close()
    for r in rows:  # and the recorded T is the oracle's
        ref = _scheduled_oracle(r, n_cells)
        for rec in range(4):
            assert relerr(h["T"][rec, r], ref[2 * rec + 1][src]) <= 1e-10, (n_cells, r, rec)


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


# ---- 9. field shapes -------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 5])
def test_field_shapes(n_cells):
    _torch()
    from tvfem import NativeError
    from tvfem import _native as N
    ens = _ensemble([0, 1, 2], n_cells)
    assert ens.n_dofs_T == ens.n_dofs == 2 * n_cells and ens.n_dofs_sigma == n_cells + 1
    for name in ("T", "T_prev", "Tf", "phi", "xi"):
        assert ens.get_field(name).shape == (3, 2 * n_cells), name
    assert ens.get_field("Tf_partial").shape == (3, 12 * n_cells)
    assert ens.get_field("sigma").shape == (3, n_cells + 1)
    for name in ("s_tilde_partial", "sigma_tilde_partial"):
        assert ens.get_field(name).shape == (3, 6 * (n_cells + 1)), name
    # the initial condition reaches every T dof, and set_field / get_field round-trip in the family's layout
    assert np.all(ens.get_field("T") == np.array([BARS[b][1] for b in (0, 1, 2)])[:, None])
    assert np.all(ens.get_field("Tf_partial") == np.array([BARS[b][1] for b in (0, 1, 2)])[:, None])
    for name, n in (("T", 2 * n_cells), ("Tf_partial", 12 * n_cells), ("sigma", n_cells + 1),
                    ("sigma_tilde_partial", 6 * (n_cells + 1))):
        v = np.arange(3 * n, dtype=float).reshape(3, n) + 0.25
        ens.set_field(name, v)
        assert np.array_equal(ens.get_field(name), v), name
    wrong = [("T", 2 * n_cells + 1), ("sigma", n_cells), ("Tf_partial", 12 * n_cells - 6)]
    if n_cells > 1:  # the other family's count (at one cell both families have two dofs)
        wrong += [("T", n_cells + 1), ("sigma", 2 * n_cells), ("Tf_partial", 6 * (n_cells + 1))]
    for name, n in wrong:
        with pytest.raises(NativeError) as exc:
            ens.set_field(name, np.zeros((3, n)))
        assert exc.value.code == N.TV_ERR_ARG, (name, n)
    ens.close()
