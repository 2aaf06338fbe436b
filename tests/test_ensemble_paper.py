"""ThermoViscoEnsemble(model_mode="paper"): the paper-correct viscoelastic model in
both bar kernels (csrc/tv_ensemble.hip, csrc/tv_ensemble_dg.hip, the kPaper
instantiations of csrc/tv_ensemble_step.h), CG1 / CG1 and DG1 / CG1: against the
CPU oracle's paper mode bar by bar, against the reference-mode ensemble (the
thermal problem does not see the mode), against itself (independence of the
bars, padding lanes, splits), against the single-bar device path, the failure
contract, thermal-only steps, schedules and histories.

Tolerances are those of tests/test_paper_mode.py: T rel. L2 <= 1e-10 after
every step; Tf and Tf_partial <= 1e-10; phi and xi <= 1e-9 (the trapezoidal xi
is a sum: no cancellation); sigma, s_partial, sigma_partial, s_tilde_partial and
sigma_tilde_partial through parity_util.check_field (1e-6 on the nodes whose
source dof moved more than 1e-6 K in the oracle's last step, an absolute bound
on the rest), the deviatoric partials measured against the volumetric scale.
Every compared oracle array is asserted finite, so NaN == NaN hides nothing, and
the compared fraction, which the oracle's T alone decides, is at least 0.9 for
CG and 0.6 for DG on every bar but the equilibrium bar 4, whose T never moves
(fraction 0: it goes wholly to the absolute bound).  After six steps at 16
cells the oracle's own fractions are 1.00 for DG except bars 0 (0.71) and 3
(0.65), and >= 0.94 for CG.  Everything else is bitwise.

The hot bars (T_0 >= 850 K) lie outside the Taylor limit xi <= 2 lambda of the
degree-2 exponential: their stress grows to 5e60 within six steps, in the
oracle and here alike, and overflows later; they are compared over 6 and 8
steps and left out of the 500-step case.
"""
import functools

import numpy as np
import pytest

from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr
from test_ensemble import BARS, _coords, _params
from test_ensemble_schedule import N_STEPS, SBARS, _graded, _stage_of

pytestmark = pytest.mark.gpu

CFGS = {"cg": {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}},
        "dg": {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}}
FAMS = ["cg", "dg"]
DT = 0.1
THERMAL = ["T", "T_prev"]
VISCO = ["Tf", "Tf_partial", "phi", "xi", "sigma", "s_tilde_partial", "sigma_tilde_partial", "s_partial",
         "sigma_partial"]
STATE = THERMAL + VISCO  # the eleven state fields of a paper ensemble
STRESS = ["sigma", "s_partial", "sigma_partial", "s_tilde_partial", "sigma_tilde_partial"]
MIN_FRAC = {"cg": 0.9, "dg": 0.6}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _src(fam, n_cells):
    """sigma node -> T dof.  CG: the node itself; DG: 2 i, and 2 n_cells - 1 for the last node."""
    if fam == "cg":
        return np.arange(n_cells + 1)
    return np.append(2 * np.arange(n_cells), 2 * n_cells - 1)


def _ensemble(fam, bars, n_cells, model_mode="paper", **kw):
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    mp = dict(O.MAIN_MODEL_PARAMS)
    for k, col in (("htc", 0), ("T_0", 1), ("T_ambient", 2), ("epsilon", 3)):
        mp[k] = np.array([BARS[b][col] for b in bars])
    meshes = [RectilinearMesh([_coords(b, n_cells)]) for b in bars]
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFGS[fam], mp, model_mode=model_mode, **kw)
    ens.setup()
    return ens


def _state(ens, names=STATE):
    return {f: ens.get_field(f) for f in names}


def _same(got, want, tag, names=STATE):
    for f in names:
        assert np.array_equal(got[f], want[f], equal_nan=True), (tag, f)


def _oracle_end(ref):
    """The compared state of a paper oracle, every array finite."""
    fc, fn, f = ref.functions_current, ref.functions_next, ref.functions
    end = {"T": fc["T"], "Tf": fc["Tf"], "Tf_partial": fc["Tf_partial"], "phi": f["phi"], "xi": f["xi"],
           "sigma": fn["sigma"], "s_partial": fc["s_partial"], "sigma_partial": fc["sigma_partial"],
           "s_tilde_partial": fc["s_tilde_partial"], "sigma_tilde_partial": fc["sigma_tilde_partial"]}
    end = {k: np.array(v, dtype=np.float64) for k, v in end.items()}
    for k, v in end.items():
        assert np.all(np.isfinite(v)), f"the oracle's {k} is not finite"
    return end


@functools.lru_cache(maxsize=None)
def _oracle_run(fam, bar, n_cells, n_steps, keep_every_step):
    """One of the ten BARS through the paper oracle, once per session."""
    ref = O.OracleProblem(O.rectilinear_mesh([_coords(bar, n_cells)]), (0.0, 50.0), DT, CFGS[fam], _params(bar),
                          linear="direct", model_mode="paper")
    ref.setup()
    assert np.array_equal(ref._maps[("S", "T")], _src(fam, n_cells))
    Ts, T_before = [], None
    with np.errstate(all="ignore"):
        for _ in range(n_steps):
            T_before = ref.functions_current["T"].copy()
            ref.solve_timestep()
            if keep_every_step:
                Ts.append(ref.functions_current["T"].copy())
    return {"Ts": Ts, "T_before": T_before, "end": _oracle_end(ref)}


def _check_state(tag, fam, n_cells, got, row, ref, min_frac):
    """Row `row` of the ensemble state `got` against the oracle record `ref` (module docstring)."""
    end = ref["end"]
    e = relerr(got["T"][row], end["T"])
    print(f"[ensemble paper] {tag}: T rel {e:.2e}")
    assert e <= 1e-10, (tag, e)
    for name, tol in (("Tf", 1e-10), ("Tf_partial", 1e-10), ("phi", 1e-9), ("xi", 1e-9)):
        assert np.all(np.isfinite(got[name][row])), (tag, name)
        e = relerr(got[name][row], end[name])
        print(f"[ensemble paper] {tag}: {name} rel {e:.2e}")
        assert e <= tol, (tag, name, e)
    _, mS = cond_mask(end["T"], ref["T_before"], src_map=_src(fam, n_cells))
    vol = float(np.linalg.norm(end["sigma_partial"]))
    recs = []
    for name in STRESS:
        # the deviatoric partial stresses are rounding noise (isotropic strain): measured against the
        # volumetric scale, as tests/test_paper_mode.py does
        scale = vol if name.startswith("s_") else None
        recs.append(check_field(f"{tag} {name}", got[name][row], end[name], mS, 1 if name == "sigma" else 6,
                                min_frac=min_frac, scale=scale))
    return recs


# ---- 1. the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_parity_with_oracle(fam, n_cells):
    _torch()
    n_steps = 6
    bars = list(range(10))
    refs = [_oracle_run(fam, b, n_cells, n_steps, True) for b in bars]
    ens = _ensemble(fam, bars, n_cells)
    for s in range(n_steps):
        ens.solve_timestep()
        T = ens.get_field("T")
        for b in bars:
            e = relerr(T[b], refs[b]["Ts"][s])
            assert e <= 1e-10, (fam, n_cells, s, b, e)
    assert not ens.failed_step.any()
    got = _state(ens)
    ens.close()
    assert not np.isnan(got["sigma"]).any()  # reference mode: NaN wherever T has not moved
    assert np.all(np.isfinite(got["sigma"][4]))  # the equilibrium bar
    for b in bars:
        recs = _check_state(f"{fam} n_cells {n_cells} bar {b}", fam, n_cells, got, b, refs[b],
                            None if b == 4 else MIN_FRAC[fam])
        if b == 4:
            assert all(r["frac"] == 0.0 for r in recs)


# ---- 2. the thermal problem does not see the mode --------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_thermal_problem_does_not_see_the_mode(fam):
    _torch()
    n_cells = 16
    pap = _ensemble(fam, list(range(10)), n_cells)
    ref = _ensemble(fam, list(range(10)), n_cells, model_mode="reference")
    for s in range(6):
        pap.solve_timestep()
        ref.solve_timestep()
        for f in THERMAL:
            assert np.array_equal(pap.get_field(f), ref.get_field(f)), (fam, s, f)
        assert np.array_equal(pap.newton_iterations, ref.newton_iterations), (fam, s)
        assert np.array_equal(pap.newton_total, ref.newton_total), (fam, s)
    # and the stress is where they differ: NaN on the equilibrium bar in reference mode only
    assert np.isnan(ref.get_field("sigma")[4]).all() and np.isfinite(pap.get_field("sigma")).all()
    pap.close()
    ref.close()


# ---- 3. bitwise self-consistency -------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_independence_padding_and_split(fam):
    """A bar computes the same bits alone, among ten, and repeated into tail lanes (65
    bars), a second wave and a second workgroup (130); solve(3) + solve(5) = solve(8)."""
    _torch()
    n_cells, n_steps = 16, 8
    ten = _ensemble(fam, list(range(10)), n_cells)
    ten.solve(n_steps)
    want = _state(ten)
    its, total = ten.newton_iterations, ten.newton_total
    assert not ten.failed_step.any()
    ten.close()
    # the stress has a memory (in 1D the deviatoric strain, and with it s_partial, is exactly zero)
    assert np.abs(want["sigma_partial"]).max() > 0.0 and np.abs(want["sigma_tilde_partial"]).max() > 0.0
    split = _ensemble(fam, list(range(10)), n_cells)
    split.solve(3)
    split.solve(5)
    _same(_state(split), want, "split")
    assert np.array_equal(split.newton_total, total)
    split.close()
    for b in range(10):
        one = _ensemble(fam, [b], n_cells)
        one.solve(n_steps)
        got = _state(one)
        for f in STATE:
            assert np.array_equal(got[f][0], want[f][b], equal_nan=True), (b, f)
        assert one.newton_iterations[0] == its[b] and one.newton_total[0] == total[b]
        one.close()
    for n_bars in (65, 130):
        idx = [i % 10 for i in range(n_bars)]
        rep = _ensemble(fam, idx, n_cells)
        rep.solve(n_steps)
        got = _state(rep)
        for f in STATE:
            assert np.array_equal(got[f], want[f][idx], equal_nan=True), (n_bars, f)
        assert np.array_equal(rep.newton_iterations, its[idx])
        assert np.array_equal(rep.newton_total, total[idx])
        rep.close()


# ---- 4. long horizon -------------------------------------------------------------------------
LONG_BARS = [0, 3, 4, 7, 8]  # T_0 <= 800 K: inside the Taylor limit, the oracle stays finite


@pytest.mark.parametrize("fam", FAMS)
def test_long_horizon(fam):
    """500 steps in one solve() against the oracle; solve(250) twice is the same bits."""
    _torch()
    n_cells, n_steps = 16, 500
    ens = _ensemble(fam, LONG_BARS, n_cells)
    ens.solve(n_steps)
    assert abs(ens.t - 50.0) < 1e-9
    assert not ens.failed_step.any()
    got = _state(ens)
    total = ens.newton_total
    ens.close()
    for row, b in enumerate(LONG_BARS):
        ref = _oracle_run(fam, b, n_cells, n_steps, False)
        assert np.abs(ref["end"]["sigma"]).max() <= 10.0  # stable, as measured: 5.8e-2 (CG), 3.3 (DG)
        _check_state(f"{fam} 500 steps bar {b}", fam, n_cells, got, row, ref, None if b == 4 else MIN_FRAC[fam])
    two = _ensemble(fam, LONG_BARS, n_cells)
    two.solve(250)
    two.solve(250)
    _same(_state(two), got, "250 + 250")
    assert np.array_equal(two.newton_total, total)
    two.close()


# ---- 5. the single-bar device path -----------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_against_single_bar_path(fam):
    """The geometry.create_mesh graded bar, 20 steps at main.py's T_0 = 800 K: an ensemble
    over htc against three ThermoViscoProblem(model_mode="paper") runs."""
    _torch()
    from geometry import graded_bar
    from tvfem import ThermoViscoEnsemble
    from tvfem.problem import ThermoViscoProblem
    htcs = [100.0, 280.1, 700.0]
    mesh = graded_bar()
    n_cells = mesh.n_cells[0]
    ens = ThermoViscoEnsemble(mesh, (0.0, 2.0), DT, CFGS[fam], dict(O.MAIN_MODEL_PARAMS, htc=np.array(htcs)),
                              model_mode="paper")
    ens.setup()
    assert ens.n_steps == 20
    ens.solve(19)
    T_before = ens.get_field("T")
    ens.solve(1)
    got = _state(ens)
    ens.close()
    for row, htc in enumerate(htcs):
        dev = ThermoViscoProblem(mesh, (0.0, 2.0), DT, CFGS[fam], dict(O.MAIN_MODEL_PARAMS, htc=htc), verbose=False,
                                 write_output=False, model_mode="paper")
        dev.setup()
        dev.solve(19)
        Tb = np.array(dev.functions_current["T"].x.array)
        dev.solve(1)
        Td = np.array(dev.functions_current["T"].x.array)
        e = relerr(got["T"][row], Td)
        print(f"[ensemble paper] {fam} single-bar path htc {htc}: T rel {e:.2e}")
        assert e <= 1e-10, (htc, e)
        assert relerr(T_before[row], Tb) <= 1e-10
        _, mS = cond_mask(Td, Tb, src_map=_src(fam, n_cells))
        want = {"sigma": np.array(dev.functions_next["sigma"].x.array)}
        for k in STRESS[1:]:
            want[k] = np.array(dev.functions_current[k].x.array)
        vol = float(np.linalg.norm(want["sigma_partial"]))
        for k in STRESS:
            assert np.all(np.isfinite(want[k])), k
            check_field(f"{fam} htc {htc} {k}", got[k][row], want[k], mS, 1 if k == "sigma" else 6,
                        scale=vol if k.startswith("s_") else None)
        dev.close()


# ---- 6. the failure contract -----------------------------------------------------------------
@pytest.mark.parametrize("error_on_nonconvergence", [True, False])
@pytest.mark.parametrize("fam", FAMS)
def test_failure_semantics(fam, error_on_nonconvergence):
    """newton_max_it = 1: every bar fails its first step, is restored and frozen, and the
    stress memory stays zero.  Then two bars failed through a NaN state: the others
    advance bitwise as without them."""
    _torch()
    from tvfem import NativeError
    from tvfem import _native as N
    n_cells = 16
    ens = _ensemble(fam, list(range(10)), n_cells, newton_max_it=1, error_on_nonconvergence=error_on_nonconvergence)
    init = _state(ens)
    if error_on_nonconvergence:
        with pytest.raises(NativeError) as exc:
            ens.solve(3)
        assert exc.value.code == N.TV_ERR_NOT_CONVERGED
        assert "bar 0" in str(exc.value) and "step 1" in str(exc.value)
    else:
        ens.solve(3)
    assert np.array_equal(ens.failed_step, np.ones(10, dtype=int))
    assert np.array_equal(ens.newton_iterations, np.ones(10, dtype=int))
    got = _state(ens)
    ens.close()
    assert np.array_equal(got["T"], got["T_prev"])  # T <- T_prev
    for f in STATE:
        if f != "T":  # the visco state and T_prev are untouched, bit for bit
            assert np.array_equal(got[f], init[f], equal_nan=True), f
    assert np.all(got["s_partial"] == 0.0) and np.all(got["sigma_partial"] == 0.0)
    assert np.all(got["Tf"] == np.array([b[1] for b in BARS])[:, None])  # Tf stays T_0
    # bars 2 and 7 fail at step 1 (NaN never converges), the others advance as if alone with them
    good = _ensemble(fam, list(range(10)), n_cells)
    good.solve(3)
    want = _state(good)
    good.close()
    ens = _ensemble(fam, list(range(10)), n_cells, error_on_nonconvergence=error_on_nonconvergence)
    T = ens.get_field("T")
    T[[2, 7]] = np.nan
    ens.set_field("T", T)
    before = _state(ens)
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
    got = _state(ens)
    ens.close()
    for f in STATE:
        assert np.array_equal(got[f][ok], want[f][ok], equal_nan=True), f
        if f != "T":
            assert np.array_equal(got[f][~ok], before[f][~ok], equal_nan=True), f
    assert np.array_equal(got["T"][~ok], before["T_prev"][~ok])


# ---- 7. thermal-only steps -------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_thermal_only(fam):
    _torch()
    n_cells = 16
    ens = _ensemble(fam, list(range(10)), n_cells)
    init = _state(ens)
    ens.solve(3, thermal_only=True)
    got = _state(ens)
    assert not ens.failed_step.any()
    ens.close()
    _same(got, init, "thermal_only", VISCO)  # all nine visco fields untouched
    assert np.array_equal(got["T_prev"], got["T"])
    full = _ensemble(fam, list(range(10)), n_cells)
    full.solve(3)
    assert np.array_equal(full.get_field("T"), got["T"])
    full.close()


# ---- 8. schedules and histories --------------------------------------------------------------
def _scheduled(fam, rows, n_cells, schedule=True, **kw):
    """test_ensemble_schedule._scheduled in paper mode, either config."""
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
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFGS[fam], mp, schedule=sched, model_mode="paper", **kw)
    ens.setup()
    return ens


@functools.lru_cache(maxsize=None)
def _scheduled_oracle(fam, row, n_cells):
    """Bar `row` of SBARS through the paper oracle, its ThermalParams set to the step's stage."""
    T0, eps, L, graded, stages = SBARS[row]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=T0, epsilon=eps, htc=stages[0][1], T_ambient=stages[0][2])
    ref = O.OracleProblem(O.rectilinear_mesh([_graded(L, graded, n_cells)]), (0.0, 50.0), DT, CFGS[fam], mp,
                          linear="direct", model_mode="paper")
    ref.setup()
    Ts, T_before = [], None
    with np.errstate(all="ignore"):
        for step in range(1, N_STEPS + 1):
            _, htc, Ta = stages[_stage_of(stages, step)]
            ref.tp.htc, ref.tp.T_ambient, ref.tp.epsilon = htc, Ta, eps
            T_before = ref.functions_current["T"].copy()
            ref.solve_timestep()
            Ts.append(ref.functions_current["T"].copy())
    return {"Ts": Ts, "T_before": T_before, "end": _oracle_end(ref)}


@pytest.mark.parametrize("n_cells", [1, 3, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_schedule_parity_with_oracle(fam, n_cells):
    """The six SBARS as they are (the paper oracle stays finite on all of them over the
    8 steps, at most 1.1e75: _oracle_end asserts it).  By the oracle's T every node of
    these bars is well-conditioned in step 8 except the core of bar 0 with DG at 16 cells
    (compared fraction 0.71), so MIN_FRAC applies to all six."""
    _torch()
    rows = list(range(6))
    refs = [_scheduled_oracle(fam, r, n_cells) for r in rows]
    ens = _scheduled(fam, rows, n_cells)
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
        _check_state(f"{fam} scheduled n_cells {n_cells} bar {r}", fam, n_cells, got, r, refs[r], MIN_FRAC[fam])


def _ten(fam, n_cells, values=None, **kw):
    """The ten BARS; `values` replaces (htc, T_ambient, epsilon) of creation."""
    from tvfem import RectilinearMesh, ThermoViscoEnsemble
    htc, Ta, eps = values if values is not None else _own()
    mp = dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=np.array([b[1] for b in BARS]), T_ambient=Ta, epsilon=eps)
    meshes = [RectilinearMesh([_coords(i, n_cells)]) for i in range(10)]
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, CFGS[fam], mp, model_mode="paper", **kw)
    ens.setup()
    return ens


def _own():
    return tuple(np.array([b[c] for b in BARS]) for c in (0, 2, 3))


@pytest.mark.parametrize("fam", FAMS)
def test_schedule_that_changes_nothing_changes_no_bit(fam):
    _torch()
    n_cells = 16
    plain = _ten(fam, n_cells)
    plain.solve(N_STEPS)
    want = _state(plain)
    plain.close()
    htc, Ta, eps = _own()
    one = [dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    three = [dict(until_step=np.arange(10) % 4, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(until_step=np.arange(10) % 4 + np.arange(10) % 3 * 2, htc=htc, T_ambient=Ta, epsilon=eps),
             dict(htc=htc, T_ambient=Ta, epsilon=eps)]
    for tag, sched in (("one stage", one), ("three equal stages", three)):
        ens = _ten(fam, n_cells, schedule=sched)
        ens.solve(N_STEPS)
        _same(_state(ens), want, tag)
        ens.close()


@pytest.mark.parametrize("n_cells", [3, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_stage_change_is_a_restart(fam, n_cells):
    """Two stages with the shared end k = 3 against two unscheduled ensembles, the second
    started from the first one's eleven state fields (set_field on the two new ones)."""
    _torch()
    k = 3
    htc, Ta, eps = _own()
    htc2, Ta2, eps2 = htc[::-1].copy(), Ta - 40.0, np.clip(eps + 0.05, 0.0, 1.0)[::-1].copy()
    sch = _ten(fam, n_cells, schedule=[dict(until_step=k, htc=htc, T_ambient=Ta, epsilon=eps),
                                       dict(htc=htc2, T_ambient=Ta2, epsilon=eps2)])
    sch.solve(N_STEPS)
    got = _state(sch)
    sch.close()
    first = _ten(fam, n_cells)
    first.solve(k)
    mid = _state(first)
    first.close()
    # (s_partial is exactly zero in 1D, no deviatoric strain: its set_field is shown to move values in
    # test_partial_stress_fields_exist_only_on_a_paper_handle)
    assert np.abs(mid["sigma_partial"]).max() > 0.0
    second = _ten(fam, n_cells, values=(htc2, Ta2, eps2))
    for f in STATE:
        second.set_field(f, mid[f])
    _same(_state(second), mid, "set_field / get_field round trip")
    second.solve(N_STEPS - k)
    _same(got, _state(second), f"n_cells {n_cells}")
    second.close()


@pytest.mark.parametrize("n_cells", [1, 16])
@pytest.mark.parametrize("fam", FAMS)
def test_history(fam, n_cells):
    """Records bitwise equal to get_field of a twin stepped `every` steps at a time: T and
    Tf at the probe node's source dof, sigma at the node; recording changes no state bit."""
    _torch()
    rows = list(range(6))
    probes = [0, n_cells // 2, n_cells]
    src = _src(fam, n_cells)[probes]
    ens = _scheduled(fam, rows, n_cells, history=dict(nodes=probes, every=2))
    ens.solve(N_STEPS)
    h = ens.get_history()
    assert np.array_equal(h["step"], [2, 4, 6, 8]) and np.allclose(h["t"], [0.2, 0.4, 0.6, 0.8])
    assert h["T"].shape == h["Tf"].shape == h["sigma"].shape == (4, 6, 3)
    for name in ("T", "Tf", "sigma"):
        assert np.all(np.isfinite(h[name])), name
    twin = _scheduled(fam, rows, n_cells)
    for rec in range(4):
        twin.solve(2)
        assert np.array_equal(h["T"][rec], twin.get_field("T")[:, src]), rec
        assert np.array_equal(h["Tf"][rec], twin.get_field("Tf")[:, src]), rec
        assert np.array_equal(h["sigma"][rec], twin.get_field("sigma")[:, probes]), rec
    _same(_state(ens), _state(twin), "with / without a history")
    twin.close()
    ens.close()
    for r in rows:  # and the recorded T is the oracle's
        ref = _scheduled_oracle(fam, r, n_cells)
        for rec in range(4):
            assert relerr(h["T"][rec, r], ref["Ts"][2 * rec + 1][src]) <= 1e-10, (n_cells, r, rec)


# ---- 9. fields of the two kinds of handle ----------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_partial_stress_fields_exist_only_on_a_paper_handle(fam):
    _torch()
    from tvfem import NativeError
    from tvfem import _native as N
    n_cells = 5
    ref = _ensemble(fam, [0, 1, 2], n_cells, model_mode="reference")
    for name in ("s_partial", "sigma_partial"):
        with pytest.raises(NativeError) as exc:
            ref.get_field(name)
        assert exc.value.code == N.TV_ERR_STATE, name
        with pytest.raises(NativeError) as exc:
            ref.set_field(name, np.zeros((3, 6 * (n_cells + 1))))
        assert exc.value.code == N.TV_ERR_STATE, name
    ref.close()
    pap = _ensemble(fam, [0, 1, 2], n_cells)
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
