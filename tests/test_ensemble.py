"""ThermoViscoEnsemble (csrc/tv_ensemble.hip): many 1D CG1 bars in one launch,
against the CPU oracle bar by bar, against itself (independence of the bars,
padding lanes, launch splitting), against the single-bar device path, and the
failure contract.

Tolerances: T rel. L2 <= 1e-10 per bar at every compared step (the project's
step tolerance); phi / Tf / xi / sigma through parity_util.check_field with
its tolerances; Newton counts equal wherever the oracle's own decision was at
least a decade from flipping, within one elsewhere (the last iterations of
these solves sit at rounding level, where a count can legitimately flip).
"""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr

pytestmark = pytest.mark.gpu

CFG = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
DT = 0.1
# htc, T_0, T_ambient, epsilon, L; bar 4 starts in equilibrium (zero residual, xi = 0, NaN stress: Q5)
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
STATE = ["T", "T_prev", "Tf", "Tf_partial", "phi", "xi", "sigma", "s_tilde_partial", "sigma_tilde_partial"]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _coords(bar, n_cells):
    L = BARS[bar][4]
    g = 0.5 if bar % 2 else 0.0
    s = np.linspace(0.0, 1.0, n_cells + 1)
    return L * (g * (1.0 - np.cos(np.pi * s)) / 2.0 + (1.0 - g) * s)


def _params(bar):
    htc, T0, Ta, eps, _ = BARS[bar]
    return dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=T0, T_ambient=Ta, epsilon=eps)


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
    return ref


def _newton_margin(form, T, Tp, rtol=1e-12, atol=1e-10, max_it=50):
    """oracle.newton_solve restated over HeatForm (T is a copy: the oracle's
    own state is untouched): the iteration count and how far, in decades, the
    nearest convergence decision of the solve was from flipping."""
    T = T.copy()
    it, conv, r0, margin = 0, False, 0.0, np.inf
    b = form.residual(T, Tp)
    with np.errstate(divide="ignore", invalid="ignore"):
        while not conv and it < max_it:
            dx = spla.spsolve(form.jacobian(T).tocsc(), b)
            T -= dx
            it += 1
            b = form.residual(T, Tp)
            r = np.linalg.norm(dx)
            if it == 1:
                r0 = r
                continue
            rel = r / r0 if r0 != 0.0 else (np.inf if r != 0.0 else np.nan)
            conv = bool(rel < rtol or r < atol)
            if conv:
                m = np.fmax(np.log10(rtol / rel), np.log10(atol / r))
            else:
                m = np.fmin(np.log10(rel / rtol), np.log10(r / atol))
            margin = min(margin, float(m))
    return it, margin


@functools.lru_cache(maxsize=None)
def _oracle_run(bar, n_cells, n_steps, keep_every_step):
    """One bar through the oracle, computed once per session: T after every
    step (or only the last), the state at the end, T before the last step and
    per step (Newton count, decision margin)."""
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


def _check_end(tag, ens, row, bar, ref):
    """T and the viscoelastic fields of ensemble row `row` against oracle run `ref` of bar `bar`."""
    assert relerr(ens.get_field("T")[row], ref["end"]["T"]) <= 1e-10
    mT, _ = cond_mask(ref["end"]["T"], ref["T_before"])
    for name in ("phi", "Tf", "xi", "sigma"):
        check_field(f"{tag} bar {bar} {name}", ens.get_field(name)[row], ref["end"][name], mT, 1,
                    min_frac=None if bar == 4 else 0.9)


@pytest.mark.parametrize("n_cells", [1, 2, 3, 16])
def test_parity_with_oracle(n_cells):
    _torch()
    n_steps = 6
    bars = list(range(10))
    refs = [_oracle_run(b, n_cells, n_steps, True) for b in bars]
    ens = _ensemble(bars, n_cells)
    strict = total = 0
    for s in range(n_steps):
        ens.solve_timestep()
        T = ens.get_field("T")
        its = ens.newton_iterations
        for b in bars:
            e = relerr(T[b], refs[b]["Ts"][s])
            assert e <= 1e-10, (n_cells, s, b, e)
            want, margin = refs[b]["hist"][s]
            total += 1
            if margin >= 1.0:
                strict += 1
                assert its[b] == want, (n_cells, s, b, int(its[b]), want, margin)
            else:
                assert abs(int(its[b]) - want) <= 1, (n_cells, s, b, int(its[b]), want, margin)
    print(f"[ensemble] n_cells {n_cells}: {strict}/{total} solves in the strict Newton-count group; "
          f"counts {sorted({h[0] for r in refs for h in r['hist']})}")
    assert strict >= 0.6 * total, (strict, total)
    assert not ens.failed_step.any()
    for b in bars:
        _check_end(f"n_cells {n_cells}", ens, b, b, refs[b])
    ens.close()


def test_independence_and_padding():
    """A bar computes the same bits alone, in the ten-bar ensemble, and repeated
    into tail lanes (65 bars), a second wave and a second workgroup (130)."""
    _torch()
    n_cells, n_steps = 16, 6
    ten = _ensemble(list(range(10)), n_cells)
    ten.solve(n_steps)
    want = {f: ten.get_field(f) for f in STATE}
    its = ten.newton_iterations
    ten.close()
    for b in range(10):
        one = _ensemble([b], n_cells)
        one.solve(n_steps)
        for f in STATE:
            assert np.array_equal(one.get_field(f)[0], want[f][b], equal_nan=True), (b, f)
        assert one.newton_iterations[0] == its[b]
        one.close()
    for n_bars in (65, 130):
        idx = [i % 10 for i in range(n_bars)]
        rep = _ensemble(idx, n_cells)
        rep.solve(n_steps)
        for f in STATE:
            assert np.array_equal(rep.get_field(f), want[f][idx], equal_nan=True), (n_bars, f)
        assert np.array_equal(rep.newton_iterations, its[idx])
        rep.close()


def test_long_horizon():
    """500 steps in one solve() against the oracle; solve(250) twice is the same bits."""
    _torch()
    n_cells, n_steps = 16, 500
    bars = [0, 9]
    ens = _ensemble(bars, n_cells)
    ens.solve(n_steps)
    assert abs(ens.t - 50.0) < 1e-9
    for row, b in enumerate(bars):
        _check_end("500 steps", ens, row, b, _oracle_run(b, n_cells, n_steps, False))
    two = _ensemble(bars, n_cells)
    two.solve(250)
    two.solve(250)
    for f in STATE:
        assert np.array_equal(two.get_field(f), ens.get_field(f), equal_nan=True), f
    assert np.array_equal(two.newton_total, ens.newton_total)
    ens.close()
    two.close()


def test_against_single_bar_path():
    """The geometry.create_mesh graded bar, 20 steps: an ensemble over htc against
    three ThermoViscoProblem runs (Jacobi-PCG Newton, launch per operation)."""
    _torch()
    from geometry import graded_bar
    from tvfem import ThermoViscoEnsemble
    from tvfem.problem import ThermoViscoProblem
    htcs = [100.0, 280.1, 700.0]
    mesh = graded_bar()
    ens = ThermoViscoEnsemble(mesh, (0.0, 2.0), DT, CFG, dict(O.MAIN_MODEL_PARAMS, htc=np.array(htcs)))
    ens.setup()
    assert ens.n_steps == 20
    ens.solve(19)
    T_before = ens.get_field("T")
    ens.solve(1)
    T, sigma = ens.get_field("T"), ens.get_field("sigma")
    ens.close()
    for row, htc in enumerate(htcs):
        dev = ThermoViscoProblem(mesh, (0.0, 2.0), DT, CFG, dict(O.MAIN_MODEL_PARAMS, htc=htc), verbose=False,
                                 write_output=False)
        dev.setup()
        dev.solve(19)
        Tb = dev.get_field("T")
        dev.solve(1)
        e = relerr(T[row], dev.get_field("T"))
        assert e <= 1e-10, (htc, e)
        assert relerr(T_before[row], Tb) <= 1e-10
        mT, _ = cond_mask(dev.get_field("T"), Tb)
        check_field(f"htc {htc} sigma", sigma[row], dev.get_field("sigma"), mT, 1)
        dev.close()


@pytest.mark.parametrize("error_on_nonconvergence", [True, False])
def test_failure_semantics(error_on_nonconvergence):
    """newton_max_it = 1: the incremental criterion cannot converge at iteration
    1, so every bar fails its first step, is restored and frozen."""
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
    # bar 4: zero residual, zero increment -- the state is still the initial condition, bit for bit
    for f in STATE:
        assert np.array_equal(ens.get_field(f)[4], init[f][4], equal_nan=True), f
    assert np.all(init["T"][4] == BARS[4][1]) and np.all(init["T_prev"][4] == BARS[4][1])
    ens.close()


def test_thermal_only():
    _torch()
    n_cells = 16
    ens = _ensemble(list(range(10)), n_cells)
    ens.solve(3, thermal_only=True)
    T, sigma = ens.get_field("T"), ens.get_field("sigma")
    assert not ens.failed_step.any()
    ens.close()
    assert np.all(sigma == 0.0)
    for b in range(10):
        ref = _oracle(b, n_cells)
        ref.solve(3, thermal_only=True)
        e = relerr(T[b], ref.functions_current["T"])
        assert e <= 1e-10, (b, e)
