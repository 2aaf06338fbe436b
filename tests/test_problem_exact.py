"""ThermoViscoProblem(model_mode="paper", relaxation="exact"): the exact kernels of csrc/tv_visco.hip
(k_visco_fused_exact, k_visco_S_exact) in 1D, 2D and 3D, box and general meshes.

Cases, parameters and step count: tests/problem_exact_cases.py (T_0 = 920 K, 8 steps).

1. Stress parity with a DRIVEN oracle.  The oracle (unchanged, inside tests/exact_relaxation.py) does not
   solve T: after every device step the device's T is copied into it and its visco_update() runs, so the
   comparison is of the update alone (nobody has shown that the device's Krylov iterates and the oracle's agree
   to 1e-10 at 920 K; test 2 pins T instead).  Tolerances of tests/test_paper_mode.py: Tf, Tf_partial <= 1e-10,
   phi, xi <= 1e-9, sigma and the four partial stresses by check_field at 1e-6 (deviatoric pair on the
   volumetric scale), mask from the last step's T change, min_frac 0.9.  A second oracle driven by the same T
   WITHOUT the patch must differ from the patched one by more than 1e-3 rel. L2 in sigma: at 920 K the Taylor
   polynomial has left the exponential (at main.py's 800 K the two differ by 4e-7 .. 1e-4 only and a parity
   test could not tell them apart).
2. Only the stress sees it: an exact problem and its Taylor twin hold the same bits in T, T_prev, Tf,
   Tf_partial, phi, xi and take the same Newton / Krylov counts after every step; the exact sigma is finite
   and below 1; on 3d_cg the twin's exceeds 1e6 after 8 steps (oracle: 3.1e12).  A problem created Taylor and
   switched with set_relaxation("exact") before step 1 is bitwise the exact one in every field.
3. 1D against ThermoViscoEnsemble(model_mode="paper", relaxation="exact"): geometry.graded_bar(), both
   pairings, htc 100 / 280.1 / 700 with T_0 800 / 873 / 920, 20 steps (the construction of
   tests/ensemble_parity.against_single_bar_path): T <= 1e-10, the five stress fields by check_field.
4. The setter's contract on a live context.
5. General meshes (tv_create_unstructured): the distorted quad / hex meshes of tests/test_unstructured.py,
   exact against Taylor as in 2.
"""
import numpy as np
import pytest

from exact_relaxation import exact_relaxation
from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr
from problem_exact_cases import (CASES, CG, DG, DT, MP, N_STEPS, STRESS, THERMAL, fields, gpu, oracle, problem,
                                 same_bits)

pytestmark = pytest.mark.gpu


# ---- 1. the driven oracle --------------------------------------------------------------------
def _drive(ref, T, exact):
    ref.functions_current["T"][:] = T
    with np.errstate(all="ignore"):
        if exact:
            with exact_relaxation():
                ref.visco_update()
        else:
            ref.visco_update()
    ref.functions_previous["T"][:] = ref.functions_current["T"]


@pytest.mark.parametrize("materialize", [True, False], ids=["materialized", "lean"])
@pytest.mark.parametrize("name", list(CASES))
def test_stress_matches_driven_oracle(name, materialize):
    gpu()
    dev = problem(name, materialize=materialize)
    assert (dev.model_mode, dev.relaxation) == ("paper", "exact")
    ref, tay = oracle(name), oracle(name)
    dev.setup()
    for _ in range(N_STEPS):
        T_before = ref.functions_current["T"].copy()
        dev.solve_timestep()
        T = np.array(dev.functions_current["T"].x.array)
        _drive(ref, T, True)
        _drive(tay, T, False)
    d2 = len(CASES[name][0]) ** 2
    fc, fn, f = ref.functions_current, ref.functions_next, ref.functions
    for k, v in (("Tf", fc["Tf"]), ("Tf_partial", fc["Tf_partial"]), ("phi", f["phi"]), ("xi", f["xi"]),
                 ("sigma", fn["sigma"])) + tuple((k, fc[k]) for k in STRESS[1:]):
        assert np.all(np.isfinite(v)), f"the oracle's {k} is not finite"
    mT = np.abs(ref.functions_current["T"] - T_before) > 1e-6
    mS = mT[ref._maps[("S", "T")]]
    for k, got, want, tol in (("Tf_partial", dev.functions_current["Tf_partial"].x.array, fc["Tf_partial"], 1e-10),
                              ("Tf", dev.functions_current["Tf"].x.array, fc["Tf"], 1e-10),
                              ("phi", dev.functions["phi"].x.array, f["phi"], 1e-9),
                              ("xi", dev.functions["xi"].x.array, f["xi"], 1e-9)):
        e = relerr(got, want)
        print(f"[problem exact] {name}: {k} rel {e:.2e}")
        assert e < tol, (k, e)
    sig = np.array(dev.functions_next["sigma"].x.array)
    assert np.all(np.isfinite(sig))
    check_field(f"sigma[{name},exact]", sig, fn["sigma"], mS, d2, min_frac=0.9)
    vol = float(np.linalg.norm(fc["sigma_partial"]))
    for k in STRESS[1:]:
        check_field(f"{k}[{name},exact]", dev.functions_current[k].x.array, fc[k], mS, 6 * d2, min_frac=0.9,
                    scale=vol if k.startswith("s_") else None)
    dev.close()
    # the test can tell the two relaxations apart
    d = float(np.linalg.norm(tay.functions_next["sigma"] - fn["sigma"]) / np.linalg.norm(fn["sigma"]))
    print(f"[problem exact] {name}: Taylor oracle vs exact oracle, sigma rel {d:.3e}; max |sigma| exact "
          f"{np.abs(fn['sigma']).max():.3e}")
    assert d > 1e-3, d


# ---- 2. only the stress sees it --------------------------------------------------------------
def _twins(mk, setup_kw=None, taylor_above=None, switched=True, steps=N_STEPS):
    ex, ta = mk("exact"), mk("taylor")
    sw = mk("taylor") if switched else None
    assert (ex.relaxation, ta.relaxation) == ("exact", "taylor")
    for p in (ex, ta, sw):
        if p is not None:
            p.setup(**(setup_kw or {}))
    if sw is not None:
        sw.set_relaxation("exact")
        assert sw.relaxation == "exact"
    for s in range(steps):
        for p in (ex, ta, sw):
            if p is not None:
                with np.errstate(all="ignore"):
                    p.solve_timestep()
        fe, ft = fields(ex), fields(ta, THERMAL + ("sigma",))
        for k in THERMAL:
            assert same_bits(fe[k], ft[k]), (s, k)
        assert (ex.last_newton_iterations, ex.last_krylov_iterations) == \
            (ta.last_newton_iterations, ta.last_krylov_iterations), s
        assert np.all(np.isfinite(fe["sigma"])) and np.abs(fe["sigma"]).max() < 1.0, (s, np.abs(fe["sigma"]).max())
        if sw is not None:
            fs = fields(sw)
            for k in fe:
                assert same_bits(fs[k], fe[k]), (s, k)
    smax_e, smax_t = float(np.abs(fe["sigma"]).max()), float(np.abs(ft["sigma"]).max())
    print(f"[problem exact] twins: max |sigma| exact {smax_e:.3e}, Taylor {smax_t:.3e}")
    assert not same_bits(fe["sigma"], ft["sigma"])
    if taylor_above is not None:
        assert smax_t > taylor_above, smax_t
    for p in (ex, ta, sw):
        if p is not None:
            p.close()


@pytest.mark.parametrize("name,dirichlet", [("1d_cg", False), ("2d_dg_cg", False), ("3d_cg", False), ("2d_cg", True)],
                         ids=["1d_cg", "2d_dg_cg", "3d_cg", "2d_cg_dirichlet"])
def test_only_the_stress_sees_the_relaxation(name, dirichlet):
    gpu()
    _twins(lambda relaxation: problem(name, relaxation=relaxation), dict(dirichlet_bc=True) if dirichlet else None,
           taylor_above=1e6 if name == "3d_cg" else None)


# ---- 3. 1D against the ensemble --------------------------------------------------------------
@pytest.mark.parametrize("fam", ["cg", "dg"])
def test_graded_bar_matches_exact_ensemble(fam):
    gpu()
    from geometry import graded_bar
    from tvfem import ThermoViscoEnsemble
    from tvfem.problem import ThermoViscoProblem
    cfg = {"T": CG if fam == "cg" else DG, "sigma": CG}
    sets = list(zip([100.0, 280.1, 700.0], [800.0, 873.0, 920.0]))  # htc, T_0
    mesh = graded_bar()
    n_cells = mesh.n_cells[0]
    ens = ThermoViscoEnsemble(mesh, (0.0, 2.0), DT, cfg,
                              dict(O.MAIN_MODEL_PARAMS, htc=np.array([s[0] for s in sets]),
                                   T_0=np.array([s[1] for s in sets])), model_mode="paper", relaxation="exact")
    ens.setup()
    assert ens.n_steps == 20
    ens.solve(19)
    T_before = ens.get_field("T")
    ens.solve(1)
    got = {k: ens.get_field(k) for k in ("T",) + STRESS}
    ens.close()
    src = np.arange(n_cells + 1) if fam == "cg" else np.append(2 * np.arange(n_cells), 2 * n_cells - 1)
    for row, (htc, T0) in enumerate(sets):
        dev = ThermoViscoProblem(mesh, (0.0, 2.0), DT, cfg, dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=T0),
                                 verbose=False, write_output=False, model_mode="paper", relaxation="exact")
        dev.setup()
        dev.solve(19)
        Tb = np.array(dev.functions_current["T"].x.array)
        dev.solve(1)
        Td = np.array(dev.functions_current["T"].x.array)
        e = relerr(got["T"][row], Td)
        print(f"[problem exact] ensemble {fam} htc {htc} T_0 {T0}: T rel {e:.2e}")
        assert e <= 1e-10, (htc, e)
        assert relerr(T_before[row], Tb) <= 1e-10
        _, mS = cond_mask(Td, Tb, src_map=src)
        want = {"sigma": np.array(dev.functions_next["sigma"].x.array)}
        for k in STRESS[1:]:
            want[k] = np.array(dev.functions_current[k].x.array)
        vol = float(np.linalg.norm(want["sigma_partial"]))
        for k in STRESS:
            assert np.all(np.isfinite(want[k])), k
            check_field(f"ensemble {fam} htc {htc} {k}", got[k][row], want[k], mS, 1 if k == "sigma" else 6,
                        scale=vol if k.startswith("s_") else None)
        dev.close()


# ---- 4. the setter's contract ----------------------------------------------------------------
def test_setter_contract_on_a_reference_context():
    gpu()
    from tvfem import _native as N
    a = problem("2d_cg", relaxation="taylor", model_mode="reference", mp=O.MAIN_MODEL_PARAMS)
    b = problem("2d_cg", relaxation="taylor", model_mode="reference", mp=O.MAIN_MODEL_PARAMS)
    a.setup()
    b.setup()
    lib = a._lib
    assert lib.tv_set_relaxation(a._ctx, N.TV_RELAX_EXACT) == N.TV_ERR_STATE
    msg = lib.tv_last_error(a._ctx).decode()
    assert "exact relaxation needs paper mode" in msg, msg
    assert lib.tv_set_relaxation(a._ctx, 7) == N.TV_ERR_ARG
    assert lib.tv_set_relaxation(a._ctx, -1) == N.TV_ERR_ARG
    assert lib.tv_set_relaxation(a._ctx, N.TV_RELAX_TAYLOR) == N.TV_OK
    with pytest.raises(ValueError, match="relaxation='exact' needs model_mode='paper'"):
        a.set_relaxation("exact")
    with pytest.raises(ValueError, match="relaxation must be"):
        a.set_relaxation("pade")
    assert a.relaxation == "taylor"
    names = ("T", "T_prev", "Tf", "Tf_partial", "phi", "xi", "sigma", "s_tilde_partial", "sigma_tilde_partial")
    for s in range(2):
        a.solve_timestep()
        b.solve_timestep()
        fa, fb = fields(a, names), fields(b, names)
        for k in names:
            assert same_bits(fa[k], fb[k]), (s, k)
    a.close()
    b.close()
    # a paper context takes both values, and back again is the Taylor twin's next step
    p = problem("1d_cg", relaxation="exact")
    assert lib.tv_set_relaxation(p._ctx, 7) == N.TV_ERR_ARG
    p.set_relaxation("taylor")
    assert p.relaxation == "taylor"
    p.set_relaxation("exact")
    assert p.relaxation == "exact"
    p.close()


# ---- 5. general meshes -----------------------------------------------------------------------
UMESHES = {"quad": ((9, 5), (3.0, 1.0)), "hex": ((7, 5, 4), (2.0, 2.0, 1.0))}  # tests/test_unstructured.py


@pytest.mark.parametrize("name", list(UMESHES))
def test_unstructured_exact_against_taylor(name):
    gpu()
    from tvfem import distorted_box_mesh
    from tvfem.mesh import UnstructuredMesh
    from tvfem.problem import ThermoViscoProblem
    n, L = UMESHES[name]
    m = distorted_box_mesh(L, n, amp=0.2, seed=0, shuffle=True)
    assert isinstance(m, UnstructuredMesh)  # tv_create_unstructured

    def mk(relaxation):
        return ThermoViscoProblem(m, (0.0, 1.0), DT, {"T": CG, "sigma": CG}, dict(MP), verbose=False,
                                  model_mode="paper", relaxation=relaxation)
    _twins(mk)
