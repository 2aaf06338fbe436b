"""Auxiliary-space multigrid for DG1 temperature on general quadrilateral /
hexahedral meshes (options.preconditioner = TV_PC_AUX: csrc/tv_umdg_aux.hip,
csrc/tv_amg.cpp aux_setup), the preconditioner in PCGAMG's role
(ThermoViscoProblem.py:343-346) for the reference's own DG1 / CG1 pairing:

  * the cycle (tv_precond_apply, the PCApply of the solve) is pinned to the numpy
    restatement tests/dg_aux_reference.py, built on the oracle's assembled
    operators: relative error <= 1e-10, symmetry <= 1e-12 (the bars of
    tests/test_amg.py::test_amg_vcycle_matches_restatement), r.z > 0;
  * the Newton solution is pinned to the oracle's Jacobi-PCG steps (T <= 1e-10 per
    step; the preconditioner only changes the Krylov counts, which must fall) and,
    on the stiff `quad3`, to the device's own Jacobi path, pinned elsewhere.

Meshes: `quad` (72 cells) and `hex` (140 cells) of tests/test_unstructured_dg.py --
no multiple of 64, the last wave part padding, two levels -- and `quad3` (2,115
cells, 2,208 vertices: off multiples of 64, more than 2000 vertices, so one
aggregation level below CG1; dt alpha / h^2 ~ 54).  A three-level hexahedral case
is left out: its oracle assembly takes most of a minute, and the levels below CG1
are the dimension-blind code tests/test_amg.py covers in 3D.
"""
import functools

import numpy as np
import pytest

from dg_aux_reference import AuxCycle, aux_mesh
from oracle import tv_oracle as O
from parity_util import check_field, relerr
from test_unstructured_dg import config, device, device_layout, host_layout, mesh, oracle_steps

pytestmark = pytest.mark.gpu

LEVELS = {"quad": 2, "hex": 2, "quad3": 3}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def aux_device(name, fT="DG", fS="CG", mode="reference", **kw):
    from tvfem.problem import ThermoViscoProblem
    return ThermoViscoProblem(aux_mesh(name), (0.0, 1.0), 0.1, config(fT, fS), dict(O.MAIN_MODEL_PARAMS),
                              verbose=False, model_mode=mode, **kw)


def _cycle_against_restatement(torch, dev, name, mg_levels=0):
    """tv_precond_apply at T = 700 + U(0, 150) against the restatement: (error, symmetry, r.z, levels)"""
    d = aux_mesh(name).dim
    n = aux_mesh(name).num_cells * 2 ** d
    rng = np.random.default_rng(5)
    T = 700.0 + rng.uniform(0.0, 150.0, n)
    dev.set_field("T", T)
    dev._flush()
    cyc = AuxCycle(name, T, mg_levels=mg_levels)
    r, y = rng.standard_normal((2, n))
    out = []
    for v in (r, y):
        vd = torch.tensor(device_layout(d, v), dtype=torch.float64, device="cuda")
        zd = torch.empty_like(vd)
        assert dev._lib.tv_precond_apply(dev._ctx, vd.data_ptr(), zd.data_ptr()) == 0, dev._lib.tv_last_error(dev._ctx)
        out.append(host_layout(d, zd.cpu().numpy()))
    z_r, z_y = out
    return relerr(z_r, cyc.apply(r)), abs(y @ z_r - r @ z_y) / abs(y @ z_r), r @ z_r, cyc


# ---- 1. the cycle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quad", "hex", "quad3"])
def test_aux_cycle_matches_restatement(name):
    torch = _torch()
    dev = aux_device(name, preconditioner="aux")
    dev.setup()
    e, sym, rz, cyc = _cycle_against_restatement(torch, dev, name)
    dev.close()
    print(f"[um dg aux] cycle {name}: {cyc.n_levels} levels ({[lv[0].shape[0] for lv in cyc.levels]}), omega0 "
          f"{cyc.omega0:.4f}, vs numpy {e:.2e}, symmetry {sym:.1e}")
    assert cyc.n_levels == LEVELS[name]
    assert e <= 1e-10, e
    assert sym <= 1e-12, sym
    assert rz > 0.0


# ---- 2. steps against the oracle -------------------------------------------------------------
@pytest.mark.parametrize("name,fT,fS,mode", [("quad", "DG", "CG", "reference"), ("hex", "DG", "CG", "reference"),
                                             ("hex_ordered", "DG", "CG", "reference"), ("hex", "DG", "DG", "paper")])
def test_aux_steps_match_oracle(name, fT, fS, mode):
    _torch()
    want = oracle_steps(name, fT, fS, mode)
    dev = device(name, fT, fS, mode, preconditioner="aux")
    dev.setup()
    its, errs = [], []
    for s in range(len(want["T"])):
        dev.solve_timestep()
        its.append((dev.last_newton_iterations, dev.last_krylov_iterations))
        errs.append(relerr(dev.functions_current["T"].x.array, want["T"][s]))
    sigma = np.array(dev.functions_next["sigma"].x.array)
    dev.close()
    k_dev, k_ref = sum(k for _, k in its), sum(k for _, k in want["history"])
    print(f"[um dg aux] {name} {fT}/{fS} {mode}: T per step {['%.1e' % e for e in errs]}, (Newton, Krylov) {its} "
          f"oracle (Jacobi) {want['history']}: {k_dev} against {k_ref} Krylov iterations")
    assert max(errs) <= 1e-10, errs
    for (n_d, _), (n_r, _) in zip(its, want["history"]):
        assert abs(n_d - n_r) <= 1, (its, want["history"])
    assert 3 * k_dev < 2 * k_ref, (k_dev, k_ref)
    check_field(f"sigma[{name},{fT}/{fS},{mode},aux]", sigma, want["sigma"], want["mS"], mesh(name).dim ** 2,
                min_frac=0.9)


# ---- 3. the drop at stiffness ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quad3_jacobi_steps():
    """two steps of `quad3` on the device's Jacobi path (pinned by tests/test_unstructured_dg.py), read only"""
    dev = aux_device("quad3")
    dev.setup()
    Ts, its = [], []
    for _ in range(2):
        dev.solve_timestep()
        Ts.append(np.array(dev.functions_current["T"].x.array))
        its.append((dev.last_newton_iterations, dev.last_krylov_iterations))
    dev.close()
    return Ts, its


def _quad3_steps(**kw):
    dev = aux_device("quad3", preconditioner="aux", **kw)
    dev.setup()
    Ts, its = [], []
    for _ in range(2):
        dev.solve_timestep()
        Ts.append(np.array(dev.functions_current["T"].x.array))
        its.append((dev.last_newton_iterations, dev.last_krylov_iterations))
    return dev, Ts, its


def test_aux_cuts_the_iterations_at_stiffness():
    _torch()
    T_j, its_j = quad3_jacobi_steps()
    dev, T_a, its_a = _quad3_steps()
    dev.close()
    errs = [relerr(a, j) for a, j in zip(T_a, T_j)]
    k_a, k_j = sum(k for _, k in its_a), sum(k for _, k in its_j)
    print(f"[um dg aux] quad3: T aux vs Jacobi {['%.1e' % e for e in errs]}, (Newton, Krylov) aux {its_a} Jacobi "
          f"{its_j}: {k_a} against {k_j} Krylov iterations")
    assert max(errs) <= 1e-10, errs
    for (n_a, _), (n_j, _) in zip(its_a, its_j):
        assert abs(n_a - n_j) <= 1, (its_a, its_j)
    assert 4 * k_a < k_j, (k_a, k_j)


# ---- 4. reproducible -------------------------------------------------------------------------
def test_aux_is_bitwise_reproducible():
    _torch()
    runs = []
    for _ in range(2):
        dev = device("hex", preconditioner="aux")
        dev.setup()
        for _ in range(2):
            dev.solve_timestep()
        runs.append((np.array(dev.functions_current["T"].x.array), np.array(dev.functions_next["sigma"].x.array),
                     dev.last_krylov_iterations))
        dev.close()
    (Ta, Sa, ka), (Tb, Sb, kb) = runs
    assert ka == kb
    assert np.array_equal(Ta.view(np.uint64), Tb.view(np.uint64))
    assert np.array_equal(Sa.view(np.uint64), Sb.view(np.uint64))


# ---- 5. DG + CG1 only ------------------------------------------------------------------------
def test_aux_two_levels_on_request():
    torch = _torch()
    T_j, _ = quad3_jacobi_steps()
    dev, T_a, its_a = _quad3_steps(mg_levels=2)
    dev.close()
    errs = [relerr(a, j) for a, j in zip(T_a, T_j)]
    # a fresh context: the level-0 weight is estimated once, at the temperature of the first application
    dev = aux_device("quad3", preconditioner="aux", mg_levels=2)
    dev.setup()
    e, sym, rz, cyc = _cycle_against_restatement(torch, dev, "quad3", mg_levels=2)
    dev.close()
    print(f"[um dg aux] quad3, mg_levels=2: T vs Jacobi {['%.1e' % x for x in errs]}, (Newton, Krylov) {its_a}; "
          f"cycle vs numpy {e:.2e}, symmetry {sym:.1e}")
    assert cyc.n_levels == 2 and len(cyc.levels) == 1
    assert max(errs) <= 1e-10, errs
    assert e <= 1e-10 and sym <= 1e-12 and rz > 0.0


# ---- 6. refusals and the public names --------------------------------------------------------
def test_aux_refusals_name_their_reason():
    _torch()
    from tvfem import RectilinearMesh
    from tvfem import _native as N
    from tvfem.problem import ThermoViscoProblem
    with pytest.raises(N.NativeError) as ei:
        device("quad", "CG", "CG", preconditioner="aux")
    assert ei.value.code == N.TV_ERR_ARG and "TV_PC_AUX needs a DG temperature" in str(ei.value)
    assert "TV_PC_AMG" in str(ei.value)
    with pytest.raises(N.NativeError) as ei:
        device("quad", preconditioner="amg")  # unchanged, and now points here
    assert ei.value.code == N.TV_ERR_ARG and "TV_PC_AMG needs a CG temperature" in str(ei.value)
    assert "TV_PC_AUX" in str(ei.value)
    axes = [np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 4), np.linspace(0.0, 0.5, 3)]
    with pytest.raises(N.NativeError) as ei:
        ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, config("DG", "CG"), dict(O.MAIN_MODEL_PARAMS),
                           verbose=False, preconditioner="aux")
    assert ei.value.code == N.TV_ERR_ARG and "TV_PC_GMG" in str(ei.value)
    with pytest.raises(N.NativeError) as ei:
        device("hex", n_parts=2, part=0, preconditioner="aux")
    assert ei.value.code == N.TV_ERR_ARG and "CG temperature and stress spaces only" in str(ei.value)
    ok = device("quad", mode="paper", preconditioner="aux")  # (reference mode refuses any Dirichlet condition)
    assert ok._lib.tv_set_dirichlet(ok._ctx, 1, 300.0) == N.TV_ERR_STATE
    assert "TV_PC_AUX" in ok._lib.tv_last_error(ok._ctx).decode()
    ok.setup()
    assert ok.ksp.getPC().getType() == "gamg"
    ok.solve_timestep()
    ok.close()


# ---- 7. several cell groups per wave ---------------------------------------------------------
def test_aux_large_quadrilateral_grid():
    """768 x 704 = 540,672 cells and 541,645 vertices: above 2048 workgroups x 4 waves x 64 items, where
    every wave of the level-0 kernels takes several cell / vertex groups (no smaller mesh reaches that loop;
    the mesh of tests/test_unstructured_dg.py::test_large_quadrilateral_grid_operators_match_box_dg_path).
    The oracle does not assemble this size, so: the cycle is symmetric (1e-12, the bar above) and positive,
    and one step agrees with the device's Jacobi path (1e-10) at under a quarter of its Krylov iterations
    (dt alpha / h^2 = 40, the stiffness of `quad3`: a cycle that missed groups would not reach either)."""
    torch = _torch()
    from tvfem import RectilinearMesh, UnstructuredMesh
    from tvfem.problem import ThermoViscoProblem
    m = UnstructuredMesh.from_rectilinear(RectilinearMesh([np.linspace(0.0, 38.4, 769), np.linspace(0.0, 35.2, 705)]))
    out = {}
    for pc in ("jacobi", "aux"):
        p = ThermoViscoProblem(m, (0.0, 1.0), 0.1, config("DG", "CG"), dict(O.MAIN_MODEL_PARAMS), verbose=False,
                               preconditioner=pc)
        p.setup()
        p.solve_timestep()
        out[pc] = (np.array(p.functions_current["T"].x.array), p.last_newton_iterations, p.last_krylov_iterations)
        if pc == "aux":
            n = p.num_dofs(0)[0]
            assert n == 4 * 768 * 704
            rng = np.random.default_rng(7)
            r, y = (torch.tensor(v, dtype=torch.float64, device="cuda") for v in rng.standard_normal((2, n)))
            zr, zy = torch.empty_like(r), torch.empty_like(r)
            assert p._lib.tv_precond_apply(p._ctx, r.data_ptr(), zr.data_ptr()) == 0
            assert p._lib.tv_precond_apply(p._ctx, y.data_ptr(), zy.data_ptr()) == 0
            sym = abs(float(y @ zr) - float(r @ zy)) / abs(float(y @ zr))
            rz = float(r @ zr)
        p.close()
    e = relerr(out["aux"][0], out["jacobi"][0])
    print(f"[um dg aux] 540,672 quadrilaterals: T aux vs Jacobi {e:.1e}, (Newton, Krylov) aux {out['aux'][1:]} "
          f"Jacobi {out['jacobi'][1:]}, cycle symmetry {sym:.1e}")
    assert sym <= 1e-12 and rz > 0.0
    assert e <= 1e-10
    assert abs(out["aux"][1] - out["jacobi"][1]) <= 1
    assert 4 * out["aux"][2] < out["jacobi"][2]
