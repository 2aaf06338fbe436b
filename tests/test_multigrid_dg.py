"""The box multigrid for a DG1 temperature (options.preconditioner = TV_PC_GMG
on a rectilinear 3D mesh, benchmark configuration C5's preconditioner) against
its numpy restatement tests/dg_gmg_reference.py, built on the oracle's assembled
operators: tv_precond_apply, the PCApply of the solve.  tests/test_krylov.py
("gmg-dg", "gmg-dg-graded") holds the same cycle as the solve runs it.

What the cycle runs and nothing else does: the fast diagonalisation of the cell
blocks with approximate reciprocals (tv_dg.hip fdm_mul / fdm2), the Robin weight
as the facet mean (k_dg_gface) and its factor dt / (dt alpha), k_dg_bsmooth /
k_dg_bpost, the cell-vertex transfers k_mg_dg_restrict / k_mg_dg_prolong /
k_mg_dg_T, and the weight omega0 = 2 / (1.21 lambda) from 30 power iterations,
estimated at the first apply and kept.

Grids (dg_gmg_reference.GRIDS): `two_blocks` 9 x 7 x 5 cells (315: one full
256-thread block of cells and a partial one, no multiple of 64, odd counts on
every axis; automatic depth: three CG levels), `graded` 7 x 5 x 3 (the
neighbours' lengths in the SIPG penalty), `thin` 1 x 3 x 2 (a Robin facet on both
sides of an axis, both neighbour indices clamped).

Bars: relative L2 <= 1e-10 against the restatement (the project's bar for the
auxiliary-space cycle and for T; the kernel's comment claims about 1e-12 per
reciprocal), symmetry <= 1e-12 and r.Br > 0 as for the CG cycle
(tests/test_multigrid.py).  Everything else is bitwise.

Measured (relative L2 against the restatement / symmetry, MI355X):
two_blocks 1.04e-15 / 5.8e-16, graded_3 9.80e-16 / 3.8e-16, thin 1.11e-15 /
1.7e-16 (its J x against the oracle's 5.75e-16), graded_alpha 9.90e-16 / 1.8e-16;
the kept weight 1.01e-15, against 1.76e-05 for the restatement with omega0 from
T_b.  The approximate reciprocals of fdm2 do not show at 1e-15: each carries a
Newton step.

The Dirichlet tests found a defect, fixed with them (tv_mgsolve.cpp
dirichlet_masks): with the flag set the cycle masked its DG -> CG transfers with
a dinv that nothing writes on a DG1 context (all zero), so it collapsed to the
block smoother alone -- 4.1e-01 from the restatement, 1.2e-15 from
omega0 B^-1 r -- and two steps of `two_blocks` took (122, 128) Krylov iterations
instead of (23, 23).
"""
import functools

import numpy as np
import pytest

from dg_gmg_reference import GRIDS, DgBox, DgGmgCycle, params
from parity_util import relerr
from test_unstructured_dg import device_layout, host_layout

pytestmark = pytest.mark.gpu

DG = {"element": "DG", "degree": 1}
# id: (grid, dt, alpha (None: the default 1), mg_levels)
CYCLES = {
    "two_blocks": ("two_blocks", 0.1, None, 0),
    "graded_3": ("graded", 0.1, None, 3),
    "thin": ("thin", 0.1, None, 0),
    "graded_alpha": ("graded", 0.25, 0.37, 0),  # dt / (dt alpha) != 1 on the Robin term of the blocks
}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@functools.lru_cache(maxsize=None)
def box(grid, dt=0.1, alpha=None):
    """the T-independent reference side of a grid: assembled once, read only"""
    return DgBox(GRIDS[grid], dt, params(alpha))


def problem(grid, dt=0.1, alpha=None, mg_levels=0, mode="reference"):
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    return ThermoViscoProblem(RectilinearMesh(GRIDS[grid]), (0.0, 1.0), dt, {"T": DG, "sigma": DG}, params(alpha),
                              verbose=False, part_axis=2, preconditioner="gmg", mg_levels=mg_levels, model_mode=mode)


def set_T(p, T):
    p.set_field("T", T)
    p._flush()


def pcapply(torch, p, r):
    """tv_precond_apply on a cell-major vector"""
    rd = torch.tensor(device_layout(3, r), dtype=torch.float64, device="cuda")
    zd = torch.empty_like(rd)
    assert p._lib.tv_precond_apply(p._ctx, rd.data_ptr(), zd.data_ptr()) == 0, p._lib.tv_last_error(p._ctx)
    return host_layout(3, zd.cpu().numpy())


def random_T(n, seed=11):
    return 700.0 + np.random.default_rng(seed).uniform(0.0, 150.0, n)


def bitwise(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. the cycle against the restatement ------------------------------------------------------
@pytest.mark.parametrize("case", list(CYCLES))
def test_dg_cycle_matches_restatement(case):
    torch = _torch()
    grid, dt, alpha, levels = CYCLES[case]
    b = box(grid, dt, alpha)
    rng = np.random.default_rng(11)
    T = 700.0 + rng.uniform(0.0, 150.0, b.n)
    r, y = rng.standard_normal((2, b.n))
    p = problem(grid, dt, alpha, levels)
    try:
        p.setup()
        set_T(p, T)  # before the first apply: omega0 is estimated there, at this T
        if grid == "thin":  # the operator first: one cell along x, every x facet a Robin facet
            xd = torch.tensor(device_layout(3, y), dtype=torch.float64, device="cuda")
            wd = torch.empty_like(xd)
            assert p._lib.tv_jacobian_apply(p._ctx, xd.data_ptr(), wd.data_ptr()) == 0, p._lib.tv_last_error(p._ctx)
            eJ = relerr(host_layout(3, wd.cpu().numpy()), b.jacobian(T) @ y)
            print(f"[dg gmg] {case}: tv_jacobian_apply vs the oracle's J {eJ:.2e}")
            assert eJ < 1e-12, eJ
        z_r, z_y = pcapply(torch, p, r), pcapply(torch, p, y)
    finally:
        p.close()
    cyc = DgGmgCycle(b, T, mg_levels=levels)
    e = relerr(z_r, cyc.apply(r))
    e_block = relerr(z_r, cyc.smooth(r))
    sym = abs(y @ z_r - r @ z_y) / abs(y @ z_r)
    print(f"[dg gmg] cycle {case}: {cyc.cg_levels} CG levels, omega0 {cyc.omega0:.6f}, vs numpy {e:.2e} "
          f"(vs the block smoother alone {e_block:.1e}), symmetry {sym:.1e}, r.Br {r @ z_r:.3e}")
    assert e < 1e-10, e
    assert sym < 1e-12, sym
    assert r @ z_r > 0.0


# ---- 2. the weight is estimated once ----------------------------------------------------------
def test_dg_weight_is_kept_from_the_first_apply():
    """omega0 comes from the T of the first apply and stays; the blocks, J and the
    CG levels follow the T of each apply.  The restatement with omega0 from T_b
    must be far away (> 100 times the achieved error), or the case shows nothing."""
    torch = _torch()
    b = box("two_blocks")
    Ta = random_T(b.n)
    Tb = Ta + 40.0
    r = np.random.default_rng(3).standard_normal(b.n)
    p = problem("two_blocks")
    try:
        p.setup()
        set_T(p, Ta)
        z_a = pcapply(torch, p, r)
        set_T(p, Tb)
        z_b = pcapply(torch, p, r)
    finally:
        p.close()
    e_a = relerr(z_a, DgGmgCycle(b, Ta).apply(r))
    e_kept = relerr(z_b, DgGmgCycle(b, Tb, T_weight=Ta).apply(r))
    e_fresh = relerr(z_b, DgGmgCycle(b, Tb).apply(r))
    print(f"[dg gmg] kept weight: at T_a {e_a:.2e}; at T_b with omega0 from T_a {e_kept:.2e}, "
          f"with omega0 from T_b {e_fresh:.2e}")
    assert e_a < 1e-10, e_a
    assert e_kept < 1e-10, e_kept
    assert e_fresh > 100.0 * e_kept, (e_fresh, e_kept)


# ---- 3. Dirichlet mode has no effect on a DG1 temperature ------------------------------------
def test_dg_dirichlet_flag_leaves_the_cycle_alone():
    """No DG dof belongs to a facet: the constraint is empty, and the cycle must
    not mask its transfers (with a dinv nothing writes on a DG context the cycle
    would collapse to omega0 B^-1 r: still SPD, only the Krylov count shows it)."""
    torch = _torch()
    b = box("two_blocks")
    T = random_T(b.n)
    r = np.random.default_rng(3).standard_normal(b.n)
    p = problem("two_blocks", mode="paper")
    try:
        p.setup()
        set_T(p, T)
        z0 = pcapply(torch, p, r)
        assert p._lib.tv_set_dirichlet(p._ctx, 1, 600.0) == 0, p._lib.tv_last_error(p._ctx)
        z1 = pcapply(torch, p, r)
    finally:
        p.close()
    cyc = DgGmgCycle(b, T)
    print(f"[dg gmg] Dirichlet flag: before vs numpy {relerr(z0, cyc.apply(r)):.2e}, after {relerr(z1, cyc.apply(r)):.2e} "
          f"(after vs the block smoother alone {relerr(z1, cyc.smooth(r)):.1e})")
    assert relerr(z0, cyc.apply(r)) < 1e-10
    assert bitwise(z0, z1)


def test_dg_steps_with_dirichlet_flag_are_the_steps_without():
    _torch()
    out = []
    for flag in (False, True):
        p = problem("two_blocks", mode="paper")
        try:
            p.setup(dirichlet_bc=flag)
            its = []
            for _ in range(2):
                p.solve_timestep()
                its.append((p.last_newton_iterations, p.last_krylov_iterations))
            out.append((np.array(p.get_field("T")), its))
        finally:
            p.close()
    (T0, its0), (T1, its1) = out
    print(f"[dg gmg] two steps, (Newton, Krylov) per step: without the flag {its0}, with it {its1}")
    assert its0 == its1
    assert bitwise(T0, T1)


# ---- 4. determinism ---------------------------------------------------------------------------
def test_dg_cycle_is_deterministic():
    torch = _torch()
    b = box("two_blocks")
    T = random_T(b.n)
    r = np.random.default_rng(3).standard_normal(b.n)
    zs = []
    for _ in range(2):
        p = problem("two_blocks")
        try:
            p.setup()
            set_T(p, T)
            zs.append(pcapply(torch, p, r))
        finally:
            p.close()
    assert bitwise(zs[0], zs[1])
