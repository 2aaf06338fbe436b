"""The five Krylov solves (pcg_solve, pcg_solve_cgs, pcg_solve_mg and the two
forms of pcg_solve_mg_dist, all driven by krylov_drive) as ONE linear solve
each, against tests/krylov_reference.kspcg in long double on the oracle's
assembled J(T) and F(T, T_prev): the iterates, the counts and the end reasons.

One linear solve is isolated with solver.max_it = 1 (one Newton iteration,
error_on_nonconvergence off): solver.solve() returns (1, False),
last_krylov_iterations is that solve's count, the field "dx" its result, and
T_after == T_before - dx bitwise.  T and T_prev are set before every solve.

Reference preconditioners: r / diag J (Jacobi forms; get_field returns the
reference's dof order for DG too), gmg_reference.vcycle_reference at the
automatic depth (multigrid, CG1) and dg_gmg_reference.DgGmgCycle (multigrid,
DG1: "gmg-dg").  So the multigrid cases pin the cycle AS THE SOLVE
RUNS IT (mg_iteration: x0 = omega D^-1 r inside the PCG update launch, the
kernels gated on the device state, the sums from the reduction tails), not the
tv_precond_apply entry point.

Tolerances (relative L2 of dx against the long-double iterate): 1e-12 for the
Jacobi forms (the operator tolerance of test_gpu_parity: rounding only), 1e-11
for multigrid (the tolerance at which the V-cycle itself is pinned; 1e-10 for
the DG1 cycle, whose cell-block solve uses approximate reciprocals).  The
float64 run of the same reference is printed beside each result: it is the
rounding floor, <= 4e-16 on "plate" for all 27 Jacobi and all 5 multigrid
iterates.  Everything else is exact: counts, bitwise equalities, error strings.
"""
import functools
import os
import sys

import numpy as np
import pytest

import dg_gmg_reference as DGR
from gmg_reference import auto_levels, vcycle_reference
from krylov_reference import kspcg
from oracle import tv_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.1
KSP_DEFAULTS = dict(rtol=1e-5, atol=1e-50, divtol=1e5, max_it=10000)
GRIDS = {
    # tests/test_multigrid.CASES: three multigrid levels, several workgroups, partial tiles
    "plate": [np.linspace(0.0, 4.0, 33), np.linspace(0.0, 3.0, 25), np.linspace(0.0, 1.0, 9)],
    "graded": [np.concatenate([np.linspace(0.0, 0.5, 9), np.linspace(0.5, 2.5, 9)[1:]]),
               np.linspace(0.0, 2.0, 17), np.linspace(0.0, 0.75, 8)],
    # tests/test_gpu_parity.AXES
    "2d": [np.linspace(0.0, 3.0, 13), np.linspace(0.0, 1.0, 5)],
    "3d": [np.linspace(0.0, 2.0, 9), np.linspace(0.0, 2.0, 7), np.linspace(0.0, 1.0, 5)],
    # the DG1 box multigrid.  "dg": dg_gmg_reference.GRIDS["two_blocks"] (315 cells: two workgroups of cells,
    # the second partial).  "dg-graded": "graded" above at half its cell counts (8 x 8 x 3 cells; the
    # neighbours' lengths in the SIPG penalty) -- the oracle takes half a minute to assemble DG1 on "graded"
    # itself, and on dg_gmg_reference.GRIDS["graded"] the reference's dp_6 lies 5e-4 from the threshold
    # (a marginal count, which end_reason_sequence refuses); here the nearest is 5e-2
    "dg": DGR.GRIDS["two_blocks"],
    "dg-graded": [np.concatenate([np.linspace(0.0, 0.5, 5), np.linspace(0.5, 2.5, 5)[1:]]),
                  np.linspace(0.0, 2.0, 9), np.linspace(0.0, 0.75, 4)],
}
# id: (grid, family, mesh kind, reference B, constructor arguments, TVFEM_MG_RR, Krylov form the context must report)
FORMS = {
    "kspcg-plate": ("plate", "CG", "box", "jacobi", dict(pcg_variant="kspcg"), None, "kspcg"),
    "kspcg-graded": ("graded", "CG", "box", "jacobi", dict(pcg_variant="kspcg"), None, "kspcg"),
    "single-plate": ("plate", "CG", "box", "jacobi", dict(pcg_variant="single"), None, "single"),
    "single-graded": ("graded", "CG", "box", "jacobi", dict(pcg_variant="single"), None, "single"),
    "unfused-2d": ("2d", "CG", "box", "jacobi", dict(pcg_variant="kspcg"), None, "kspcg"),
    "unfused-3d-dg": ("3d", "DG", "box", "jacobi", dict(pcg_variant="kspcg"), None, "kspcg"),
    "unfused-3d-um": ("3d", "CG", "um", "jacobi", dict(pcg_variant="kspcg"), None, "kspcg"),
    "gmg-plate": ("plate", "CG", "box", "gmg", dict(preconditioner="gmg"), "0", "kspcg"),
    "gmg-plate-rr": ("plate", "CG", "box", "gmg", dict(preconditioner="gmg"), "1", "kspcg"),
    "gmg-graded": ("graded", "CG", "box", "gmg", dict(preconditioner="gmg"), "0", "kspcg"),
    # DG1 temperature: cell-block smoothing (k_dg_bupdate's init, first, odd and even forms), the CG1 box below
    "gmg-dg": ("dg", "DG", "box", "gmg-dg", dict(preconditioner="gmg"), None, "kspcg"),
    "gmg-dg-graded": ("dg-graded", "DG", "box", "gmg-dg", dict(preconditioner="gmg"), None, "kspcg"),
}
# gmg-dg: the bar at which tests/test_multigrid_dg.py pins the DG cycle itself
TOL = {"jacobi": 1e-12, "gmg": 1e-11, "gmg-dg": 1e-10}


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.sqrt(((a - b) @ (a - b)) / (b @ b)))


def bitwise(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def state(X):
    """the state of every case, at dof coordinates X (drawn in this order)"""
    rng = np.random.default_rng(0)
    T = 700.0 + 100.0 * np.cos(X[:, 0] / 3.0) + rng.uniform(-5, 5, X.shape[0])
    return T, T + rng.uniform(-3, 3, X.shape[0])


# ---- the reference side: assembled once per (grid, family), never modified -----
@functools.lru_cache(maxsize=None)
def system(grid, fam):
    sp = O.Space(O.rectilinear_mesh(GRIDS[grid]), fam, 1)
    form = O.HeatForm(sp, DT, O.ThermalParams.from_dict(O.MAIN_MODEL_PARAMS))
    X = sp.dof_coordinates()
    T, Tp = state(X)
    J = form.jacobian(T).tocsr()
    F = form.residual(T, Tp)
    centre = int(np.argmin(((X - 0.5 * (X.min(axis=0) + X.max(axis=0))) ** 2).sum(axis=1)))  # an interior dof
    for a in (T, Tp, F):
        a.setflags(write=False)
    return dict(form=form, T=T, Tp=Tp, J=J, F=F, centre=centre)


@functools.lru_cache(maxsize=None)
def precond(grid, fam, pc):
    s = system(grid, fam)
    if pc == "jacobi":
        d = s["J"].diagonal()
        return lambda r: r / d
    if pc == "gmg-dg":  # omega0 is estimated at the first solve's T: every solve here starts from s["T"]
        return DGR.DgGmgCycle(DGR.DgBox(GRIDS[grid], DT), s["T"])
    mp = dict(O.MAIN_MODEL_PARAMS)
    return vcycle_reference(GRIDS[grid], s["T"], mp, DT, auto_levels(GRIDS[grid], DT, mp["alpha"]))


@functools.lru_cache(maxsize=None)
def reference(grid, fam, pc):
    """the default-tolerance solve in long double (every iterate) and in float64"""
    s, B = system(grid, fam), precond(grid, fam, pc)
    return kspcg(s["J"], s["F"], B), kspcg(s["J"], s["F"], B, dtype=np.float64)


def ref_solve(form_id, **tol):
    grid, fam, _, pc = FORMS[form_id][:4]
    s = system(grid, fam)
    if "divtol" in tol:
        tol["dtol"] = tol.pop("divtol")
    return kspcg(s["J"], s["F"], precond(grid, fam, pc), **tol)


# ---- the device side ----------------------------------------------------------
def device(form_id, monkeypatch, **kw):
    from tvfem import RectilinearMesh, UnstructuredMesh
    from tvfem.problem import ThermoViscoProblem
    grid, fam, kind, _, args, rr, _ = FORMS[form_id]
    if rr is not None:
        monkeypatch.setenv("TVFEM_MG_RR", rr)
    axes = GRIDS[grid]
    mesh = RectilinearMesh(axes)
    if kind == "um":
        mesh = UnstructuredMesh.from_rectilinear(mesh)
    el = {"element": fam, "degree": 1}
    p = ThermoViscoProblem(mesh, (0.0, 1.0), DT, {"T": el, "sigma": el}, dict(O.MAIN_MODEL_PARAMS), verbose=False,
                           part_axis=2 if len(axes) == 3 else -1, **args, **kw)
    p.setup()
    one_linear_solve(p)
    return p


def one_linear_solve(p):
    p.solver.max_it = 1
    p.solver.error_on_nonconvergence = False


def solve(p, T, Tp):
    """one linear solve from (T, T_prev): (count, dx, T after)"""
    p.set_field("T", T)
    p.set_field("T_prev", Tp)
    p._flush()
    assert p.solver.solve() == (1, False)
    dx, T1 = p.get_field("dx"), p.get_field("T")
    assert bitwise(T1, T - dx), "T_after != T_before - dx"
    return p.last_krylov_iterations, dx, T1


def failing_solve(p, T, Tp, reason):
    """a solve that must end with `reason`: TV_ERR_KSP, and T bitwise as set"""
    from tvfem import _native as N
    p.set_field("T", T)
    p.set_field("T_prev", Tp)
    p._flush()
    with pytest.raises(N.NativeError, match=reason) as e:
        p.solver.solve()
    assert e.value.code == N.TV_ERR_KSP, e.value.code
    assert bitwise(p.get_field("T"), T), f"T changed by a solve that ended with {reason}"
    assert bitwise(p.get_field("T_prev"), Tp)


# ---- (a) the iterates ----------------------------------------------------------
@pytest.mark.parametrize("form_id", list(FORMS))
def test_iterates_match_reference(form_id, monkeypatch):
    """ksp_fixed_its = j for j in {1, 2, k_ref}: the solve ends at iteration j
    as DIVERGED_ITS, which accept_its makes a good outcome, and dx is the
    reference's iterate x_j."""
    _gpu()
    grid, fam, _, pc, _, _, variant = FORMS[form_id]
    s = system(grid, fam)
    ref, ref64 = reference(grid, fam, pc)
    assert ref.reason == "CONVERGED_RTOL" and ref.its >= 3
    worst = []
    for j in (1, 2, ref.its):
        p = device(form_id, monkeypatch, ksp_fixed_its=j)
        try:
            k, dx, _ = solve(p, s["T"], s["Tp"])
            assert p.pcg_variant == variant
        finally:
            p.close()
        e, floor = relerr(dx, ref.x[j]), relerr(ref64.x[j], ref.x[j])
        print(f"[krylov] {form_id}: iterate {j} of {ref.its}: device vs long double {e:.2e} "
              f"(float64 reference vs long double {floor:.1e})")
        assert k == j, (j, k)
        worst.append((e, j))
    assert max(worst)[0] < TOL[pc], worst


# ---- (b), (c) the end reasons, on one context ------------------------------------
def end_reason_sequence(p, T, Tp, nan_at, ref=None, tol=None, steps=range(1, 10), tag=""):
    """ref: the reference solve of form `ref` (None: the exact properties only,
    k from step 1 of this context)."""
    ksp = p.ksp
    out = {}
    assert ksp.getTolerances() == tuple(KSP_DEFAULTS.values())

    def check(dx, x_ref, step):
        if x_ref is not None:
            e = relerr(dx, x_ref)
            print(f"[krylov] {tag} step {step}: dx vs long double {e:.2e}")
            assert e < tol, (step, e)

    full = None if ref is None else ref_solve(ref)
    if full is not None:
        # no case may be marginal: every dp_j well away from the threshold
        ttol = max(1e-5 * full.dp[0], 1e-50)
        margin = min(abs(float(dp / ttol) - 1.0) for dp in full.dp)
        print(f"[krylov] {tag}: reference k = {full.its}, nearest dp_j / ttol - 1 = {margin:.2e}")
        assert margin >= 1e-3, margin
    # 1. default tolerances
    k, dx1, _ = solve(p, T, Tp)
    if full is not None:
        assert k == full.its, (k, full.its)
        check(dx1, full.x[k], 1)
    assert k >= 4, k
    out["k"] = k
    if 2 in steps:
        # 2. atol between dp_m and dp_{m-1}: ends at m < k (the hint queued k launches)
        m = k // 2
        atol = float(np.sqrt(full.dp[m] * full.dp[m - 1]))
        at = ref_solve(ref, atol=atol)
        assert (at.its, at.reason) == (m, "CONVERGED_ATOL")
        assert min(abs(float(dp) / atol - 1.0) for dp in at.dp) >= 1e-3
        ksp.setTolerances(atol=atol)
        km, dxm, _ = solve(p, T, Tp)
        assert km == m, (km, m)
        check(dxm, at.x[m], 2)
        ksp.setTolerances(**KSP_DEFAULTS)
    # 3. defaults again (after step 2 the hint is m < k: the follow-up batches run)
    k3, dx3, _ = solve(p, T, Tp)
    assert k3 == k and bitwise(dx3, dx1), (3, k3)
    # 4. max_it = k: converged AT max_it
    ksp.setTolerances(max_it=k)
    k4, dx4, _ = solve(p, T, Tp)
    assert k4 == k and bitwise(dx4, dx1), (4, k4)
    # 5. max_it = k - 1
    ksp.setTolerances(max_it=k - 1)
    if full is not None:
        r5 = ref_solve(ref, max_it=k - 1)
        assert (r5.its, r5.reason) == (k - 1, "DIVERGED_ITS")
    failing_solve(p, T, Tp, "DIVERGED_ITS")
    ksp.setTolerances(**KSP_DEFAULTS)
    if 6 in steps:
        # 6. divtol below dp_1 / dp_0
        divtol = 0.5 * float(full.dp[1] / full.dp[0])
        assert divtol > 10 * 1e-5  # far above rtol: iteration 1 does not converge
        r6 = ref_solve(ref, divtol=divtol)
        assert (r6.its, r6.reason) == (1, "DIVERGED_DTOL")
        ksp.setTolerances(divtol=divtol)
        failing_solve(p, T, Tp, "DIVERGED_DTOL")
        ksp.setTolerances(**KSP_DEFAULTS)
    # 7. atol = 1e300: converged before the first iteration
    ksp.setTolerances(atol=1e300)
    k7, dx7, T7 = solve(p, T, Tp)
    assert k7 == 0 and not dx7.any() and bitwise(T7, T), (7, k7)
    ksp.setTolerances(**KSP_DEFAULTS)
    # 8. one NaN in T: the reference's own end reason, at iteration 0
    Tn = T.copy()
    Tn[nan_at] = np.nan
    if full is not None:
        grid, fam, _, pc = FORMS[ref][:4]
        s = system(grid, fam)
        Fn = s["form"].residual(Tn, Tp)
        assert not np.isfinite(Fn).all()
        # (the reason is decided on dp_0 = ||B F||: J(T) need not be assembled again)
        r8 = kspcg(s["J"], Fn, precond(grid, fam, pc))
        assert (r8.its, r8.reason) == (0, "DIVERGED_NANORINF")
    failing_solve(p, Tn, Tp, "DIVERGED_NANORINF")
    # 9. defaults, T reset: the context survived three failed solves
    k9, dx9, _ = solve(p, T, Tp)
    assert k9 == k and bitwise(dx9, dx1), (9, k9)
    return out


@pytest.mark.parametrize("form_id", list(FORMS))
def test_end_reasons_on_one_context(form_id, monkeypatch):
    """Steps 1-9 on ONE context (each solve starts from the hint the previous one
    left): rtol at k; atol at m = k // 2 with k launches queued; k again from the
    hint m; converged at max_it = k; DIVERGED_ITS at max_it = k - 1;
    DIVERGED_DTOL at iteration 1; atol = 1e300 (0 iterations, dx = 0);
    DIVERGED_NANORINF from one NaN in T; then the first result again, bitwise.
    Every failed solve leaves T bitwise as it was set."""
    _gpu()
    grid, fam, _, pc, _, _, variant = FORMS[form_id]
    s = system(grid, fam)
    p = device(form_id, monkeypatch)
    try:
        end_reason_sequence(p, s["T"], s["Tp"], s["centre"], ref=form_id, tol=TOL[pc], tag=form_id)
        assert p.pcg_variant == variant
    finally:
        p.close()


@pytest.mark.parametrize("case,variant", [("box_gmg_distributed", "kspcg"), ("box_gmg_single_reduction", "single")])
def test_end_reasons_distributed_forms(case, variant):
    """The two forms of pcg_solve_mg_dist, on the host-staged one-rank transport
    (tools/loopback_check: the middle slab of three receives its own periodic
    images).  That slab solves a periodic image problem which the oracle does
    not assemble, so there is NO independent reference here: steps 1, 3, 4, 5,
    7, 8 and 9 with k taken from step 1 of the same context -- exact
    properties only (counts, bitwise equalities, error strings).  The
    world-2 / world-3 tests of tests/test_partition.py stay the parity check
    of these forms."""
    _gpu()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loopback_check as L
    p = L._problem(*L.CASES[case])
    try:
        L._host_loopback(p)
        p.setup()
        one_linear_solve(p)
        X = p.functionSpaces["T"].tabulate_dof_coordinates()
        T, Tp = state(X)
        nan_at = int(np.argmin(((X - 0.5 * (X.min(axis=0) + X.max(axis=0))) ** 2).sum(axis=1)))
        out = end_reason_sequence(p, T, Tp, nan_at, steps=(1, 3, 4, 5, 7, 8, 9), tag=case)
        print(f"[krylov] {case}: form {p.pcg_variant}, k = {out['k']}")
        assert p.pcg_variant == variant
    finally:
        p.close()
