"""Out-of-bounds accesses of the kernels, seen through red zones (tests/guard_util.py).

GPU AddressSanitizer is not available where this project runs, every device
vector is a page-rounded allocation of its own and the tests hand the kernels
fresh, well-aligned torch tensors: a read or a write a few bytes outside a
vector lands in mapped slack and shows nowhere.  Every case here runs the same
call sequence twice -- in a context created with TVFEM_ALLOC_GUARD (every
allocation of the library between two guards filled with NaN bit patterns, or
zeros around index arrays) and with the caller's vectors inside NaN-filled
arenas, then in a plain context with fresh tensors -- and asserts

  (a) outputs and state fields are bitwise equal between the two runs: the
      kernels are deterministic and the runs differ only in addresses and in
      what lies outside the vectors, so a difference is an out-of-bounds read;
  (b) every guard, the library's and the caller arenas', still holds its fill
      (no out-of-bounds write), and the mode was really on (n_guarded > 0);
  (c) the guarded result agrees with the oracle the existing suite uses for the
      call, at that suite's tolerance (J x, F, diag 1e-12; V-cycle 1e-11).

Not seen: accesses further out than the 64 KiB guards (they exceed a fine node
plane of every grid here, so a miss by a row or a plane still lands inside),
over-reads of index arrays (their guards hold zeros so that a masked over-read
stays a valid index), LDS, memory that torch or RCCL allocate.

Grids and builders are those of the existing tests (imported, not copied).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from guard_util import assert_guards_intact, guard_check, guard_env, guarded, plain_env
from oracle import tv_oracle as O
from parity_util import relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CG = {"element": "CG", "degree": 1}
DG = {"element": "DG", "degree": 1}
MP = dict(O.MAIN_MODEL_PARAMS)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Run:
    """One of the two runs of a case: vectors and the end-of-run checks."""

    def __init__(self, monkeypatch, on):
        self.on = on
        self.checks = []
        (guard_env if on else plain_env)(monkeypatch)

    def vec(self, values, lead=0):
        """(tensor, device pointer) holding `values`: inside a NaN arena, or a fresh tensor"""
        import torch
        if self.on:
            view, ptr, check = guarded(values, lead)
            self.checks.append(check)
            return view, ptr
        t = torch.tensor(np.asarray(values, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda")
        return t, t.data_ptr()

    def finish(self, lib):
        """(b), while the contexts of the run are still live"""
        if self.on:
            assert_guards_intact(lib)
            for check in self.checks:
                check()
        else:
            assert guard_check(lib)[0] == 0  # the plain run is plain


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return np.array_equal(a, b)


def _twice(monkeypatch, fn):
    """fn(run) -> {name: array}, once guarded and once plain; (a); returns the guarded result"""
    got = fn(Run(monkeypatch, True))
    plain = fn(Run(monkeypatch, False))
    plain_env(monkeypatch)
    assert got.keys() == plain.keys()
    for k in got:
        if not _same_bits(got[k], plain[k]):
            g, p = np.asarray(got[k], dtype=float).ravel(), np.asarray(plain[k], dtype=float).ravel()
            raise AssertionError(f"(a) {k}: guarded and plain run differ in {int((g != p).sum())} of {g.size} values "
                                 f"({int(np.isnan(g).sum())} NaN guarded, {int(np.isnan(p).sum())} NaN plain): "
                                 "an out-of-bounds read")
    return got


def _fields(p, names):
    out = {}
    for f in names:
        out[f] = p.get_field(f)
    return out


STATE = ("T", "Tf", "phi", "xi", "sigma")


# ---- F, J x, diag J on caller vectors ---------------------------------------------------------
from test_gpu_parity import AXES, EDGE_GRIDS, PCG_GRIDS, device_layout, host_layout  # noqa: E402


@functools.lru_cache(maxsize=None)
def _operator_oracle(grid, fam):
    """T, T_prev, x and F(T), J(T) x, diag J(T) of the oracle, in its own dof order, once per grid"""
    axes = (EDGE_GRIDS if grid in EDGE_GRIDS else AXES)[grid]
    cfg = {"T": {"element": fam, "degree": 1}, "sigma": {"element": fam, "degree": 1}}
    ref = O.OracleProblem(O.rectilinear_mesh(axes), (0.0, 1.0), 0.1, cfg, MP, linear="pcg")
    ref.setup()
    rng = np.random.default_rng(11)
    n = ref.VT.n
    X = np.zeros((n, 3))
    X[:, :len(axes)] = ref.VT.dof_coordinates()
    T = 700.0 + 100.0 * np.cos(X[:, 0] / 3.0) + rng.uniform(-5, 5, n)
    Tp = T + rng.uniform(-3, 3, n)
    x = rng.standard_normal(n)
    J = ref.form.jacobian(T)
    return X, T, Tp, x, ref.form.residual(T, Tp), J @ x, J.diagonal()


def _operators(monkeypatch, grid, fam, lead, part_axis=None):
    _torch()
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = (EDGE_GRIDS if grid in EDGE_GRIDS else AXES)[grid]
    Xr, T, Tp, x, F_ref, Jx_ref, d_ref = _operator_oracle(grid, fam)
    cfg = {"T": {"element": fam, "degree": 1}, "sigma": {"element": fam, "degree": 1}}
    if part_axis is None:
        part_axis = 2 if len(axes) == 3 else -1
    order = {}

    def run(R):
        dev = ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, cfg, MP, part_axis=part_axis, verbose=False)
        dev.setup()
        # the device's dof order against the oracle's (the storage permutation of part_axis 1); DG: cell-major
        # host layout on both sides, the same cell order for the part_axis used there
        if fam == "CG":
            Xd = dev.functionSpaces["T"].tabulate_dof_coordinates()
            od, orr = np.lexsort(Xd.T[::-1]), np.lexsort(Xr.T[::-1])
            assert np.allclose(Xd[od], Xr[orr])
            to_dev = np.empty(len(od), dtype=np.int64)
            to_dev[od] = orr  # device dof i holds oracle dof to_dev[i]
        else:
            to_dev = np.arange(T.size)
        order["to_dev"] = to_dev
        dev.set_field("T", T[to_dev])
        dev.set_field("T_prev", Tp[to_dev])
        lib, ctx = dev._lib, dev._ctx
        n = T.size
        _, Td = R.vec(device_layout(dev, T[to_dev], fam), lead)
        Fv, Fd = R.vec(np.zeros(n), lead)
        assert lib.tv_residual(ctx, Td, Fd) == 0, lib.tv_last_error(ctx)
        _, xd = R.vec(device_layout(dev, x[to_dev], fam), lead)
        yv, yd = R.vec(np.zeros(n), lead)
        assert lib.tv_jacobian_apply(ctx, xd, yd) == 0, lib.tv_last_error(ctx)
        dv, dd = R.vec(np.zeros(n), lead)
        assert lib.tv_jacobian_diag(ctx, dd) == 0, lib.tv_last_error(ctx)
        out = {"F": host_layout(dev, Fv.cpu().numpy(), fam), "Jx": host_layout(dev, yv.cpu().numpy(), fam),
               "diag": host_layout(dev, dv.cpu().numpy(), fam)}
        R.finish(lib)
        dev.close()
        return out

    got = _twice(monkeypatch, run)
    to_dev = order["to_dev"]
    for name, want in (("F", F_ref), ("Jx", Jx_ref), ("diag", d_ref)):
        e = relerr(got[name], want[to_dev])
        print(f"[guard] {grid} {fam} lead {lead} part_axis {part_axis}: {name} vs oracle {e:.2e}")
        assert e < 1e-12, (name, e)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("grid,part_axis", [("x71_y1cell", 2), ("z1cell", 2), ("chunks", 2), ("chunks", 1)])
def test_cg_march_operators(grid, part_axis, lead, monkeypatch):
    """k_cg_march and its boundary passes (tv_cg.hip) on the edge grids, both storage orders, caller
    vectors guarded, 16-byte aligned (lead 0) and only 8-byte aligned (lead 1)"""
    _operators(monkeypatch, grid, "CG", lead, part_axis)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("fam", ["CG", "DG"])
@pytest.mark.parametrize("grid", ["1d_graded", "2d"])
def test_operators_1d_2d(grid, fam, lead, monkeypatch):
    _operators(monkeypatch, grid, fam, lead)


# ---- DG1 tile and cell kernels ----------------------------------------------------------------
def test_dg_kernels(monkeypatch):
    """The 65 x 14 x 8 grid of test_dg_tile_kernel_matches_cell_kernel: J x on guarded caller vectors
    and one coupled step, cell kernel and tile kernel (chunk 2).  (c): the tile kernel against the
    cell kernel, as that test (the oracle is too slow to assemble DG1 at this size)."""
    _torch()
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = [np.linspace(0.0, 6.4, 65), np.concatenate([np.linspace(0.0, 0.4, 5), np.linspace(0.4, 1.3, 10)[1:]]),
            np.linspace(0.0, 0.7, 8)]
    res = {}
    for kern, chunk in (("cells", 0), ("tile", 2)):
        def run(R):
            p = ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, {"T": DG, "sigma": DG}, MP, part_axis=2,
                                   materialize=False, verbose=False, dg_kernel=kern, dg_tile_chunk=chunk)
            p.setup()
            p.solve_timestep()
            out = _fields(p, STATE)
            n = out["T"].size
            r = np.random.default_rng(3)
            T = 700.0 + r.uniform(0.0, 150.0, n)
            x = r.standard_normal(n)
            p.set_field("T", T)
            p._flush()
            _, xd = R.vec(device_layout(p, x, "DG"))
            yv, yd = R.vec(np.zeros(n))
            assert p._lib.tv_jacobian_apply(p._ctx, xd, yd) == 0, p._lib.tv_last_error(p._ctx)
            out["Jx"] = host_layout(p, yv.cpu().numpy(), "DG")
            R.finish(p._lib)
            p.close()
            return out
        res[kern] = _twice(monkeypatch, run)
    assert relerr(res["tile"]["Jx"], res["cells"]["Jx"]) < 1e-12
    assert relerr(res["tile"]["T"], res["cells"]["T"]) < 1e-10


# ---- the V-cycle ------------------------------------------------------------------------------
from gmg_reference import auto_levels, vcycle_reference  # noqa: E402
from test_multigrid import CASES, VCYCLE_CASES  # noqa: E402


@functools.lru_cache(maxsize=None)
def _vcycle_oracle(case):
    axes, levels = VCYCLE_CASES[case]
    n = int(np.prod([len(a) for a in axes]))
    rng = np.random.default_rng(11)
    T = 700.0 + rng.uniform(0.0, 150.0, n)
    r = rng.standard_normal(n)
    y = rng.standard_normal(n)
    nlev = levels if levels else auto_levels(axes, 0.1, MP["alpha"])
    return T, r, y, vcycle_reference(axes, T, MP, 0.1, nlev)(r)


@pytest.mark.parametrize("rr", [0, 1], ids=["jx_restrict", "fused_restrict"])
@pytest.mark.parametrize("case", list(VCYCLE_CASES))
def test_vcycle(case, rr, monkeypatch):
    """tv_precond_apply (tv_mg.hip) with r and z guarded, level 0's restriction after J x (k_mg_restrict_pairs)
    and fused (k_mg_rrestrict: its x lanes hold fine pairs and the row's last node has no partner, so the pair
    of the last row of the last plane used to end one double past x, b and the face arrays, kept harmless
    only by the hardware's range check of the buffer load; the value meets a weight 0, and 0 x NaN would poison
    b_1 and with it all of z).  Symmetry and (c) against the numpy V-cycle, 1e-11."""
    _torch()
    monkeypatch.setenv("TVFEM_MG_RR", str(rr))
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes, levels = VCYCLE_CASES[case]
    T, r, y, Br = _vcycle_oracle(case)

    def run(R):
        p = ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, {"T": CG, "sigma": CG}, MP, verbose=False,
                               part_axis=2, preconditioner="gmg", mg_levels=levels)
        p.setup()
        p.set_field("T", T)
        p._flush()
        out = {}
        for name, v, lead in (("z_r", r, 0), ("z_y", y, 1)):
            _, vd = R.vec(v, lead)
            zv, zd = R.vec(np.zeros(v.size), lead)
            assert p._lib.tv_precond_apply(p._ctx, vd, zd) == 0, p._lib.tv_last_error(p._ctx)
            out[name] = zv.cpu().numpy()
        R.finish(p._lib)
        p.close()
        return out

    got = _twice(monkeypatch, run)
    e = relerr(got["z_r"], Br)
    sym = abs(y @ got["z_r"] - r @ got["z_y"]) / abs(y @ got["z_r"])
    print(f"[guard] V-cycle {case} TVFEM_MG_RR={rr}: vs numpy {e:.2e}, symmetry {sym:.1e}")
    assert e < 1e-11, e
    assert sym < 1e-12, sym
    assert r @ got["z_r"] > 0.0


def test_dg_multigrid(monkeypatch):
    """The DG1 -> CG1 multigrid on the 13 x 11 x 6 grid of test_gmg_dg_steps_match_oracle: tv_precond_apply on
    guarded vectors and one step.  (c): T of the step against the oracle at that test's 1e-10."""
    _torch()
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = [np.linspace(0.0, 3.0, 13), np.linspace(0.0, 2.5, 11), np.linspace(0.0, 1.0, 6)]
    cfg = {"T": DG, "sigma": DG}

    def run(R):
        p = ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, cfg, MP, verbose=False, part_axis=2,
                               preconditioner="gmg")
        p.setup()
        p.solve_timestep()
        out = _fields(p, STATE)
        n = out["T"].size
        r = np.random.default_rng(5).standard_normal(n)
        _, rd = R.vec(r)
        zv, zd = R.vec(np.zeros(n))
        assert p._lib.tv_precond_apply(p._ctx, rd, zd) == 0, p._lib.tv_last_error(p._ctx)
        out["z"] = zv.cpu().numpy()
        R.finish(p._lib)
        p.close()
        return out

    got = _twice(monkeypatch, run)
    ref = O.OracleProblem(O.rectilinear_mesh(axes), (0.0, 1.0), 0.1, cfg, MP, linear="pcg")
    ref.setup()
    ref.solve_timestep()
    assert relerr(got["T"], ref.functions_current["T"]) < 1e-10
    assert np.isfinite(got["z"]).all()


# ---- whole steps: the Krylov loop, fused matvec, updates, reductions -------------------------------
def _steps(monkeypatch, mk, steps, setup_kw=None):
    def run(R):
        p = mk()
        p.setup(**(setup_kw or {}))
        for _ in range(steps):
            p.solve_timestep()
        out = _fields(p, STATE)
        out["its"] = np.array([p.last_newton_iterations, p.last_krylov_iterations])
        R.finish(p._lib)
        p.close()
        return out
    return _twice(monkeypatch, run)


@functools.lru_cache(maxsize=None)
def _step_oracle(key, steps, mode="reference", dirichlet=False):
    axes = {"graded": PCG_GRIDS["graded"], "plate": CASES["plate"],
            "dirichlet": [np.linspace(0.0, 2.0, 17), np.linspace(0.0, 2.0, 17), np.linspace(0.0, 1.0, 9)]}[key]
    ref = O.OracleProblem(O.rectilinear_mesh(axes), (0.0, 1.0), 0.1, {"T": CG, "sigma": CG}, MP, linear="pcg",
                          model_mode=mode)
    ref.setup(dirichlet_bc=True) if dirichlet else ref.setup()
    for _ in range(steps):
        ref.solve_timestep()
    return ref.functions_current["T"].copy()


@pytest.mark.parametrize("variant", ["kspcg", "single"])
def test_krylov_jacobi_steps(variant, monkeypatch):
    """tv_pcg.hip / tv_solver.cpp on PCG_GRIDS["graded"], both Krylov forms, two steps; (c): T 1e-10"""
    _torch()
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = PCG_GRIDS["graded"]
    got = _steps(monkeypatch, lambda: ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, {"T": CG, "sigma": CG},
                                                         MP, part_axis=2, materialize=False, verbose=False,
                                                         pcg_variant=variant), 2)
    assert relerr(got["T"], _step_oracle("graded", 2)) < 1e-10


@pytest.mark.parametrize("rr", [0, 1], ids=["jx_restrict", "fused_restrict"])
def test_krylov_gmg_steps(rr, monkeypatch):
    """CASES["plate"] with the multigrid preconditioner, both level-0 restrictions, two steps; (c): T 1e-10"""
    _torch()
    monkeypatch.setenv("TVFEM_MG_RR", str(rr))
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = CASES["plate"]
    got = _steps(monkeypatch, lambda: ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, {"T": CG, "sigma": CG},
                                                         MP, part_axis=2, verbose=False, preconditioner="gmg"), 2)
    assert relerr(got["T"], _step_oracle("plate", 2)) < 1e-10


def test_dirichlet_step(monkeypatch):
    """The Dirichlet masks on the 17 x 17 x 9 paper-mode grid of test_gmg_dirichlet_matches_oracle, one step"""
    _torch()
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    axes = [np.linspace(0.0, 2.0, 17), np.linspace(0.0, 2.0, 17), np.linspace(0.0, 1.0, 9)]
    got = _steps(monkeypatch, lambda: ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, {"T": CG, "sigma": CG},
                                                         MP, part_axis=2, verbose=False, preconditioner="gmg",
                                                         model_mode="paper"), 1, dict(dirichlet_bc=True))
    assert relerr(got["T"], _step_oracle("dirichlet", 1, "paper", True)) < 1e-10


# ---- the visco update -------------------------------------------------------------------------
@pytest.mark.parametrize("materialize", [True, False], ids=["materialized", "lean"])
@pytest.mark.parametrize("dim", [1, 3])
def test_visco_update(dim, materialize, monkeypatch):
    """tv_visco.hip at the random state of test_visco_pointwise_random_state; every readable field bitwise.
    (c): the scalar fields against the oracle's update at that test's 1e-12 (materialized, where it reads them)."""
    _torch()
    from tvfem import RectilinearMesh
    from tvfem._native import FIELDS, NativeError
    from tvfem.problem import ThermoViscoProblem
    axes = AXES["1d_uniform"] if dim == 1 else AXES["3d"]
    cfg = {"T": CG, "sigma": CG}
    n = int(np.prod([len(a) for a in axes]))
    rng = np.random.default_rng(1)
    T = rng.uniform(760.0, 900.0, n)
    Tp = T + rng.uniform(-2.0, 2.0, n)
    Tfp = np.repeat(T, 6) + rng.uniform(-1, 1, 6 * n)
    st = rng.standard_normal(n * 6 * dim * dim) * 1e-3
    sg = rng.standard_normal(n * 6 * dim * dim) * 1e-3
    state = (("T", T), ("T_prev", Tp), ("Tf_partial", Tfp), ("s_tilde_partial", st), ("sigma_tilde_partial", sg))

    def run(R):
        dev = ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, cfg, MP, part_axis=2 if dim == 3 else -1,
                                 materialize=materialize, verbose=False)
        dev.setup()
        for fld, v in state:
            dev.set_field(fld, v)
        assert dev._lib.tv_visco_update(dev._ctx) == 0
        dev._device_version += 1
        out = {}
        for f in FIELDS:
            try:
                out[f] = dev.get_field(f)
            except NativeError:  # not materialised in the lean layout
                pass
        R.finish(dev._lib)
        dev.close()
        return out

    got = _twice(monkeypatch, run)
    assert {"T", "Tf", "phi", "xi", "sigma"} <= got.keys()
    ref = O.OracleProblem(O.rectilinear_mesh(axes), (0.0, 1.0), 0.1, cfg, MP, linear="pcg")
    ref.setup()
    ref.functions_current["T"][:] = T
    ref.functions_previous["T"][:] = Tp
    ref.functions_current["Tf_partial"][:] = Tfp
    ref.functions_previous["Tf_partial"][:] = Tfp
    ref.functions_current["s_tilde_partial"][:] = st
    ref.functions_current["sigma_tilde_partial"][:] = sg
    ref.visco_update()
    for k, v in (("phi", ref.functions["phi"]), ("xi", ref.functions["xi"]), ("Tf", ref.functions_current["Tf"])):
        assert relerr(got[k], v) < 1e-12, k
    assert relerr(got["sigma"], ref.functions_next["sigma"]) < 1e-9


# ---- unstructured meshes and the algebraic multigrid ------------------------------------------
def test_unstructured_operators(monkeypatch):
    """tv_um.hip on the smallest mesh of test_unstructured_operators_match_oracle ("quad"): F, J x, diag J on
    guarded caller vectors (lead 1) and one step; (c): 1e-12 against the oracle"""
    _torch()
    from test_unstructured import make_pair
    m, dev0, ref = make_pair("quad")
    dev0.close()
    ref.setup()
    rng = np.random.default_rng(0)
    n = ref.VT.n
    X = ref.VT.dof_coordinates()
    T = 700.0 + 100.0 * np.cos(X[:, 0] / 0.7) + rng.uniform(-5, 5, n)
    Tp = T + rng.uniform(-3, 3, n)
    x = rng.standard_normal(n)

    def run(R):
        _, dev, _ = make_pair("quad")
        dev.setup()
        dev.solve_timestep()
        out = _fields(dev, STATE)
        dev.set_field("T", T)
        dev.set_field("T_prev", Tp)
        lib, ctx = dev._lib, dev._ctx
        _, Td = R.vec(T, 1)
        Fv, Fd = R.vec(np.zeros(n), 1)
        assert lib.tv_residual(ctx, Td, Fd) == 0
        _, xd = R.vec(x, 1)
        yv, yd = R.vec(np.zeros(n), 1)
        assert lib.tv_jacobian_apply(ctx, xd, yd) == 0
        dv, dd = R.vec(np.zeros(n), 1)
        assert lib.tv_jacobian_diag(ctx, dd) == 0
        out.update(F=Fv.cpu().numpy(), Jx=yv.cpu().numpy(), diag=dv.cpu().numpy())
        R.finish(lib)
        dev.close()
        return out

    got = _twice(monkeypatch, run)
    J = ref.form.jacobian(T)
    assert relerr(got["F"], ref.form.residual(T, Tp)) < 1e-12
    assert relerr(got["Jx"], J @ x) < 1e-12
    assert relerr(got["diag"], J.diagonal()) < 1e-12


def test_amg_vcycle_and_step(monkeypatch):
    """tv_amg*. on the smallest mesh of test_amg_vcycle_matches_restatement ("two_levels"): tv_precond_apply on
    guarded vectors and one step; (c): against the restated hierarchy at that test's 1e-10"""
    _torch()
    from oracle import amg as OA
    from test_amg import VCYCLE_CASES as AMG_CASES, _mesh, _omesh
    from tvfem.problem import ThermoViscoProblem
    nc, L = AMG_CASES["two_levels"]
    m = _mesh(nc, L, seed=2, shuffle=True)
    nv = m.num_vertices
    rng = np.random.default_rng(5)
    T = 700.0 + rng.uniform(0.0, 150.0, nv)
    r = rng.standard_normal(nv)

    def run(R):
        p = ThermoViscoProblem(m, (0.0, 1.0), 0.1, {"T": CG, "sigma": CG}, MP, verbose=False, preconditioner="amg")
        p.setup()
        T0 = p.get_field("T")
        p.set_field("T", T)
        p._flush()
        _, rd = R.vec(r, 1)
        zv, zd = R.vec(np.zeros(nv), 1)
        # (first: the smoother weight is estimated once, at the T of the first application)
        assert p._lib.tv_precond_apply(p._ctx, rd, zd) == 0, p._lib.tv_last_error(p._ctx)
        out = {"z": zv.cpu().numpy()}
        p.set_field("T", T0)
        p._flush()
        p.solve_timestep()
        out.update(_fields(p, STATE))
        R.finish(p._lib)
        p.close()
        return out

    got = _twice(monkeypatch, run)
    om = _omesh(m)
    V = O.HeatForm(O.Space(om, "CG"), 0.1, O.ThermalParams.from_dict({**MP, "epsilon": 0.0, "htc": 0.0})).jacobian(T)
    J = O.HeatForm(O.Space(om, "CG"), 0.1, O.ThermalParams.from_dict(MP)).jacobian(T)
    levels = OA.build(V, dims=None)
    d0 = 1.0 / J.diagonal()
    om0 = 2.0 / (1.1 * OA.lam_max_device(J, d0))
    assert relerr(got["z"], OA.apply(levels, r, d0, om0)) < 1e-10


# ---- slab partitions over the host transport --------------------------------------------------
def _part_run(world, port, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "guard_part_check.py"),
           *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("GUARD_PART_CHECK ")]
    assert line, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(line[0].split(" ", 1)[1])


@pytest.mark.parametrize("name,extra", [("cg_gmg", ("--pc", "gmg", "--pcg", "kspcg")),
                                        ("dg", ("--family", "DG", "--pcg", "kspcg"))])
def test_partitioned_step(name, extra):
    """Two slabs on one GPU over the host transport (tests/guard_part_check.py, the smallest world-2 CG + GMG
    and DG cases of tests/test_partition.py: the 10 x 30 x 5 box): one step guarded, then plain, in the same
    processes; ghost planes and send buffers are guarded allocations.  (c): T against the single partition at
    that file's 1e-12."""
    _torch()
    g = _part_run(2, 29900 + (7 if name == "dg" else 0), extra)
    print("[guard] partitioned", name, json.dumps(g))
    for rank in range(2):
        assert g["n_guarded"][rank] > 0 and g["guard_bytes"][rank] >= 64 * 1024 and g["n_damaged"][rank] == 0, g
        assert g["n_guarded_plain"][rank] == 0, g
    assert g["digest"] == g["digest_plain"], g  # (a): sha256 of every rank's state fields
    assert g["T_vs_single"] < 1e-12, g


# ---- the ensemble kernels ---------------------------------------------------------------------
ENSEMBLE_STEPS_EVERY = {"reference": (20, 5), "paper": (8, 2), "exact": (8, 2)}


def ensemble_cell(cell, n_bars, n_cells, monkeypatch):
    """One (family, model) cell of tests/ensemble_cases.py: tail lanes (65 bars), a second wave and workgroup
    (130); plain, then with a three-stage schedule and a history of 2 probes; every state field (nine, or
    eleven on a paper handle), record and statistic bitwise.  Every cell is a code object of its own, a paper
    handle has two allocations more (s_partial, sigma_partial), and n_cells = 1 is where the clamped chunk
    indices of the two sweeps are most likely to stray.  The reference cells run 20 steps with a record every
    5; the paper and exact cells 8 steps, over which the hot bars stay finite in paper mode, with a record
    every 2: there no NaN is left to hide a poisoned read behind, and every compared value is asserted finite.
    The kernels are pinned to the oracle by tests/test_ensemble*.py on these bars: (c) here is the first bar's
    T against those runs' oracle (1e-10)."""
    _torch()
    from ensemble_cases import oracle_run, plain_and_scheduled
    n_steps, every = ENSEMBLE_STEPS_EVERY[cell.model]
    got = _twice(monkeypatch, lambda R: plain_and_scheduled(cell, n_bars, n_cells, n_steps, every, R.finish))
    assert got["plain/T"].shape == (n_bars, cell.n_T(n_cells)) and got["plain/sigma"].shape == (n_bars, n_cells + 1)
    if cell.paper:
        assert got["plain/s_partial"].shape == got["plain/sigma_partial"].shape == (n_bars, 6 * (n_cells + 1))
    assert got["hist/T"].shape == (4, n_bars, 2)
    assert not got["plain/failed"].any() and not got["sched/failed"].any()
    if cell.finite_sigma:
        for k, v in got.items():
            assert np.all(np.isfinite(v)), k
    ref = oracle_run(cell, 0, n_cells, n_steps)
    assert relerr(got["plain/T"][0], ref["end"]["T"]) <= 1e-10


@pytest.mark.parametrize("n_cells", [3, 16])
@pytest.mark.parametrize("n_bars", [1, 65, 130])
def test_ensemble(n_bars, n_cells, monkeypatch):
    """tv_ensemble.hip, the CG1 reference cell; the other five: tests/test_guard_bands_{dg,paper,exact}.py."""
    from ensemble_cases import CELL
    ensemble_cell(CELL["cg-reference"], n_bars, n_cells, monkeypatch)


# ---- the instruments themselves ---------------------------------------------------------------
def test_library_red_zone_detects_a_planted_write(monkeypatch):
    """One finite double written by a host-to-device copy into the first back-guard word of field T's
    allocation (memory the library owns) is reported with its offset, and its restoration clears the report."""
    _torch()
    from tvfem import RectilinearMesh
    from tvfem._native import FIELD_ID
    from tvfem.problem import ThermoViscoProblem
    guard_env(monkeypatch, 64)
    p = ThermoViscoProblem(RectilinearMesh(AXES["3d"]), (0.0, 1.0), 0.1, {"T": CG, "sigma": CG}, MP, part_axis=2,
                           verbose=False)
    p.setup()
    lib = p._lib
    try:
        n_dofs = p.get_field("T").size  # (before the first count: the transfer's staging buffer is allocated lazily)
        ng, nd, gb = guard_check(lib)
        assert ng > 0 and nd == 0 and gb >= 8, (ng, nd, gb)  # the mode is on: only then is element n a guard word
        ptr, stride = C.c_void_p(), C.c_int64()
        assert lib.tv_field_device_ptr(p._ctx, FIELD_ID["T"], C.byref(ptr), C.byref(stride)) == 0
        n = stride.value  # T has one component: its storage is `stride` doubles long
        assert n >= n_dofs
        hip = lib  # dlsym through libtvfem.so's dependencies: the HIP runtime the library itself calls
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        word = C.c_void_p(ptr.value + 8 * n)
        old = (C.c_uint64 * 1)()
        assert hip.hipMemcpy(old, word, 8, 2) == 0  # device to host
        assert old[0] == 0xFFFFFFFFFFFFFFFF, hex(old[0])
        new = (C.c_double * 1)(1.0)
        assert hip.hipMemcpy(word, new, 8, 1) == 0  # host to device
        ng2, nd2, _ = guard_check(lib)
        msg = lib.tv_last_error(None).decode()
        print("[guard]", msg)
        assert ng2 == ng and nd2 == 1, (ng2, nd2)
        assert "offset 0 past the data" in msg and "(fill 0xFF" in msg, msg
        assert hip.hipMemcpy(word, old, 8, 1) == 0
        assert guard_check(lib)[1] == 0
    finally:
        p.close()
    assert guard_check(lib)[0] == 0


def test_caller_arena_detects_a_planted_write():
    torch = _torch()
    for where in (-1, 0):  # the guard element just before the vector, the one just behind it
        view, ptr, check = guarded(np.arange(100.0), lead=1)
        check()
        whole = view._base.view(torch.float64)  # the arena
        first = (ptr - whole.data_ptr()) // 8
        whole[first + (where if where < 0 else 100)] = 1.5
        with pytest.raises(AssertionError, match="caller arena"):
            check()
