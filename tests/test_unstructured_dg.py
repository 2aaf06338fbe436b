"""DG1 temperature on general quadrilateral / hexahedral meshes (csrc/tv_umdg.hip):
the reference's own pairing (main.py: DG1 temperature, CG1 stress) and the
other family pairings on distorted, shuffled meshes, against the oracle's
generic SIPG assembly (oracle/tv_oracle.py HeatForm._prep_interior,
_sipg_matrix) and its Jacobi-PCG Newton steps.

The meshes are the smallest that still cross a 64-cell wave boundary (72 and
140 cells, no multiple of 64): amp 0.2, seed 0, as tests/test_um_facets.py.

Tolerances are the bars of tests/test_unstructured.py and tests/parity_util.py:
operators F, J x, diag J rel. L2 <= 1e-12 (the same quadrature on both sides;
the oracle places the '-' facet points by a Newton iteration, the device from
the vertex correspondence: 3.5e-15 apart); T and Tf per step <= 1e-10; Newton
counts equal, Krylov counts within max(Newton count, 5 %); stresses by
check_field at min_frac 0.9.
"""
import functools
import os

import numpy as np
import pytest

from oracle import tv_oracle as O
from parity_util import check_field, relerr

pytestmark = pytest.mark.gpu

CG = {"element": "CG", "degree": 1}
DG = {"element": "DG", "degree": 1}
FAM = {"CG": CG, "DG": DG}

MESHES = {
    "quad": ((9, 8), (3.0, 2.0), True),
    "hex": ((7, 5, 4), (2.0, 2.0, 1.0), True),
    "hex_ordered": ((7, 5, 4), (2.0, 2.0, 1.0), False),
}
N_STEPS = 4


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@functools.lru_cache(maxsize=None)
def mesh(name):
    from tvfem import distorted_box_mesh
    n, L, shuffle = MESHES[name]
    return distorted_box_mesh(L, n, amp=0.2, seed=0, shuffle=shuffle)


def oracle_mesh(m):
    return O.Mesh(dim=m.dim, x=m.x[:, :m.dim].copy(), cells=m.cells.copy())


def device_layout(dim, a):
    """cell-major DG vector (dof = cell 2^dim + l) -> the device's [l][cell]"""
    return np.ascontiguousarray(np.asarray(a).reshape(-1, 2 ** dim).T).reshape(-1)


def host_layout(dim, a):
    return np.ascontiguousarray(np.asarray(a).reshape(2 ** dim, -1).T).reshape(-1)


def config(fT, fS):
    return {"T": FAM[fT], "sigma": FAM[fS]}


def device(name, fT="DG", fS="CG", mode="reference", **kw):
    from tvfem.problem import ThermoViscoProblem
    return ThermoViscoProblem(mesh(name), (0.0, 1.0), 0.1, config(fT, fS), dict(O.MAIN_MODEL_PARAMS), verbose=False,
                              model_mode=mode, **kw)


def oracle(name, fT="DG", fS="CG", mode="reference"):
    return O.OracleProblem(oracle_mesh(mesh(name)), (0.0, 1.0), 0.1, config(fT, fS), dict(O.MAIN_MODEL_PARAMS),
                           linear="pcg", model_mode=mode)


@functools.lru_cache(maxsize=None)
def oracle_steps(name, fT, fS, mode):
    """The oracle's N_STEPS steps, computed once per case and read only: T after every step, the
    last step's T change mask per sigma dof, Tf, sigma and the (Newton, Krylov) history."""
    ref = oracle(name, fT, fS, mode)
    ref.setup()
    Ts = []
    for _ in range(N_STEPS):
        T_before = ref.functions_current["T"].copy()
        ref.solve_timestep()
        Ts.append(ref.functions_current["T"].copy())
    mT = np.abs(Ts[-1] - T_before) > 1e-6
    return {"T": Ts, "mS": mT[ref._maps[("S", "T")]], "Tf": ref.functions_current["Tf"].copy(),
            "sigma": ref.functions_next["sigma"].copy(), "history": list(ref.newton_history)}


@functools.lru_cache(maxsize=None)
def operator_case(name):
    """T, T_prev, x of test_unstructured_operators_match_oracle on the DG dof coordinates, and
    the oracle's F, J, diag J"""
    ref = oracle(name)
    ref.setup()
    rng = np.random.default_rng(0)
    n = ref.VT.n
    X = ref.VT.dof_coordinates()
    T = 700.0 + 100.0 * np.cos(X[:, 0] / 0.7) + rng.uniform(-5, 5, n)
    Tp = T + rng.uniform(-3, 3, n)
    x = rng.standard_normal(n)
    y = rng.standard_normal(n)
    J = ref.form.jacobian(T)
    return {"X": X, "T": T, "Tp": Tp, "x": x, "y": y, "F": ref.form.residual(T, Tp), "J": J, "diag": J.diagonal()}


# ---- 4. operators ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_dg_operators_match_oracle(name):
    torch = _torch()
    oc = operator_case(name)
    dev = device(name)
    dev.setup()
    d = mesh(name).dim
    assert np.array_equal(dev._dof_coordinates(0)[:, :d], oc["X"])
    assert np.array_equal(dev._dof_coordinates(1)[:, :d], mesh(name).x[:, :d])
    dev.set_field("T", oc["T"])
    dev.set_field("T_prev", oc["Tp"])
    lib, ctx = dev._lib, dev._ctx
    # caller vectors are in the device layout ([l][cell]); the oracle's are cell-major
    t = lambda a: torch.tensor(device_layout(d, a), dtype=torch.float64, device="cuda")  # noqa: E731
    h = lambda a: host_layout(d, a.cpu().numpy())  # noqa: E731
    Td = t(oc["T"])
    Fd = torch.zeros_like(Td)
    assert lib.tv_residual(ctx, Td.data_ptr(), Fd.data_ptr()) == 0
    eF = relerr(h(Fd), oc["F"])
    xd, yd = t(oc["x"]), t(oc["y"])
    Jx, Jy = torch.zeros_like(xd), torch.zeros_like(xd)
    assert lib.tv_jacobian_apply(ctx, xd.data_ptr(), Jx.data_ptr()) == 0
    assert lib.tv_jacobian_apply(ctx, yd.data_ptr(), Jy.data_ptr()) == 0
    Jx, Jy = h(Jx), h(Jy)
    eJ = relerr(Jx, oc["J"] @ oc["x"])
    dd = torch.zeros_like(xd)
    assert lib.tv_jacobian_diag(ctx, dd.data_ptr()) == 0
    eD = relerr(h(dd), oc["diag"])
    sym = abs(oc["y"] @ Jx - oc["x"] @ Jy) / (np.linalg.norm(oc["x"]) * np.linalg.norm(Jy))
    print(f"[um dg] {name}: F {eF:.2e}, J x {eJ:.2e}, diag J {eD:.2e}, |y.Jx - x.Jy| / (|x||Jy|) {sym:.2e}")
    dev.close()
    assert eF < 1e-12 and eJ < 1e-12 and eD < 1e-12
    assert sym <= 1e-12


# ---- 5. coupled steps ------------------------------------------------------------------------
def _check_steps(name, fT, fS, mode, **kw):
    want = oracle_steps(name, fT, fS, mode)
    dev = device(name, fT, fS, mode, **kw)
    dev.setup()
    its, errs = [], []
    for s in range(N_STEPS):
        dev.solve_timestep()
        its.append((dev.last_newton_iterations, dev.last_krylov_iterations))
        errs.append(relerr(dev.functions_current["T"].x.array, want["T"][s]))
    eTf = relerr(dev.functions_current["Tf"].x.array, want["Tf"])
    sigma = np.array(dev.functions_next["sigma"].x.array)
    dev.close()
    print(f"[um dg] {name} {fT}/{fS} {mode}: T per step {['%.1e' % e for e in errs]}, Tf {eTf:.1e}, "
          f"(Newton, Krylov) {its} oracle {want['history']}")
    assert max(errs) < 1e-10, errs
    for (n_d, k_d), (n_r, k_r) in zip(its, want["history"]):
        assert n_d == n_r, (its, want["history"])
        assert abs(k_d - k_r) <= max(n_r, int(np.ceil(0.05 * k_r))), (its, want["history"])
    assert eTf < 1e-10
    check_field(f"sigma[{name},{fT}/{fS},{mode}]", sigma, want["sigma"], want["mS"], mesh(name).dim ** 2,
                min_frac=0.9)


@pytest.mark.parametrize("mode", ["reference", "paper"])
@pytest.mark.parametrize("name", list(MESHES))
def test_dg_cg_steps_match_oracle(name, mode):
    _torch()
    _check_steps(name, "DG", "CG", mode)


@pytest.mark.parametrize("mode", ["reference", "paper"])
@pytest.mark.parametrize("fT,fS", [("DG", "DG"), ("CG", "DG")])
def test_other_pairings_match_oracle(fT, fS, mode):
    _torch()
    _check_steps("hex", fT, fS, mode)


STATE = ("T", "T_prev", "Tf", "Tf_partial", "phi", "xi", "s_tilde_partial", "sigma_tilde_partial", "sigma")


def _state(dev):
    return {k: np.array(dev.get_field(k)) for k in STATE}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_lean_state_is_bitwise_the_materialized_one():
    _torch()
    a, b = device("hex", materialize=True), device("hex", materialize=False)
    for p in (a, b):
        p.setup()
        for _ in range(N_STEPS):
            p.solve_timestep()
    sa, sb = _state(a), _state(b)
    counts = (a.last_newton_iterations, a.last_krylov_iterations) == (b.last_newton_iterations,
                                                                      b.last_krylov_iterations)
    a.close()
    b.close()
    assert counts
    for k in STATE:
        assert _same_bits(sa[k], sb[k]), k


# ---- 6. a rectilinear grid through both DG device paths ---------------------------------------
def test_rectilinear_as_unstructured_matches_box_dg_path():
    _torch()
    from tvfem import RectilinearMesh, UnstructuredMesh
    from tvfem.problem import ThermoViscoProblem
    axes = [np.linspace(0.0, 2.0, 9), np.linspace(0.0, 1.5, 7), np.array([0.0, 0.2, 0.5, 1.0])]
    cfg = config("DG", "CG")
    a = ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, cfg, dict(O.MAIN_MODEL_PARAMS), verbose=False,
                           part_axis=2)
    b = ThermoViscoProblem(UnstructuredMesh.from_rectilinear(RectilinearMesh(axes)), (0.0, 1.0), 0.1, cfg,
                           dict(O.MAIN_MODEL_PARAMS), verbose=False)
    a.setup()
    b.setup()
    assert np.array_equal(a._dof_coordinates(0), b._dof_coordinates(0))
    errs, its = [], []
    for s in range(3):
        a.solve_timestep()
        b.solve_timestep()
        errs.append(relerr(b.functions_current["T"].x.array, a.functions_current["T"].x.array))
        its.append((a.last_newton_iterations, b.last_newton_iterations))
    a.close()
    b.close()
    print(f"[um dg] rectilinear grid, box DG path vs general-mesh DG path: T {['%.1e' % e for e in errs]}")
    assert max(errs) < 1e-12, errs
    assert all(x == y for x, y in its), its


def test_large_quadrilateral_grid_operators_match_box_dg_path():
    """768 x 704 = 540,672 cells: above 2048 workgroups x 4 waves x 64 cells, where every wave of the
    J x kernel takes several cell groups (no smaller mesh reaches that loop).  F, J x and diag J of a
    rectilinear grid through this path against the box DG kernels, at the operator bar; no solve."""
    torch = _torch()
    from tvfem import RectilinearMesh, UnstructuredMesh
    from tvfem.problem import ThermoViscoProblem
    axes = [np.linspace(0.0, 38.4, 769), np.linspace(0.0, 35.2, 705)]
    cfg = config("DG", "CG")
    rm = RectilinearMesh(axes)
    a = ThermoViscoProblem(rm, (0.0, 1.0), 0.1, cfg, dict(O.MAIN_MODEL_PARAMS), verbose=False)
    b = ThermoViscoProblem(UnstructuredMesh.from_rectilinear(rm), (0.0, 1.0), 0.1, cfg, dict(O.MAIN_MODEL_PARAMS),
                           verbose=False)
    n = a.num_dofs(0)[0]
    assert n == b.num_dofs(0)[0] == 4 * 768 * 704
    rng = np.random.default_rng(1)
    T = 700.0 + rng.uniform(-50, 50, n)
    Td = torch.tensor(device_layout(2, T), dtype=torch.float64, device="cuda")
    xd = torch.tensor(rng.standard_normal(n), dtype=torch.float64, device="cuda")
    out = []
    for p in (a, b):
        p.setup()
        p.set_field("T", T)
        p.set_field("T_prev", T + 1.0)
        F, y, d = torch.zeros_like(Td), torch.zeros_like(Td), torch.zeros_like(Td)
        assert p._lib.tv_residual(p._ctx, Td.data_ptr(), F.data_ptr()) == 0
        assert p._lib.tv_jacobian_apply(p._ctx, xd.data_ptr(), y.data_ptr()) == 0
        assert p._lib.tv_jacobian_diag(p._ctx, d.data_ptr()) == 0
        out.append([v.cpu().numpy() for v in (F, y, d)])
        p.close()
    errs = [relerr(u, v) for u, v in zip(out[1], out[0])]
    print(f"[um dg] 540,672 quadrilaterals, general-mesh path vs box DG path: F {errs[0]:.2e}, J x {errs[1]:.2e}, "
          f"diag J {errs[2]:.2e}")
    assert max(errs) < 1e-12, errs


# ---- 7. exact relaxation ---------------------------------------------------------------------
def test_exact_relaxation_touches_only_the_stress():
    _torch()
    ex, ta = device("hex", mode="paper", relaxation="exact"), device("hex", mode="paper")
    assert (ex.relaxation, ta.relaxation) == ("exact", "taylor")
    for p in (ex, ta):
        p.setup()
        for _ in range(N_STEPS):
            with np.errstate(all="ignore"):
                p.solve_timestep()
    se, st = _state(ex), _state(ta)
    ex.close()
    ta.close()
    for k in ("T", "Tf", "phi", "xi"):
        assert _same_bits(se[k], st[k]), k
    assert np.all(np.isfinite(se["sigma"]))
    assert not _same_bits(se["sigma"], st["sigma"])


# ---- 8. output -------------------------------------------------------------------------------
def test_dg_output_series(tmp_path):
    _torch()
    from tvfem.xdmf import read_series
    out = os.path.join(tmp_path, "umdg_out")
    m = mesh("hex")
    dev = device("hex", write_output=True, output_dir=out)
    dev.setup()
    for _ in range(2):
        dev.solve_timestep()
    T_last = dev.functions_current["T"].x.array.copy()
    sigma_last = dev.functions_next["sigma"].x.array.copy()
    dev.close()
    vtk = [0, 1, 3, 2, 4, 5, 7, 6]
    s = read_series(os.path.join(out, "T.xdmf"))
    assert len(s["times"]) == 3
    # the discontinuous copy of the mesh: node = (cell, l), cell-major
    assert np.array_equal(s["geometry"], m.x[m.cells].reshape(-1, 3))
    assert np.array_equal(s["topology"], np.arange(m.num_cells * 8).reshape(-1, 8)[:, vtk])
    assert np.array_equal(s["values"][-1].ravel(), T_last)
    g = read_series(os.path.join(out, "sigma.xdmf"))
    assert len(g["times"]) == 3
    assert np.array_equal(g["geometry"], m.x) and np.array_equal(g["topology"], m.cells[:, vtk])
    assert np.array_equal(g["values"][-1].ravel(), sigma_last)


# ---- 9. refusals -----------------------------------------------------------------------------
def test_refusals_name_their_reason():
    _torch()
    from tvfem import _native as N
    with pytest.raises(N.NativeError) as ei:
        device("quad", preconditioner="amg")
    assert ei.value.code == N.TV_ERR_ARG and "TV_PC_AMG needs a CG temperature" in str(ei.value)
    ok = device("quad")
    ok.setup()
    ok.solve_timestep()
    ok.close()
    for fT, fS in (("DG", "CG"), ("CG", "DG")):
        with pytest.raises(N.NativeError) as ei:
            device("hex", fT, fS, n_parts=2, part=0)
        assert ei.value.code == N.TV_ERR_ARG and "CG temperature and stress spaces only" in str(ei.value)
    ok = device("hex")
    ok.setup()
    ok.solve_timestep()
    ok.close()
