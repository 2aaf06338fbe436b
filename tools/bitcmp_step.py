"""A/B bit-equality helper: run a few coupled steps on a small mesh with the
library TVFEM_LIB selects (or the in-tree one) and save T, sigma, the per-step
(Newton, Krylov) counts and z = tv_precond_apply(r) at the final T (r from a
fixed-seed standard_normal), so two library builds can be compared bit for bit.
GPU only.
    python tools/bitcmp_step.py OUT.npz [jacobi|gmg] [auto|kspcg|single] [--case CASE]
The cases are one per kind of multigrid level 0 and cycle below it (CASES); the
two positional choices apply to cg-box, the default."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "fem-glass-tempering_amd")):  # tests: the meshes
    if d not in sys.path:
        sys.path.insert(0, d)

CG = {"element": "CG", "degree": 1}
DG = {"element": "DG", "degree": 1}
MP = {  # main.py:29-55, as in bench.py
    "f": 0.0, "epsilon": 0.93, "sigma": 5.670e-8, "T_ambient": 600.0, "T_0": 800.0, "alpha": 1.0,
    "htc": 280.1, "rho": 2500.0, "cp": 1433.0, "k": 1.0, "H": 627.8e3, "Tb": 869.0e0, "Rg": 8.314,
    "alpha_solid": 9.10e-6, "alpha_liquid": 25.10e-6, "Tf_init": 873.0,
}
BOX = [np.linspace(0.0, 8.0, 65), np.linspace(0.0, 6.0, 49), np.linspace(0.0, 1.0, 9)]
# tests/test_multigrid.test_gmg_dg_steps_match_oracle
DG_BOX = [np.linspace(0.0, 3.0, 13), np.linspace(0.0, 2.5, 11), np.linspace(0.0, 1.0, 6)]
# case: (T family, sigma family, preconditioner) -- the mesh in mesh_of
CASES = {
    "cg-box": ("CG", "CG", "gmg"),               # point Jacobi over the box hierarchy
    "dg-box": ("DG", "DG", "gmg"),               # DG cell blocks over the CG1 box hierarchy
    "um-amg": ("CG", "CG", "amg"),               # point Jacobi over aggregation (shuffled numbering)
    "um-amg-structured": ("CG", "CG", "amg"),    # ... over the index-space transfers (structured topology)
    "umdg-aux": ("DG", "CG", "aux"),             # the packed block inverses over the CG1 space of the mesh
}


def mesh_of(case, box=None):
    from tvfem import RectilinearMesh
    if case == "cg-box":
        return RectilinearMesh(BOX if box is None else box)
    if case == "dg-box":
        return RectilinearMesh(DG_BOX)
    if case == "umdg-aux":
        from dg_aux_reference import aux_mesh
        return aux_mesh("hex")
    from test_amg import VCYCLE_CASES, _mesh
    name = "structured" if case == "um-amg-structured" else "two_levels"
    return _mesh(*VCYCLE_CASES[name], seed=2, shuffle=name != "structured")


def problem(case, box=None, model_parameters=MP, **kw):
    """the context of a case (not set up); box: other axes for cg-box"""
    from tvfem.problem import ThermoViscoProblem
    fT, fS, pc = CASES[case]
    kw.setdefault("preconditioner", pc)
    kw.setdefault("write_output", False)
    if case == "dg-box":
        kw.setdefault("part_axis", 2)  # as that test
    fam = {"CG": CG, "DG": DG}
    return ThermoViscoProblem(mesh_of(case, box), (0.0, 1.0), 0.1, {"T": fam[fT], "sigma": fam[fS]},
                              dict(model_parameters), verbose=False, **kw)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("pc", nargs="?", default=None, help="cg-box: jacobi or gmg (default)")
    ap.add_argument("pcg", nargs="?", default="auto", help="the Krylov form (pcg_variant)")
    ap.add_argument("--case", choices=list(CASES), default="cg-box")
    a = ap.parse_args()
    if a.pc is not None and a.case != "cg-box":
        ap.error("the preconditioner of every case but cg-box is fixed")
    kw = {} if a.pc is None else {"preconditioner": a.pc}
    p = problem(a.case, pcg_variant=a.pcg, **kw)
    p.setup()
    its = []
    for _ in range(3):
        p.solve_timestep()
        its.append((p.last_newton_iterations, p.last_krylov_iterations))
    T = p.functions_current["T"].x.array.copy()
    r = torch.tensor(np.random.default_rng(7).standard_normal(T.size), dtype=torch.float64, device="cuda")
    z = torch.empty_like(r)  # device layout in and out: the comparison is elementwise
    rc = p._lib.tv_precond_apply(p._ctx, r.data_ptr(), z.data_ptr())
    if rc != 0:
        raise SystemExit(f"tv_precond_apply: {p._lib.tv_last_error(p._ctx)}")
    np.savez(a.out, T=T, sigma=p.functions_next["sigma"].x.array.copy(), its=np.array(its), z=z.cpu().numpy())
    p.close()
    print(a.out, a.case, its)


if __name__ == "__main__":
    main()
