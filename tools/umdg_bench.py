"""DG1 temperature on a general hexahedral mesh: J x, the fused PCG matvec and a
coupled step on a distorted plate, with the CG1 path of the same mesh in the
same run for context.

    python tools/umdg_bench.py [--cells 96 96 24] [--steps 5] [--warmup 2] [--reps 21] [--pc jacobi|aux]

Per family pairing (DG/CG: csrc/tv_umdg.hip, CG/CG: csrc/tv_um.hip, SELL-64):
  * J x with the Infinity Cache flushed before every launch, the median over
    --reps launches (tv_time_kernel 10), its algorithmic bytes
    (tv_kernel_bytes) and the fraction of the 8.0 TB/s HBM figure;
  * the fused matvec (p <- z + b p, w <- J p, p.w) back to back, unflushed
    (tv_time_kernel 3), and inside the solves (tv_kernel_stats 3);
  * ms per coupled step, Newton and Krylov iterations per step.
The plate keeps its plane-by-plane numbering with two vertex ids swapped, so
the CG path streams its SELL-64 operator (on a structured numbering it would
switch to its half stencils) and both paths see the locality of a generated
mesh; --numbering shuffled removes it.  One JSON to profiles/umdg_bench.json.

--pc aux: the DG/CG plate both ways in one process -- point Jacobi (the
yardstick: the same code path as without the option) and the auxiliary-space
multigrid (TV_PC_AUX, csrc/tv_umdg_aux.hip), --rounds times each, alternating,
every run a fresh context stepping from the same initial condition.  The aux
records add the cycle's time and algorithmic bytes (tv_time_kernel /
tv_kernel_bytes 11: the DG level's pre-smoothing, the transfers and the
levels below), the per-Newton refresh of the boundary cells' block inverses
(id 18) and the creation time (hierarchy and block inverses included).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fem-glass-tempering_amd"))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def run(mesh, fam_T, a, pc="jacobi"):
    from oracle.tv_oracle import MAIN_MODEL_PARAMS
    from tvfem import _native as N
    from tvfem.problem import ThermoViscoProblem
    cfg = {"T": {"element": fam_T, "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
    t0 = time.perf_counter()
    p = ThermoViscoProblem(mesh, (0.0, 1.0), 0.1, cfg, dict(MAIN_MODEL_PARAMS), verbose=False, write_output=False,
                           preconditioner=pc)
    setup_s = time.perf_counter() - t0
    p.setup()
    lib, ctx = p._lib, p._ctx
    for _ in range(a.warmup):
        p.solve_timestep()
    N.check(lib.tv_sync(ctx), ctx)
    N.check(lib.tv_kernel_timing(ctx, 1), ctx)
    its = []
    t0 = time.perf_counter()
    for _ in range(a.steps):
        p.solve_timestep()
        its.append((p.last_newton_iterations, p.last_krylov_iterations))
    N.check(lib.tv_sync(ctx), ctx)
    step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    live, cnt = C.c_double(), C.c_int64()
    N.check(lib.tv_kernel_stats(ctx, 3, C.byref(live), C.byref(cnt)), ctx)
    N.check(lib.tv_kernel_timing(ctx, 0), ctx)
    ms, by = C.c_double(), C.c_double()
    N.check(lib.tv_time_kernel(ctx, 10, a.reps, C.byref(ms)), ctx)
    N.check(lib.tv_kernel_bytes(ctx, 10, C.byref(by)), ctx)
    jx = {"ms_flushed_median": ms.value, "bytes": by.value, "GBps": by.value / (ms.value * 1e-3) / 1e9}
    jx["frac_hbm"] = jx["GBps"] / HBM_PEAK_GBS
    N.check(lib.tv_time_kernel(ctx, 0, a.reps, C.byref(ms)), ctx)
    jx["ms_back_to_back"] = ms.value
    N.check(lib.tv_time_kernel(ctx, 3, a.reps, C.byref(ms)), ctx)
    N.check(lib.tv_kernel_bytes(ctx, 3, C.byref(by)), ctx)
    fused = {"ms_back_to_back": ms.value, "ms_in_solve": live.value, "launches_timed": cnt.value,
             "bytes": jx["bytes"] - 16.0 * p.num_dofs(0)[0] + by.value}
    fused["GBps_in_solve"] = fused["bytes"] / (live.value * 1e-3) / 1e9 if live.value > 0 else None
    n = p.num_dofs(0)[0]
    extra = {}
    if pc == "aux":
        for key, kid in (("cycle", 11), ("block_refresh", 18)):
            N.check(lib.tv_time_kernel(ctx, kid, a.reps, C.byref(ms)), ctx)
            N.check(lib.tv_kernel_bytes(ctx, kid, C.byref(by)), ctx)
            extra[key] = {"ms_back_to_back": ms.value, "bytes": by.value,
                          "GBps": by.value / (ms.value * 1e-3) / 1e9 if ms.value > 0 else None}
    p.close()
    return {"T_family": fam_T, "sigma_family": "CG", "preconditioner": pc, "T_dofs": n, "create_s": setup_s,
            "ms_per_step": step_ms, "newton_its_per_step": float(np.mean([i[0] for i in its])),
            "krylov_its_per_step": float(np.mean([i[1] for i in its])), "jacobian_apply": jx, "fused_matvec": fused,
            **extra}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, nargs=3, default=[96, 96, 24], help="hexahedra per axis of the plate")
    ap.add_argument("--lengths", type=float, nargs=3, default=[4.0, 4.0, 1.0])
    ap.add_argument("--amp", type=float, default=0.1,
                    help="vertex jitter as a fraction of the cell size.  The reference's SIPG penalty 5 / h (h the "
                         "cell diameter) is only just coercive on cells this small (dt alpha / h^2 = 58): the "
                         "oracle's own J loses definiteness at 0.3 on 400 cells, and the larger the plate the "
                         "earlier its worst cell does")
    ap.add_argument("--numbering", choices=["local", "shuffled"], default="local",
                    help="local: numbered plane by plane as a mesh generator would, two vertex ids swapped; "
                         "shuffled: vertex ids and cell order permuted at random (no locality)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21, help="timed launches per isolated kernel (median / mean)")
    ap.add_argument("--only", choices=["DG", "CG"], default=None, help="time one temperature family only")
    ap.add_argument("--pc", choices=["jacobi", "aux"], default="jacobi",
                    help="aux: the DG/CG plate with point Jacobi and with the auxiliary-space multigrid, alternating")
    ap.add_argument("--rounds", type=int, default=2, help="--pc aux: runs per preconditioner")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umdg_bench.json"))
    a = ap.parse_args()
    from tvfem import distorted_box_mesh
    mesh = distorted_box_mesh(a.lengths, a.cells, amp=a.amp, seed=0, shuffle=a.numbering == "shuffled")
    if a.numbering == "local":  # the plate's own numbering but for vertices 0 and 1: local, not structured
        from tvfem import UnstructuredMesh
        x, cells = mesh.x.copy(), mesh.cells.copy()
        x[[0, 1]] = x[[1, 0]]
        cells[mesh.cells == 0], cells[mesh.cells == 1] = 1, 0
        mesh = UnstructuredMesh(3, x, cells)
    res = {"mesh": {"cells": a.cells, "lengths": a.lengths, "n_cells": mesh.num_cells,
                    "n_vertices": mesh.num_vertices, "distortion": f"amp {a.amp:g}, seed 0", "numbering": a.numbering},
           "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "hbm_peak_GBps": HBM_PEAK_GBS,
           "runs": [run(mesh, f, a) for f in ("DG", "CG") if a.only in (None, f) and not (a.pc == "aux" and f == "DG")]}
    if a.pc == "aux" and a.only in (None, "DG"):
        # the yardstick is the Jacobi step of this very process; rounds alternate so that drift hits both alike
        pairs = [[run(mesh, "DG", a, pc) for pc in ("jacobi", "aux")] for _ in range(max(1, a.rounds))]
        by_pc = {pc: [r[k] for r in pairs] for k, pc in enumerate(("jacobi", "aux"))}
        best = {pc: min(rs, key=lambda r: r["ms_per_step"]) for pc, rs in by_pc.items()}
        for pc in ("jacobi", "aux"):
            best[pc]["ms_per_step_rounds"] = [r["ms_per_step"] for r in by_pc[pc]]
            best[pc]["create_s_rounds"] = [r["create_s"] for r in by_pc[pc]]
        res["runs"] = [best["jacobi"], best["aux"]] + res["runs"]
        res["aux_vs_jacobi"] = {
            "step_time_ratio": best["aux"]["ms_per_step"] / best["jacobi"]["ms_per_step"],
            "krylov_ratio": best["aux"]["krylov_its_per_step"] / best["jacobi"]["krylov_its_per_step"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
