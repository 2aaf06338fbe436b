"""A scheduled, recorded run on a slab-partitioned box vs the same run on one partition: the
check of tools/partition_check.py (T, phi, xi, sigma and the iteration counts) with a process
schedule (--schedule, the JSON of ThermoViscoProblem's `schedule=`) and a run history open on
every rank.  Launched by tests/test_problem_schedule.py as `torch.distributed.run
--nproc-per-node 2`; every rank on GPU 0, host-staged transport over gloo.  A support script
(pytest does not collect it).

Beyond the field comparison it reports, per rank, whether the recorded extrema of the last
record are bitwise the nanmin / nanmax of that rank's OWN owned dofs (get_field), and whether
a hot spot planted on rank 1's interface plane stays out of rank 0's maximum (no ghost is read,
nothing is reduced across ranks).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fem-glass-tempering_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch.distributed as dist  # noqa: E402

from oracle.tv_oracle import MAIN_MODEL_PARAMS  # noqa: E402
from problem_schedule_cases import nan_extrema, same_bits, same_extremum  # noqa: E402
from tvfem import box_mesh  # noqa: E402
from tvfem.parallel import init_host_comm  # noqa: E402
from tvfem.problem import ThermoViscoProblem  # noqa: E402

CFG = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
STEPS = 4


def run(mesh, n_parts, part, schedule, comm=None, history=True):
    p = ThermoViscoProblem(mesh, (0, 1), 0.1, CFG, dict(MAIN_MODEL_PARAMS), n_parts=n_parts, part=part, part_axis=1,
                           verbose=False, write_output=False, schedule=schedule,
                           history=dict(points=[[0.0, 0.0, 0.0], [2.0, 6.0, 1.0]], every=1) if history else None)
    if comm is not None:
        comm(p)
    p.setup()
    its = []
    for _ in range(STEPS):
        p.solve_timestep()
        its.append((p.last_newton_iterations, p.last_krylov_iterations))
    out = {k: p.get_field(k) for k in ("T", "phi", "xi", "sigma")}
    if history:
        if n_parts > 1:
            # a hot spot on rank 1's lowest owned plane (its interface plane, which rank 0 holds as a ghost),
            # then one more step of every rank: rank 0's ghost copy of it is hotter than anything rank 0 owns
            T = np.array(out["T"])
            X = p._dof_coordinates(0)
            on_first = X[:, 1] == X[:, 1].min()  # this rank's lowest owned plane; the spot: its mid-thickness centre
            spot = int(np.flatnonzero(on_first)[np.argmin(np.abs(X[on_first, 0] - 1.0) + np.abs(X[on_first, 2] - 0.6))])
            if part == 1:
                T[spot] += 300.0
            p.set_field("T", T)
            p.solve_timestep(thermal_only=True)
        else:
            spot = 0
        T, sig = p.get_field("T"), p.get_field("sigma").reshape(-1, 9)
        h = p.get_history()
        ok = h["T"].shape[0] == STEPS + (n_parts > 1)
        mn, mx = nan_extrema(T)
        ok = ok and same_extremum(h["T_min"][-1], mn) and same_extremum(h["T_max"][-1], mx)
        for q in range(9):
            mn, mx = nan_extrema(sig[:, q])
            ok = ok and same_extremum(h["sigma_min"][-1, q], mn) and same_extremum(h["sigma_max"][-1, q], mx)
        # the probes are this rank's nearest owned dofs: the record holds their values
        ok = ok and same_bits(h["T"][-1], T[p.history_dofs["T"]])
        ok = ok and same_bits(h["sigma"][-1], sig[p.history_dofs["sigma"]])
        out["hist"] = {"own": bool(ok), "records": int(h["T"].shape[0]), "T_spot": float(T[spot]),
                       "T_ext": [float(h["T_min"][-1]), float(h["T_max"][-1])]}
    p.close()
    return out, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--comm", choices=["host"], default="host")
    ap.add_argument("--schedule", required=True, help="JSON list of stage dicts")
    a = ap.parse_args()
    schedule = json.loads(a.schedule)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    mesh = box_mesh([2.0, 6.0, 1.0], [10, 30, 5])
    loc, its = run(mesh, world, rank, schedule, comm=lambda p: init_host_comm(p, rank, world))
    gathered = [None] * world
    dist.all_gather_object(gathered, {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in loc.items()})
    if rank == 0:
        ref, its_ref = run(mesh, 1, 0, schedule)
        plain, _ = run(mesh, 1, 0, None, history=False)
        res = {"its_parts": its, "its_single": its_ref}
        for k in ("T", "phi", "xi", "sigma"):
            full = np.concatenate([np.asarray(g[k]) for g in gathered])
            res[k] = float(np.linalg.norm(full - ref[k]) / np.linalg.norm(ref[k]))
        res["schedule_changed_T"] = float(np.linalg.norm(plain["T"] - ref["T"]) / np.linalg.norm(ref["T"]))
        res["extrema_own"] = [g["hist"]["own"] for g in gathered]
        res["records"] = [g["hist"]["records"] for g in gathered]
        ext = [g["hist"]["T_ext"] for g in gathered]
        res["T_ext"] = ext
        # rank 1's interface value lies above rank 0's recorded maximum: rank 0 did not read its ghost plane
        res["ghosts_excluded"] = bool(gathered[1]["hist"]["T_spot"] > ext[0][1] and ext[1][1] > ext[0][1])
        print("SCHEDULE_PART_CHECK " + json.dumps(res), flush=True)
    dist.barrier()


if __name__ == "__main__":
    main()
