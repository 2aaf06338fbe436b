"""Test infrastructure, launched by tests/test_guard_bands.py as
`torch.distributed.run --nproc-per-node 2 tests/guard_part_check.py [--family F] [--pc P] [--pcg V]`:
one coupled step of the 10 x 30 x 5 box of tools/partition_check.py on slab
partitions over the host-staged transport (every rank on GPU 0), first with the
library's red zones on (TVFEM_ALLOC_GUARD=64, set here before the context is
created), then plain -- ghost planes and send buffers are allocations of the
library.

Every rank reports tv_guard_check of both runs (before the context is closed)
and a sha256 of its state fields; rank 0 also runs the single partition and
compares T.  Prints GUARD_PART_CHECK <json> on rank 0.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fem-glass-tempering_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401
import torch.distributed as dist  # noqa: E402

from tools.partition_check import MP  # noqa: E402
from tvfem import box_mesh  # noqa: E402
from tvfem.parallel import init_host_comm  # noqa: E402
from tvfem.problem import ThermoViscoProblem  # noqa: E402

FIELDS = ("T", "Tf", "phi", "xi", "sigma")


def run(a, mesh, world, rank, guard_kib=0):
    os.environ.pop("TVFEM_ALLOC_GUARD", None)
    if guard_kib:
        os.environ["TVFEM_ALLOC_GUARD"] = str(guard_kib)
    cfg = {"T": {"element": a.family, "degree": 1}, "sigma": {"element": a.family, "degree": 1}}
    p = ThermoViscoProblem(mesh, (0, 1), 0.1, cfg, MP, n_parts=world, part=rank, part_axis=1, verbose=False,
                           pcg_variant=a.pcg, write_output=False, preconditioner=a.pc)
    if world > 1:
        init_host_comm(p, rank, world)
    p.setup()
    p.solve_timestep()
    out = {k: p.get_field(k) for k in FIELDS}
    ng, nd, gb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = p._lib.tv_guard_check(C.byref(ng), C.byref(nd), C.byref(gb))
    if rc != 0:
        raise SystemExit(f"tv_guard_check: {p._lib.tv_last_error(None)}")
    msg = p._lib.tv_last_error(None).decode() if nd.value else ""
    p.close()
    return out, (ng.value, nd.value, gb.value, msg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=["CG", "DG"], default="CG")
    ap.add_argument("--pc", choices=["jacobi", "gmg"], default="jacobi")
    ap.add_argument("--pcg", choices=["auto", "kspcg", "single"], default="auto")
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    mesh = box_mesh([2.0, 6.0, 1.0], [10, 30, 5])

    def digest(out):
        h = hashlib.sha256()
        for k in FIELDS:
            h.update(np.ascontiguousarray(out[k]).tobytes())
        return h.hexdigest()

    out, guard = run(a, mesh, world, rank, 64)
    plain, noguard = run(a, mesh, world, rank)
    got = [None] * world
    dist.all_gather_object(got, (digest(out), digest(plain), int(sum(np.isnan(out[k]).sum() for k in FIELDS)), guard,
                                 noguard[0], out["T"].tolist()))
    if rank == 0:
        single, _ = run(a, mesh, 1, 0)
        T = np.concatenate([np.asarray(g[5]) for g in got])
        res = {"digest": [g[0] for g in got], "digest_plain": [g[1] for g in got], "nan": [g[2] for g in got],
               "n_guarded": [g[3][0] for g in got], "n_damaged": [g[3][1] for g in got],
               "guard_bytes": [g[3][2] for g in got], "damage": [g[3][3] for g in got],
               "n_guarded_plain": [g[4] for g in got],
               "T_vs_single": float(np.linalg.norm(T - single["T"]) / np.linalg.norm(single["T"]))}
        print("GUARD_PART_CHECK " + json.dumps(res), flush=True)
    dist.barrier()


if __name__ == "__main__":
    main()
