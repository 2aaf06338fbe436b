"""What process schedules and run histories cost a ThermoViscoProblem (csrc/tv_history.hip).

    python tools/history_bench.py [--parent-tree DIR] [--out profiles/history_bench.json]

1. A run with neither a schedule nor a history against the parent commit.  The bench-default
   C4 step (50 x 50 x 5 plate, 400 x 400 x 50 hexahedra, CG1, lean state, the preconditioner
   bench.py picks there) of this tree and of DIR -- a built checkout of the parent commit --
   each in a child process of its own, alternating, --reps (5) times: the median step time
   of each and the ratio, against the margin max(2 %, 3 x the parent's rep-to-rep spread), as
   tools/ensemble_bench.py --parent-tree does.  No launch was added to such a run, so it
   must stay inside the margin ("within_margin").
2. The added time of a recorded step: at C4 and at the 3D test size (8 x 6 x 4 cells), the
   same run with history=dict(3 probes, every=1), in the same alternation, the difference of
   the medians, beside the extrema pass's algorithmic bytes, (1 + d*d) * 8 B per owned dof
   read once (+ the probe values, negligible).
3. --summarize CSV: the k_history_* rows of a rocprofv3 --kernel-trace of a recorded run taken
   in a run of its own (tools/history_bench.py --child-steps ... --history under rocprofv3):
   the median duration per kernel, the extrema pass's bytes over it and its fraction of the
   8.0 TB/s HBM peak; merged into --out.

A child (--child TREE) imports the package of TREE, so the parent's tree runs its own library.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # B/s, the spec figure DESIGN.md's fractions use

MP = {"f": 0.0, "epsilon": 0.93, "sigma": 5.670e-8, "T_ambient": 600.0, "T_0": 800.0, "alpha": 1.0, "htc": 280.1,
      "rho": 2500.0, "cp": 1433.0, "k": 1.0, "H": 627.8e3, "Tb": 869.0, "Rg": 8.314, "alpha_solid": 9.10e-6,
      "alpha_liquid": 25.10e-6, "Tf_init": 873.0}  # bench.py's
SIZES = {"C4": ([50.0, 50.0, 5.0], [400, 400, 50]), "3d_test": ([2.0, 2.0, 1.0], [8, 6, 4])}


def child(tree, size, steps, warmup, history):
    """one process: the step time (ms, host clock around steps that end in a device synchronise)"""
    sys.path.insert(0, os.path.join(os.path.abspath(tree), "fem-glass-tempering_amd"))
    from tvfem import box_mesh
    from tvfem.problem import ThermoViscoProblem
    L, nc = SIZES[size]
    cells = nc[0] * nc[1] * nc[2]
    kw = {}
    if history:
        kw["history"] = dict(points=[[0.0, 0.0, 0.0], [L[0] / 2, L[1] / 2, 0.0], [L[0] / 2, L[1] / 2, L[2] / 2]],
                             every=1, max_records=steps + warmup)
    cfg = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
    p = ThermoViscoProblem(box_mesh(L, nc), (0.0, 50.0), 0.1, cfg, MP, materialize=False, verbose=False,
                           preconditioner="gmg" if cells >= 4_000_000 else "jacobi", write_output=False,
                           part_axis=1, **kw)
    p.setup()
    sync = lambda: p._lib.tv_sync(p._ctx)  # noqa: E731
    for _ in range(warmup):
        p.solve_timestep()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        p.solve_timestep()
    sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    n = p.num_dofs(0)[0]
    if history:
        assert p.get_history()["T"].shape[0] == steps + warmup
    p.close()
    print("HISTORY_BENCH_CHILD " + json.dumps({"ms_per_step": ms, "dofs": n}), flush=True)


def run_child(tree, size, steps, warmup, history):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--size", size, "--child-steps", str(steps),
           "--warmup", str(warmup)] + (["--history"] if history else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("HISTORY_BENCH_CHILD ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child failed ({tree}, {size}): " + out.stdout[-1000:] + out.stderr[-2000:])
    return json.loads(line[0].split(" ", 1)[1])


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def measure(a):
    res = {"sizes": {}, "method": "child processes, alternating, median of %d; ms per step over %d steps after %d "
                                  "warm-up steps, host clock closed by tv_sync" % (a.reps, a.steps, a.warmup)}
    for size in a.sizes:
        rows = {"plain": [], "recorded": [], "parent": []}
        dofs = None
        steps = a.steps if size == "C4" else 20 * a.steps  # a window of comparable length at the small size
        for _ in range(a.reps):
            r = run_child(ROOT, size, steps, a.warmup, False)
            rows["plain"].append(r["ms_per_step"])
            dofs = r["dofs"]
            if a.parent_tree and size == "C4":
                rows["parent"].append(run_child(a.parent_tree, size, steps, a.warmup, False)["ms_per_step"])
            rows["recorded"].append(run_child(ROOT, size, steps, a.warmup, True)["ms_per_step"])
        d = 3
        row = {"dofs": dofs, "steps_per_child": steps, "ms_per_step": rows,
               "extrema_bytes": (1 + d * d) * 8 * dofs}
        pm, ps = med_spread(rows["plain"])
        rm, _ = med_spread(rows["recorded"])
        row.update(plain_ms=pm, plain_spread=ps, recorded_ms=rm, added_ms=rm - pm)
        if rows["parent"]:
            qm, qs = med_spread(rows["parent"])
            margin = max(0.02, 3.0 * qs)
            row.update(parent_ms=qm, parent_spread=qs, margin=margin, plain_over_parent=pm / qm,
                       within_margin=pm / qm <= 1.0 + margin)
        res["sizes"][size] = row
        print(f"[history_bench] {size}: " + json.dumps({k: v for k, v in row.items() if k != "ms_per_step"}), flush=True)
    return res


def summarize(path):
    """median duration of each k_history_* kernel of a rocprofv3 kernel trace (ns columns)"""
    dur = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if "k_history_" not in name:
                continue
            key = name[name.index("k_history_"):].split("(")[0].split("E")[0]
            dur.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return {k: {"launches": len(v), "median_us": statistics.median(v) / 1e3} for k, v in dur.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--sizes", nargs="+", default=["C4", "3d_test"], choices=list(SIZES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_bench.json"))
    ap.add_argument("--child", default=None, metavar="TREE", help="(internal) one timed run on TREE's package")
    ap.add_argument("--size", default="C4", choices=list(SIZES))
    ap.add_argument("--child-steps", type=int, default=10)
    ap.add_argument("--history", action="store_true")
    ap.add_argument("--summarize", default=None, metavar="CSV", help="a rocprofv3 kernel trace of a recorded C4 run")
    ap.add_argument("--trace-dofs", type=int, default=8200851, help="--summarize: owned dofs of the traced run (C4)")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.size, a.child_steps, a.warmup, a.history)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    if a.summarize:
        k = summarize(a.summarize)
        nbytes = (1 + 9) * 8 * a.trace_dofs
        t = k["k_history_extrema"]["median_us"] * 1e-6
        res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace, a run of its own", "dofs": a.trace_dofs,
                               "kernels": k, "extrema_bytes": nbytes, "extrema_bytes_per_s": nbytes / t,
                               "extrema_fraction_of_hbm_peak": nbytes / t / HBM_PEAK}
        print("[history_bench] " + json.dumps(res["kernel_trace"]), flush=True)
    else:
        res.update(measure(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
