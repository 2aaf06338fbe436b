#!/usr/bin/env python
"""Throughput of ThermoViscoEnsemble against one bar after another.

Workload: the graded geometry.create_mesh bar, CG1 / CG1, the main.py
parameters with htc spread linearly over 50 .. 1000, 500 steps (main.py's
run).  Timed, each after a warm-up of the same shape:

  * ensembles of 64, 1024, 4096 and 16384 bars: host clock around solve(),
    which returns after the device has finished (median of --reps fresh
    ensembles);
  * the same work without the ensemble: 4 bars one after another through
    ThermoViscoProblem, 500 steps each, the clock around solve() and a field
    read that waits for the device (context creation left out); scaled
    linearly to any ensemble size.

Writes one JSON (default profiles/ensemble_bench.json): bar-steps/s per size,
the sequential rate, the ratio, and the whole-solve fraction of the HBM peak
from the kernel's algorithmic bytes ("1D ensembles"):

  per node and Newton iteration   80 B  forward sweep reads T, T_prev and two
                                        cell coefficients, writes the two
                                        Thomas scratch values; back
                                        substitution reads them and T, writes T
  per node and step              344 B  the viscoelastic update: reads T,
                                        T_prev, 6 Tf_partial, 12 tilde values;
                                        writes 6 Tf_partial, Tf, phi, xi,
                                        12 tilde values, sigma, T_prev

The floor the design must hold: at 4096 bars at least 64x (one wavefront's
width) the sequential bar-steps/s; the tool exits non-zero below it.

--scheduled measures what process schedules and probe histories cost instead
(default output profiles/ensemble_schedule_bench.json): per size the wall time
of the same run without a schedule, of a two-stage run (per-bar quench ends
spread over steps 20 .. 100, htc 900 -> 60, three probes, a record every 10
steps), and -- with --parent-tree, a built checkout of the parent commit --
of the unscheduled run there, measured by the parent's own copy of this tool
in a child process of the same session (numbers of different machines or days
are not comparable).  The margin the two new figures are held against is
the larger of 2 % and three times the parent's own rep-to-rep spread.

--dg measures the DG1-temperature / CG1-stress ensemble (main.py's own
fe_config, csrc/tv_ensemble_dg.hip; default output
profiles/ensemble_dg_bench.json): the same bar (48 cells, 96 T dofs), parameters
and sizes, against --seq-bars bars one after another through ThermoViscoProblem
with the same DG / CG config, and in the same run the CG1 / CG1 ensemble, for
the DG / CG time ratio beside the ratio of the algorithmic bytes:

  per cell and Newton iteration  176 B  forward sweep reads 2 T, 2 T_prev and
                                        two cell coefficients, writes the six
                                        values of C and d; back substitution
                                        reads them and 2 T, writes 2 T
  per T dof and step             144 B  t_part: reads T, T_prev, 6 Tf_partial;
                                        writes 6 Tf_partial, Tf, phi, xi, T_prev
  per mesh node and step         200 B  s_part: reads 12 tilde values; writes
                                        them and sigma

The same 64x floor at 4096 bars holds; the tool exits non-zero below it.

--paper measures the paper model mode (model_mode="paper", the kPaper
instantiations of both kernels; default output
profiles/ensemble_paper_bench.json, one key per pairing), CG1 / CG1 or with --dg
DG1 / CG1: the same
bar, parameters (T_0 = 800 K, inside the Taylor limit) and sizes, in one run the
paper ensemble, the reference-mode ensemble and --seq-bars (default here: 1)
paper-mode bars through ThermoViscoProblem(model_mode="paper"); per size the
paper / reference time ratio beside the ratio of the algorithmic bytes.  Paper
mode adds to the viscoelastic update one read of Tf per T dof and twelve
written partial stresses per node:

  CG   per node and step      448 B  (reference 344 B)
  DG   per T dof and step     152 B  (reference 144 B)
       per mesh node and step 296 B  (reference 200 B)

The ratios are recorded, not judged; the 64x floor at 4096 bars against the
paper-mode sequential path holds, and the tool exits non-zero below it.

--exact measures the exact exponential relaxation (model_mode="paper",
relaxation="exact", the kModel = 2 instantiations; default output
profiles/ensemble_exact_bench.json, one key per pairing), CG1 / CG1 or with --dg
DG1 / CG1: the setup of --paper except T_0 = 873 K, above Tb, where the Taylor
form overflows.  In one run the exact ensemble, the same ensemble with
relaxation="taylor" (its stress overflows at this T_0; the thermal problem and
the Newton counts do not see it, and only its time is used) and --seq-bars
(default 1) bars through ThermoViscoProblem(model_mode="paper",
relaxation="exact") with the ensemble's own parameters, T_0 = 873 K included:
the same model on both sides of the ratio.  The relaxation moves
no byte; per Prony term two exp and two expm1 calls take the place of two
short polynomials.  The exact / taylor time ratio is recorded,
not judged; the 64x floor at 4096 bars holds, and the tool exits non-zero below.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fem-glass-tempering_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12  # B/s, MI355X
FLOOR = 64.0
CFGS = {"cg": {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}},
        "dg": {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}}
FAMILIES = {"cg": "CG1/CG1", "dg": "DG1/CG1"}
# ThermoViscoEnsemble keywords of a model
ENS_KW = {"reference": {}, "paper": dict(model_mode="paper"), "exact": dict(model_mode="paper", relaxation="exact")}
# the algorithmic bytes (module docstring): CG per node, DG per cell / T dof / node; [reference, paper]
BYTES_NODE_NEWTON = 80
BYTES_NODE_STEP = [344, 448]
DG_BYTES_CELL_NEWTON = 176
DG_BYTES_TDOF_STEP = [144, 152]
DG_BYTES_NODE_STEP = [200, 296]
EXACT_T_0 = 873.0  # above Tb = 869 K, where glass is tempered from: outside the Taylor limit


def _rec(vgpr, sgpr_spill, private=0):
    return {"vgpr_count": vgpr, "sgpr_spill_count": sgpr_spill, "vgpr_spill_count": 0,
            "private_segment_fixed_size": private, "scratch_instructions": 0, "occupancy_waves_per_simd": 2}


# the cross-compiler's resource report of the instantiations of csrc/tv_ensemble_step.h in csrc/tv_ensemble.hip
# and csrc/tv_ensemble_dg.hip (gfx950, the Makefile's flags: -O3 -ffp-contract=off; tools/kres.py; DESIGN.md
# section 15 says how it is obtained).  scratch_instructions counts scratch loads / stores in the instruction
# stream.
KERNEL_RECORD = {
    ("cg", "reference", "plain"): _rec(234, 63), ("cg", "reference", "scheduled"): _rec(239, 77),
    ("dg", "reference", "plain"): _rec(236, 63), ("dg", "reference", "scheduled"): _rec(241, 73, 20),
    ("cg", "paper", "plain"): _rec(233, 82), ("cg", "paper", "scheduled"): _rec(237, 96, 20),
    ("dg", "paper", "plain"): _rec(238, 61), ("dg", "paper", "scheduled"): _rec(243, 79, 20),
    ("cg", "exact", "plain"): _rec(235, 73), ("cg", "exact", "scheduled"): _rec(239, 135, 20),
    ("dg", "exact", "plain"): _rec(241, 92), ("dg", "exact", "scheduled"): _rec(245, 117, 20),
}


def kernel_record(fam, model):
    return {kind + "_instantiation": KERNEL_RECORD[fam, model, kind] for kind in ("plain", "scheduled")}


def bytes_per_bar_step(fam, paper, its, n_nodes):
    n_cells = n_nodes - 1
    if fam == "dg":
        return (n_cells * DG_BYTES_CELL_NEWTON * its + 2 * n_cells * DG_BYTES_TDOF_STEP[paper]
                + n_nodes * DG_BYTES_NODE_STEP[paper])
    return n_nodes * (BYTES_NODE_NEWTON * its + BYTES_NODE_STEP[paper])


def bytes_model(fam, paper):
    if fam == "dg":
        d = {"per_cell_newton_iteration": DG_BYTES_CELL_NEWTON, "per_T_dof_step": DG_BYTES_TDOF_STEP[paper],
             "per_node_step": DG_BYTES_NODE_STEP[paper]}
        return dict(d, reference_per_T_dof_step=DG_BYTES_TDOF_STEP[0],
                    reference_per_node_step=DG_BYTES_NODE_STEP[0]) if paper else d
    d = {"per_node_newton_iteration": BYTES_NODE_NEWTON, "per_node_step": BYTES_NODE_STEP[paper]}
    return dict(d, reference_per_node_step=BYTES_NODE_STEP[0]) if paper else d


def mode_of(args):
    """What one run measures: the cell (family, model) and the cell it is held against, the names under which
    the comparison is written, T_0, the output file and whether it is keyed by the families, --seq-bars."""
    fam = "dg" if args.dg else "cg"
    timed = "solve() and a final field read per bar; context creation and setup left out"
    if args.exact:
        return dict(cell=(fam, "exact"), label=f"exact {FAMILIES[fam]}", baseline=(fam, "paper"),
                    baseline_key="taylor_ensemble", baseline_label="taylor", time_ratio="exact_over_taylor_time",
                    bytes_ratio=None, T_0=EXACT_T_0, out="ensemble_exact_bench.json", keyed=True, seq_bars=1,
                    bytes_model="paper mode's (tools/ensemble_bench.py --paper): the relaxation moves no byte",
                    timed="ThermoViscoProblem {families} model_mode=paper relaxation=exact at the ensemble's own "
                          "T_0 = {T_0:g} K, all {steps} steps: " + timed)
    if args.paper:
        return dict(cell=(fam, "paper"), label=f"paper {FAMILIES[fam]}", baseline=(fam, "reference"),
                    baseline_key="reference_ensemble", baseline_label="reference",
                    time_ratio="paper_over_reference_time", bytes_ratio="paper_over_reference_algorithmic_bytes",
                    T_0=None, out="ensemble_paper_bench.json", keyed=True, seq_bars=1,
                    bytes_model=bytes_model(fam, True),
                    timed="ThermoViscoProblem {families} model_mode=paper: " + timed)
    if args.dg:
        return dict(cell=("dg", "reference"), label="DG", baseline=("cg", "reference"), baseline_key="cg_ensemble",
                    baseline_label="CG", time_ratio="dg_over_cg_time", bytes_ratio="dg_over_cg_algorithmic_bytes",
                    T_0=None, out="ensemble_dg_bench.json", keyed=False, seq_bars=4,
                    bytes_model=bytes_model("dg", False), timed="ThermoViscoProblem DG1/CG1: " + timed)
    return dict(cell=("cg", "reference"), label="", baseline=None, T_0=None, out="ensemble_bench.json", keyed=False,
                seq_bars=4, bytes_model=bytes_model("cg", False), timed=timed)


def _maker(mesh, span, fam, model, params):
    """n_bars -> a set-up ensemble of the cell, htc spread over the bars."""
    from tvfem import ThermoViscoEnsemble

    def ensemble(n_bars):
        ens = ThermoViscoEnsemble(mesh, span, 0.1, CFGS[fam], dict(params, htc=np.linspace(50.0, 1000.0, n_bars)),
                                  **ENS_KW[model])
        ens.setup()
        return ens
    return ensemble


def _write(out, res, key=None):
    """res as the file `out`, or, keyed, as its entry `key`: a run replaces its own key and keeps the others."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if key is not None:
        both = {}
        if os.path.exists(out):
            with open(out) as fh:
                both = json.load(fh)
        both[key] = res
        res = both
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=key is not None)
        fh.write("\n")


def _time_ensembles(make, sizes, steps, reps):
    """Median / min / max wall time of solve(steps) over `reps` fresh ensembles per size, after a warm-up."""
    rows = []
    for n_bars in sizes:
        warm = make(n_bars)
        warm.solve(5)
        warm.close()
        walls, its = [], 0.0
        for _ in range(reps):
            ens = make(n_bars)
            t0 = time.perf_counter()
            ens.solve(steps)  # returns after the device has finished
            walls.append(time.perf_counter() - t0)
            assert not ens.failed_step.any()
            its = float(ens.newton_total.mean()) / steps
            ens.close()
        med = statistics.median(walls)
        rows.append({"n_bars": n_bars, "wall_s": med, "wall_s_min": min(walls), "wall_s_max": max(walls),
                     "spread": (max(walls) - min(walls)) / med, "newton_its_per_step": its})
    return rows


def _time_sequential(mesh, span, cfg, n, steps, params=None, **problem_kw):
    """`n` bars one after another through ThermoViscoProblem, htc spread as in the ensembles, one context per
    bar, after a warm-up: (the time loops alone, the same with context creation and setup).  `params`
    replaces main.py's model parameters."""
    from tvfem.problem import ThermoViscoProblem
    if params is None:
        from main import model_params
    else:
        model_params = params

    def single(htc, steps):
        prob = ThermoViscoProblem(mesh, span, 0.1, cfg, dict(model_params, htc=float(htc)), verbose=False,
                                  write_output=False, **problem_kw)
        prob.setup()
        t0 = time.perf_counter()
        prob.solve(steps)
        prob.get_field("T")  # waits for the queued work
        wall = time.perf_counter() - t0
        prob.close()
        return wall

    single(280.1, 5)
    t0 = time.perf_counter()
    wall = sum(single(htc, steps) for htc in np.linspace(50.0, 1000.0, n))
    return wall, time.perf_counter() - t0


def scheduled_bench(args):
    from geometry import graded_bar
    from main import model_params
    from tvfem import ThermoViscoEnsemble

    mesh = graded_bar()
    n_nodes = mesh.num_vertices
    span = (0.0, args.steps * 0.1)
    CFG = CFGS["cg"]
    plain = _maker(mesh, span, "cg", "reference", model_params)

    def scheduled(n_bars):
        quench_end = np.round(np.linspace(20.0, 100.0, n_bars)).astype(int)
        ens = ThermoViscoEnsemble(mesh, span, 0.1, CFG, dict(model_params), n_bars=n_bars,
                                  schedule=[dict(until_step=quench_end, htc=900.0), dict(htc=60.0)],
                                  history=dict(nodes=[0, (n_nodes - 1) // 2, n_nodes - 1], every=10))
        ens.setup()
        return ens

    def neutral(n_bars):  # the unscheduled physics through the scheduled kernel: what the instantiation costs
        htc = np.linspace(50.0, 1000.0, n_bars)
        ens = ThermoViscoEnsemble(mesh, span, 0.1, CFG, dict(model_params, htc=htc), schedule=[dict(htc=htc)],
                                  history=dict(nodes=[0, (n_nodes - 1) // 2, n_nodes - 1], every=10))
        ens.setup()
        return ens

    parent = None
    if args.parent_tree:  # the parent commit's own tool, package and library, in a process of its own
        tmp = os.path.join(tempfile.mkdtemp(), "parent.json")
        cmd = [sys.executable, os.path.join(os.path.abspath(args.parent_tree), "tools", "ensemble_bench.py"),
               "--steps", str(args.steps), "--reps", str(args.reps), "--seq-bars", "1", "--out", tmp,
               "--sizes"] + [str(n) for n in args.sizes]
        env = {k: v for k, v in os.environ.items() if k not in ("TVFEM_LIB", "PYTHONPATH")}
        subprocess.run(cmd, env=env, check=True, stdout=subprocess.DEVNULL)
        with open(tmp) as fh:
            parent = json.load(fh)["ensemble"]
        for r in parent:
            r["spread"] = (r["wall_s_max"] - r["wall_s_min"]) / r["wall_s"]
    new_plain = _time_ensembles(plain, args.sizes, args.steps, args.reps)
    new_sched = _time_ensembles(scheduled, args.sizes, args.steps, args.reps)
    new_neutral = _time_ensembles(neutral, args.sizes, args.steps, args.reps)
    rows = []
    for i, n_bars in enumerate(args.sizes):
        row = {"n_bars": n_bars, "unscheduled": new_plain[i], "scheduled": new_sched[i],
               "scheduled_over_unscheduled": new_sched[i]["wall_s"] / new_plain[i]["wall_s"],
               "one_stage_own_values_with_history": new_neutral[i],
               "one_stage_own_values_over_unscheduled": new_neutral[i]["wall_s"] / new_plain[i]["wall_s"]}
        line = (f"{n_bars:6d} bars: unscheduled {new_plain[i]['wall_s'] * 1e3:8.2f} ms "
                f"({new_plain[i]['newton_its_per_step']:.3f} its)  "
                f"scheduled {new_sched[i]['wall_s'] * 1e3:8.2f} ms ({new_sched[i]['newton_its_per_step']:.3f} its)  "
                f"one stage, own values {new_neutral[i]['wall_s'] * 1e3:8.2f} ms")
        if parent:
            base = parent[i]["wall_s"]
            row["parent_unscheduled"] = parent[i]
            row["margin"] = max(0.02, 3.0 * parent[i]["spread"])
            row["unscheduled_over_parent"] = new_plain[i]["wall_s"] / base
            row["scheduled_over_parent"] = new_sched[i]["wall_s"] / base
            row["within_margin"] = {"unscheduled": row["unscheduled_over_parent"] <= 1.0 + row["margin"],
                                    "scheduled": row["scheduled_over_parent"] <= 1.0 + row["margin"]}
            line += (f"  parent {base * 1e3:8.2f} ms (spread {parent[i]['spread']:.2%})  ratios "
                     f"{row['unscheduled_over_parent']:.4f} / {row['scheduled_over_parent']:.4f}  "
                     f"margin {row['margin']:.2%}")
        rows.append(row)
        print(line, flush=True)
    res = {"workload": {"mesh": "geometry.graded_bar", "n_nodes": n_nodes, "steps": args.steps, "dt": 0.1,
                        "families": "CG1/CG1", "reps": args.reps,
                        "unscheduled": "htc linspace(50, 1000, n_bars), as ensemble_bench.json",
                        "scheduled": "two stages, quench end per bar linspace(20, 100, n_bars) steps, htc 900 -> 60, "
                                     "probes at the two surfaces and the mid-plane, every 10 steps"},
           "parent": "the parent commit's own checkout and tool, child process of the same session"
                     if parent else None,
           "kernel": kernel_record("cg", "reference"), "sizes": rows}
    out = args.out or os.path.join(ROOT, "profiles", "ensemble_schedule_bench.json")
    _write(out, res)
    print(json.dumps({"out": out}))


def bench(args, mode):
    """The mode's ensemble per size, the ensemble it is held against, the sequential path; one JSON."""
    from geometry import graded_bar
    from main import model_params

    mesh = graded_bar()
    n_nodes = mesh.num_vertices
    n_cells = n_nodes - 1
    span = (0.0, args.steps * 0.1)
    fam, model = mode["cell"]
    paper = model != "reference"
    families = FAMILIES[fam]
    params = dict(model_params) if mode["T_0"] is None else dict(model_params, T_0=mode["T_0"])
    make = _maker(mesh, span, fam, model, params)
    workload = {"mesh": "geometry.graded_bar", "n_nodes": n_nodes, "steps": args.steps, "dt": 0.1,
                "htc": "linspace(50, 1000, n_bars)", "families": families, "reps": args.reps}
    if mode["baseline"]:
        workload["n_cells"] = n_cells
    if paper:
        workload.update(T_0=params["T_0"], model_mode="paper")
    elif fam == "dg":
        workload["n_dofs_T"] = 2 * n_cells
    if model == "exact":  # a last look at the state the timed kernel leaves: finite in exact mode at this T_0
        probe = make(64)
        probe.solve(args.steps)
        sigma = probe.get_field("sigma")
        probe.close()
        if not np.all(np.isfinite(sigma)):
            sys.exit("exact relaxation: sigma is not finite")
        workload.update(relaxation="exact", sigma_abs_max_exact_64_bars=float(np.abs(sigma).max()),
                        taylor_ensemble="the same ensemble with relaxation=taylor, same process; at this T_0 its "
                                        "stress overflows (the thermal problem and the Newton counts are the "
                                        "same), so only its time is used")

    timed = _time_ensembles(make, args.sizes, args.steps, args.reps)
    base = None
    if mode["baseline"]:
        base = _time_ensembles(_maker(mesh, span, *mode["baseline"], params), args.sizes, args.steps, args.reps)
    rows = []
    for i, r in enumerate(timed):
        bar_steps = r["n_bars"] * args.steps
        nbytes = bar_steps * bytes_per_bar_step(fam, paper, r["newton_its_per_step"], n_nodes)
        row = dict(r, bar_steps_per_s=bar_steps / r["wall_s"], algorithmic_bytes=nbytes,
                   hbm_fraction_of_8TBps=nbytes / r["wall_s"] / HBM_PEAK)
        line = (f"{mode['label']} ensemble {r['n_bars']:6d} bars: {r['wall_s'] * 1e3:9.2f} ms  "
                f"{row['bar_steps_per_s']:12.4g} bar-steps/s  {r['newton_its_per_step']:.2f} Newton its/step  "
                f"{row['hbm_fraction_of_8TBps']:.2%} of HBM peak")
        if base is None:
            del row["spread"]  # ensemble_bench.json holds the three wall times
        else:
            b = base[i]
            row[mode["baseline_key"]] = dict(b, bar_steps_per_s=bar_steps / b["wall_s"])
            row[mode["time_ratio"]] = r["wall_s"] / b["wall_s"]
            line += f";  {mode['baseline_label']} {b['wall_s'] * 1e3:9.2f} ms  time ratio {row[mode['time_ratio']]:.3f}"
            if mode["bytes_ratio"]:
                bfam, bmodel = mode["baseline"]
                bbytes = bar_steps * bytes_per_bar_step(bfam, bmodel != "reference", b["newton_its_per_step"], n_nodes)
                row[mode["baseline_key"]]["algorithmic_bytes"] = bbytes
                row[mode["bytes_ratio"]] = nbytes / bbytes
                line += f"  byte ratio {row[mode['bytes_ratio']]:.3f}"
            if not paper:
                row["us_per_T_dof_and_step_of_a_lane"] = r["wall_s"] / args.steps / (2 * n_cells) * 1e6
        rows.append(row)
        print(line.lstrip(), flush=True)

    # the same work one bar after another (what a parameter study costs without the ensemble), in the
    # ensemble's own model and at its own parameters
    seq_wall, seq_total = _time_sequential(mesh, span, CFGS[fam], args.seq_bars, args.steps, params=params,
                                           **ENS_KW[model])
    seq_rate = args.seq_bars * args.steps / seq_wall  # the time loops alone: context creation left out
    print(f"sequential {args.seq_bars} {mode['label']} bar(s): ".replace("  ", " ")
          + f"{seq_wall:.3f} s  {seq_rate:.4g} bar-steps/s", flush=True)
    for r in rows:
        r["ratio_to_sequential"] = r["bar_steps_per_s"] / seq_rate
    sequential = {"bars": args.seq_bars, "wall_s": seq_wall, "bar_steps_per_s": seq_rate,
                  "timed": mode["timed"].format(families=families, T_0=params["T_0"], steps=args.steps)}
    if base is None:
        sequential["wall_s_with_context_creation"] = seq_total
    if model == "exact":
        sequential["T_0"] = params["T_0"]
    res = {"workload": workload, "bytes_model": mode["bytes_model"]}
    if base is not None:
        res["kernel"] = kernel_record(fam, model)
    res.update(ensemble=rows, sequential=sequential, floor_ratio_at_4096=FLOOR)
    at = [r for r in rows if r["n_bars"] == 4096]
    if at:
        res["ratio_at_4096"] = at[0]["ratio_to_sequential"]
        print(f"ratio at 4096 bars: {res['ratio_at_4096']:.1f}x (floor {FLOOR:g}x)")
    out = args.out or os.path.join(ROOT, "profiles", mode["out"])
    _write(out, res, families if mode["keyed"] else None)
    print(json.dumps({"out": out, "ratio_at_4096": res.get("ratio_at_4096")}))
    if at and res["ratio_at_4096"] < FLOOR:
        sys.exit(f"{mode['label']} ensemble below the {FLOOR:g}x floor at 4096 bars".lstrip())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 4096, 16384])
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seq-bars", type=int, default=None, help="default 4 (--paper: 1)")
    ap.add_argument("--out", default=None, help="default profiles/ensemble_bench.json "
                                                "(--scheduled: profiles/ensemble_schedule_bench.json, "
                                                "--dg: profiles/ensemble_dg_bench.json, "
                                                "--paper: profiles/ensemble_paper_bench.json)")
    ap.add_argument("--scheduled", action="store_true", help="the cost of a schedule and a history (see above)")
    ap.add_argument("--dg", action="store_true",
                    help="the DG1-temperature / CG1-stress ensemble against its sequential path and the CG ensemble")
    ap.add_argument("--parent-tree", default=None,
                    help="--scheduled: a built checkout of the parent commit; its own tools/ensemble_bench.py runs")
    ap.add_argument("--paper", action="store_true",
                    help="the paper-mode ensemble (with --dg: DG1 / CG1) against the reference-mode ensemble and "
                         "its own sequential path")
    ap.add_argument("--exact", action="store_true",
                    help="the exact-relaxation paper ensemble (with --dg: DG1 / CG1) at T_0 = 873 K against the "
                         "paper-mode ensemble and one sequential exact-relaxation bar")
    args = ap.parse_args()
    if args.scheduled and not (args.paper or args.exact):
        return scheduled_bench(args)
    mode = mode_of(args)
    if args.seq_bars is None:
        args.seq_bars = mode["seq_bars"]
    bench(args, mode)


if __name__ == "__main__":
    main()
