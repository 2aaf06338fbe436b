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
(default 1) paper-mode bars through ThermoViscoProblem(model_mode="paper"),
which has no exact mode: that side runs at main.py's T_0 = 800 K, inside the
Taylor limit, so that it stays finite over all the steps.  The relaxation moves
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
BYTES_NODE_NEWTON = 80
BYTES_NODE_STEP = 344
FLOOR = 64.0
CFG = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
CFG_DG = {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
DG_BYTES_CELL_NEWTON = 176
DG_BYTES_TDOF_STEP = 144
DG_BYTES_NODE_STEP = 200
# the cross-compiler's resource report of csrc/tv_ensemble_dg.hip and csrc/tv_ensemble.hip (gfx950, the Makefile's
# flags: -O3 -ffp-contract=off), both instantiations of csrc/tv_ensemble_step.h; DESIGN.md section 15 says how it
# is obtained.  scratch_instructions counts scratch loads / stores in the instruction stream.
DG_KERNEL_RECORD = {
    "plain_instantiation": {"vgpr_count": 236, "sgpr_spill_count": 63, "vgpr_spill_count": 0,
                            "private_segment_fixed_size": 0, "scratch_instructions": 0,
                            "occupancy_waves_per_simd": 2},
    "scheduled_instantiation": {"vgpr_count": 241, "sgpr_spill_count": 73, "vgpr_spill_count": 0,
                                "private_segment_fixed_size": 20, "scratch_instructions": 0,
                                "occupancy_waves_per_simd": 2},
}
KERNEL_RECORD = {
    "plain_instantiation": {"vgpr_count": 234, "sgpr_spill_count": 63, "vgpr_spill_count": 0,
                            "private_segment_fixed_size": 0, "scratch_instructions": 0,
                            "occupancy_waves_per_simd": 2},
    "scheduled_instantiation": {"vgpr_count": 239, "sgpr_spill_count": 77, "vgpr_spill_count": 0,
                                "private_segment_fixed_size": 0, "scratch_instructions": 0,
                                "occupancy_waves_per_simd": 2},
}

PAPER_BYTES_NODE_STEP = 448
PAPER_DG_BYTES_TDOF_STEP = 152
PAPER_DG_BYTES_NODE_STEP = 296
# the kPaper instantiations, obtained the same way (tools/kres.py)
PAPER_KERNEL_RECORD = {
    "plain_instantiation": {"vgpr_count": 233, "sgpr_spill_count": 82, "vgpr_spill_count": 0,
                            "private_segment_fixed_size": 0, "scratch_instructions": 0,
                            "occupancy_waves_per_simd": 2},
    "scheduled_instantiation": {"vgpr_count": 237, "sgpr_spill_count": 96, "vgpr_spill_count": 0,
                                "private_segment_fixed_size": 20, "scratch_instructions": 0,
                                "occupancy_waves_per_simd": 2},
}
PAPER_DG_KERNEL_RECORD = {
    "plain_instantiation": {"vgpr_count": 238, "sgpr_spill_count": 61, "vgpr_spill_count": 0,
                            "private_segment_fixed_size": 0, "scratch_instructions": 0,
                            "occupancy_waves_per_simd": 2},
    "scheduled_instantiation": {"vgpr_count": 243, "sgpr_spill_count": 79, "vgpr_spill_count": 0,
                                "private_segment_fixed_size": 20, "scratch_instructions": 0,
                                "occupancy_waves_per_simd": 2},
}

EXACT_T_0 = 873.0  # above Tb = 869 K, where glass is tempered from: outside the Taylor limit
# the kModel = 2 (exact relaxation) instantiations, obtained the same way
EXACT_KERNEL_RECORD = {
    "plain_instantiation": {"vgpr_count": 235, "sgpr_spill_count": 73, "vgpr_spill_count": 0,
                            "private_segment_fixed_size": 0, "scratch_instructions": 0,
                            "occupancy_waves_per_simd": 2},
    "scheduled_instantiation": {"vgpr_count": 239, "sgpr_spill_count": 135, "vgpr_spill_count": 0,
                                "private_segment_fixed_size": 20, "scratch_instructions": 0,
                                "occupancy_waves_per_simd": 2},
}
EXACT_DG_KERNEL_RECORD = {
    "plain_instantiation": {"vgpr_count": 241, "sgpr_spill_count": 92, "vgpr_spill_count": 0,
                            "private_segment_fixed_size": 0, "scratch_instructions": 0,
                            "occupancy_waves_per_simd": 2},
    "scheduled_instantiation": {"vgpr_count": 245, "sgpr_spill_count": 117, "vgpr_spill_count": 0,
                                "private_segment_fixed_size": 20, "scratch_instructions": 0,
                                "occupancy_waves_per_simd": 2},
}


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

    def plain(n_bars):
        ens = ThermoViscoEnsemble(mesh, span, 0.1, CFG, dict(model_params, htc=np.linspace(50.0, 1000.0, n_bars)))
        ens.setup()
        return ens

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
           "kernel": KERNEL_RECORD, "sizes": rows}
    out = args.out or os.path.join(ROOT, "profiles", "ensemble_schedule_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": out}))


def dg_bench(args):
    from geometry import graded_bar
    from main import model_params
    from tvfem import ThermoViscoEnsemble

    mesh = graded_bar()
    n_nodes = mesh.num_vertices
    n_cells = n_nodes - 1
    span = (0.0, args.steps * 0.1)

    def make(cfg):
        def ensemble(n_bars):
            ens = ThermoViscoEnsemble(mesh, span, 0.1, cfg, dict(model_params, htc=np.linspace(50.0, 1000.0, n_bars)))
            ens.setup()
            return ens
        return ensemble

    dg = _time_ensembles(make(CFG_DG), args.sizes, args.steps, args.reps)
    cg = _time_ensembles(make(CFG), args.sizes, args.steps, args.reps)
    rows = []
    for d, c in zip(dg, cg):
        bar_steps = d["n_bars"] * args.steps
        nbytes = bar_steps * (n_cells * DG_BYTES_CELL_NEWTON * d["newton_its_per_step"]
                              + 2 * n_cells * DG_BYTES_TDOF_STEP + n_nodes * DG_BYTES_NODE_STEP)
        cg_bytes = bar_steps * n_nodes * (BYTES_NODE_NEWTON * c["newton_its_per_step"] + BYTES_NODE_STEP)
        row = dict(d, bar_steps_per_s=bar_steps / d["wall_s"], algorithmic_bytes=nbytes,
                   hbm_fraction_of_8TBps=nbytes / d["wall_s"] / HBM_PEAK,
                   us_per_T_dof_and_step_of_a_lane=d["wall_s"] / args.steps / (2 * n_cells) * 1e6,
                   cg_ensemble=dict(c, bar_steps_per_s=bar_steps / c["wall_s"], algorithmic_bytes=cg_bytes),
                   dg_over_cg_time=d["wall_s"] / c["wall_s"], dg_over_cg_algorithmic_bytes=nbytes / cg_bytes)
        rows.append(row)
        print(f"DG ensemble {d['n_bars']:6d} bars: {d['wall_s'] * 1e3:9.2f} ms  {row['bar_steps_per_s']:12.4g} "
              f"bar-steps/s  {d['newton_its_per_step']:.2f} its/step  {row['hbm_fraction_of_8TBps']:.2%} of HBM peak;  "
              f"CG {c['wall_s'] * 1e3:9.2f} ms  time ratio {row['dg_over_cg_time']:.3f}  "
              f"byte ratio {row['dg_over_cg_algorithmic_bytes']:.3f}", flush=True)

    seq_wall, _ = _time_sequential(mesh, span, CFG_DG, args.seq_bars, args.steps)  # the same bar, DG / CG
    seq_rate = args.seq_bars * args.steps / seq_wall
    print(f"sequential {args.seq_bars} DG/CG bars: {seq_wall:.3f} s  {seq_rate:.4g} bar-steps/s", flush=True)
    for r in rows:
        r["ratio_to_sequential"] = r["bar_steps_per_s"] / seq_rate
    res = {"workload": {"mesh": "geometry.graded_bar", "n_nodes": n_nodes, "n_cells": n_cells,
                        "n_dofs_T": 2 * n_cells, "steps": args.steps, "dt": 0.1, "htc": "linspace(50, 1000, n_bars)",
                        "families": "DG1/CG1", "reps": args.reps},
           "bytes_model": {"per_cell_newton_iteration": DG_BYTES_CELL_NEWTON, "per_T_dof_step": DG_BYTES_TDOF_STEP,
                           "per_node_step": DG_BYTES_NODE_STEP},
           "kernel": DG_KERNEL_RECORD, "ensemble": rows,
           "sequential": {"bars": args.seq_bars, "wall_s": seq_wall, "bar_steps_per_s": seq_rate,
                          "timed": "ThermoViscoProblem DG1/CG1: solve() and a final field read per bar; context "
                                   "creation and setup left out"},
           "floor_ratio_at_4096": FLOOR}
    at = [r for r in rows if r["n_bars"] == 4096]
    if at:
        res["ratio_at_4096"] = at[0]["ratio_to_sequential"]
        print(f"ratio at 4096 bars: {res['ratio_at_4096']:.1f}x (floor {FLOOR:g}x)")
    out = args.out or os.path.join(ROOT, "profiles", "ensemble_dg_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": out, "ratio_at_4096": res.get("ratio_at_4096")}))
    if at and res["ratio_at_4096"] < FLOOR:
        sys.exit(f"DG ensemble below the {FLOOR:g}x floor at 4096 bars")


def paper_bench(args):
    from geometry import graded_bar
    from main import model_params
    from tvfem import ThermoViscoEnsemble

    mesh = graded_bar()
    n_nodes = mesh.num_vertices
    n_cells = n_nodes - 1
    span = (0.0, args.steps * 0.1)
    cfg = CFG_DG if args.dg else CFG
    families = "DG1/CG1" if args.dg else "CG1/CG1"

    def make(mode):
        def ensemble(n_bars):
            ens = ThermoViscoEnsemble(mesh, span, 0.1, cfg, dict(model_params, htc=np.linspace(50.0, 1000.0, n_bars)),
                                      model_mode=mode)
            ens.setup()
            return ens
        return ensemble

    def model_bytes(its, paper):
        if args.dg:
            return (n_cells * DG_BYTES_CELL_NEWTON * its
                    + 2 * n_cells * (PAPER_DG_BYTES_TDOF_STEP if paper else DG_BYTES_TDOF_STEP)
                    + n_nodes * (PAPER_DG_BYTES_NODE_STEP if paper else DG_BYTES_NODE_STEP))
        return n_nodes * (BYTES_NODE_NEWTON * its + (PAPER_BYTES_NODE_STEP if paper else BYTES_NODE_STEP))

    pap = _time_ensembles(make("paper"), args.sizes, args.steps, args.reps)
    ref = _time_ensembles(make("reference"), args.sizes, args.steps, args.reps)
    rows = []
    for p, r in zip(pap, ref):
        bar_steps = p["n_bars"] * args.steps
        nbytes = bar_steps * model_bytes(p["newton_its_per_step"], True)
        ref_bytes = bar_steps * model_bytes(r["newton_its_per_step"], False)
        row = dict(p, bar_steps_per_s=bar_steps / p["wall_s"], algorithmic_bytes=nbytes,
                   hbm_fraction_of_8TBps=nbytes / p["wall_s"] / HBM_PEAK,
                   reference_ensemble=dict(r, bar_steps_per_s=bar_steps / r["wall_s"], algorithmic_bytes=ref_bytes),
                   paper_over_reference_time=p["wall_s"] / r["wall_s"],
                   paper_over_reference_algorithmic_bytes=nbytes / ref_bytes)
        rows.append(row)
        print(f"paper {families} ensemble {p['n_bars']:6d} bars: {p['wall_s'] * 1e3:9.2f} ms  "
              f"{row['bar_steps_per_s']:12.4g} bar-steps/s  {p['newton_its_per_step']:.2f} its/step  "
              f"{row['hbm_fraction_of_8TBps']:.2%} of HBM peak;  reference {r['wall_s'] * 1e3:9.2f} ms  "
              f"time ratio {row['paper_over_reference_time']:.3f}  "
              f"byte ratio {row['paper_over_reference_algorithmic_bytes']:.3f}", flush=True)

    seq_wall, _ = _time_sequential(mesh, span, cfg, args.seq_bars, args.steps, model_mode="paper")
    seq_rate = args.seq_bars * args.steps / seq_wall
    print(f"sequential {args.seq_bars} paper-mode {families} bar(s): {seq_wall:.3f} s  {seq_rate:.4g} bar-steps/s",
          flush=True)
    for r in rows:
        r["ratio_to_sequential"] = r["bar_steps_per_s"] / seq_rate
    res = {"workload": {"mesh": "geometry.graded_bar", "n_nodes": n_nodes, "n_cells": n_cells, "steps": args.steps,
                        "dt": 0.1, "htc": "linspace(50, 1000, n_bars)", "T_0": model_params["T_0"],
                        "families": families, "model_mode": "paper", "reps": args.reps},
           "bytes_model": ({"per_cell_newton_iteration": DG_BYTES_CELL_NEWTON,
                            "per_T_dof_step": PAPER_DG_BYTES_TDOF_STEP, "per_node_step": PAPER_DG_BYTES_NODE_STEP,
                            "reference_per_T_dof_step": DG_BYTES_TDOF_STEP,
                            "reference_per_node_step": DG_BYTES_NODE_STEP} if args.dg else
                           {"per_node_newton_iteration": BYTES_NODE_NEWTON, "per_node_step": PAPER_BYTES_NODE_STEP,
                            "reference_per_node_step": BYTES_NODE_STEP}),
           "kernel": PAPER_DG_KERNEL_RECORD if args.dg else PAPER_KERNEL_RECORD, "ensemble": rows,
           "sequential": {"bars": args.seq_bars, "wall_s": seq_wall, "bar_steps_per_s": seq_rate,
                          "timed": f"ThermoViscoProblem {families} model_mode=paper: solve() and a final field read "
                                   "per bar; context creation and setup left out"},
           "floor_ratio_at_4096": FLOOR}
    at = [r for r in rows if r["n_bars"] == 4096]
    if at:
        res["ratio_at_4096"] = at[0]["ratio_to_sequential"]
        print(f"ratio at 4096 bars: {res['ratio_at_4096']:.1f}x (floor {FLOOR:g}x)")
    # one file for both pairings, keyed by the families: a run replaces its own key and keeps the other
    out = args.out or os.path.join(ROOT, "profiles", "ensemble_paper_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    both = {}
    if os.path.exists(out):
        with open(out) as fh:
            both = json.load(fh)
    both[families] = res
    with open(out, "w") as fh:
        json.dump(both, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": out, "ratio_at_4096": res.get("ratio_at_4096")}))
    if at and res["ratio_at_4096"] < FLOOR:
        sys.exit(f"paper ensemble below the {FLOOR:g}x floor at 4096 bars")


def exact_bench(args):
    from geometry import graded_bar
    from main import model_params
    from tvfem import ThermoViscoEnsemble

    mesh = graded_bar()
    n_nodes = mesh.num_vertices
    n_cells = n_nodes - 1
    span = (0.0, args.steps * 0.1)
    cfg = CFG_DG if args.dg else CFG
    families = "DG1/CG1" if args.dg else "CG1/CG1"
    hot = dict(model_params, T_0=EXACT_T_0)

    def make(relaxation):
        def ensemble(n_bars):
            ens = ThermoViscoEnsemble(mesh, span, 0.1, cfg, dict(hot, htc=np.linspace(50.0, 1000.0, n_bars)),
                                      model_mode="paper", relaxation=relaxation)
            ens.setup()
            return ens
        return ensemble

    # a last look at the state the timed kernel leaves: finite in exact mode at this T_0
    probe = make("exact")(64)
    probe.solve(args.steps)
    sigma = probe.get_field("sigma")
    probe.close()
    if not np.all(np.isfinite(sigma)):
        sys.exit("exact relaxation: sigma is not finite")
    ex = _time_ensembles(make("exact"), args.sizes, args.steps, args.reps)
    ta = _time_ensembles(make("taylor"), args.sizes, args.steps, args.reps)
    rows = []
    for e, t in zip(ex, ta):
        bar_steps = e["n_bars"] * args.steps
        its = e["newton_its_per_step"]
        if args.dg:  # the bytes of paper mode: the relaxation moves none
            per_bar_step = (n_cells * DG_BYTES_CELL_NEWTON * its + 2 * n_cells * PAPER_DG_BYTES_TDOF_STEP
                            + n_nodes * PAPER_DG_BYTES_NODE_STEP)
        else:
            per_bar_step = n_nodes * (BYTES_NODE_NEWTON * its + PAPER_BYTES_NODE_STEP)
        nbytes = bar_steps * per_bar_step
        row = dict(e, bar_steps_per_s=bar_steps / e["wall_s"], algorithmic_bytes=nbytes,
                   hbm_fraction_of_8TBps=nbytes / e["wall_s"] / HBM_PEAK,
                   taylor_ensemble=dict(t, bar_steps_per_s=bar_steps / t["wall_s"]),
                   exact_over_taylor_time=e["wall_s"] / t["wall_s"])
        rows.append(row)
        print(f"exact {families} ensemble {e['n_bars']:6d} bars: {e['wall_s'] * 1e3:9.2f} ms  "
              f"{row['bar_steps_per_s']:12.4g} bar-steps/s  {its:.2f} its/step  "
              f"{row['hbm_fraction_of_8TBps']:.2%} of HBM peak;  taylor {t['wall_s'] * 1e3:9.2f} ms  "
              f"time ratio {row['exact_over_taylor_time']:.3f}", flush=True)

    # the single-problem path has no exact mode: one Taylor paper-mode bar, at main.py's T_0 = 800 K so that it
    # stays finite over all the steps
    seq_wall, _ = _time_sequential(mesh, span, cfg, args.seq_bars, args.steps, model_mode="paper")
    seq_rate = args.seq_bars * args.steps / seq_wall
    print(f"sequential {args.seq_bars} paper-mode {families} bar(s) at T_0 = {model_params['T_0']:g} K: "
          f"{seq_wall:.3f} s  {seq_rate:.4g} bar-steps/s", flush=True)
    for r in rows:
        r["ratio_to_sequential"] = r["bar_steps_per_s"] / seq_rate
    res = {"workload": {"mesh": "geometry.graded_bar", "n_nodes": n_nodes, "n_cells": n_cells, "steps": args.steps,
                        "dt": 0.1, "htc": "linspace(50, 1000, n_bars)", "T_0": EXACT_T_0, "families": families,
                        "model_mode": "paper", "relaxation": "exact", "reps": args.reps,
                        "taylor_ensemble": "the same ensemble with relaxation=taylor, same process; at this T_0 its "
                                           "stress overflows (the thermal problem and the Newton counts are the "
                                           "same), so only its time is used",
                        "sigma_abs_max_exact_64_bars": float(np.abs(sigma).max())},
           "bytes_model": "paper mode's (tools/ensemble_bench.py --paper): the relaxation moves no byte",
           "kernel": EXACT_DG_KERNEL_RECORD if args.dg else EXACT_KERNEL_RECORD, "ensemble": rows,
           "sequential": {"bars": args.seq_bars, "wall_s": seq_wall, "bar_steps_per_s": seq_rate,
                          "T_0": model_params["T_0"],
                          "timed": f"ThermoViscoProblem {families} model_mode=paper (Taylor; no exact mode exists "
                                   f"there) at T_0 = {model_params['T_0']:g} K, inside the Taylor limit, all "
                                   f"{args.steps} steps: solve() and a final field read per bar; context creation "
                                   "and setup left out"},
           "floor_ratio_at_4096": FLOOR}
    at = [r for r in rows if r["n_bars"] == 4096]
    if at:
        res["ratio_at_4096"] = at[0]["ratio_to_sequential"]
        print(f"ratio at 4096 bars: {res['ratio_at_4096']:.1f}x (floor {FLOOR:g}x)")
    # one file for both pairings, keyed by the families: a run replaces its own key and keeps the other
    out = args.out or os.path.join(ROOT, "profiles", "ensemble_exact_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    both = {}
    if os.path.exists(out):
        with open(out) as fh:
            both = json.load(fh)
    both[families] = res
    with open(out, "w") as fh:
        json.dump(both, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": out, "ratio_at_4096": res.get("ratio_at_4096")}))
    if at and res["ratio_at_4096"] < FLOOR:
        sys.exit(f"exact ensemble below the {FLOOR:g}x floor at 4096 bars")


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
                         "paper-mode ensemble and one sequential paper-mode bar")
    args = ap.parse_args()
    if args.seq_bars is None:
        args.seq_bars = 1 if args.paper or args.exact else 4
    if args.exact:
        return exact_bench(args)
    if args.paper:
        return paper_bench(args)
    if args.scheduled:
        return scheduled_bench(args)
    if args.dg:
        return dg_bench(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "ensemble_bench.json")

    from geometry import graded_bar
    from main import model_params
    from tvfem import ThermoViscoEnsemble

    mesh = graded_bar()
    n_nodes = mesh.num_vertices
    span = (0.0, args.steps * 0.1)

    def ensemble(n_bars):
        ens = ThermoViscoEnsemble(mesh, span, 0.1, CFG, dict(model_params, htc=np.linspace(50.0, 1000.0, n_bars)))
        ens.setup()
        return ens

    rows = []
    for r in _time_ensembles(ensemble, args.sizes, args.steps, args.reps):
        n_bars, wall, its = r["n_bars"], r["wall_s"], r["newton_its_per_step"]
        bar_steps = n_bars * args.steps
        nbytes = bar_steps * n_nodes * (BYTES_NODE_NEWTON * its + BYTES_NODE_STEP)
        rows.append({"n_bars": n_bars, "wall_s": wall, "wall_s_min": r["wall_s_min"], "wall_s_max": r["wall_s_max"],
                     "bar_steps_per_s": bar_steps / wall, "newton_its_per_step": its,
                     "algorithmic_bytes": nbytes, "hbm_fraction_of_8TBps": nbytes / wall / HBM_PEAK})
        print(f"ensemble {n_bars:6d} bars: {wall * 1e3:9.2f} ms  {bar_steps / wall:12.4g} bar-steps/s  "
              f"{its:.2f} Newton its/step  {nbytes / wall / HBM_PEAK:.2%} of HBM peak", flush=True)

    # the same work one bar after another (what a parameter study costs without the ensemble)
    seq_wall, seq_total = _time_sequential(mesh, span, CFG, args.seq_bars, args.steps)
    seq_rate = args.seq_bars * args.steps / seq_wall  # the time loops alone: context creation left out
    print(f"sequential {args.seq_bars} bars: {seq_wall:.3f} s  {seq_rate:.4g} bar-steps/s", flush=True)
    for r in rows:
        r["ratio_to_sequential"] = r["bar_steps_per_s"] / seq_rate
    res = {"workload": {"mesh": "geometry.graded_bar", "n_nodes": n_nodes, "steps": args.steps, "dt": 0.1,
                        "htc": "linspace(50, 1000, n_bars)", "families": "CG1/CG1", "reps": args.reps},
           "bytes_model": {"per_node_newton_iteration": BYTES_NODE_NEWTON, "per_node_step": BYTES_NODE_STEP},
           "ensemble": rows,
           "sequential": {"bars": args.seq_bars, "wall_s": seq_wall, "bar_steps_per_s": seq_rate,
                          "wall_s_with_context_creation": seq_total,
                          "timed": "solve() and a final field read per bar; context creation and setup left out"},
           "floor_ratio_at_4096": FLOOR}
    at = [r for r in rows if r["n_bars"] == 4096]
    if at:
        res["ratio_at_4096"] = at[0]["ratio_to_sequential"]
        print(f"ratio at 4096 bars: {res['ratio_at_4096']:.1f}x (floor {FLOOR:g}x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": args.out, "ratio_at_4096": res.get("ratio_at_4096")}))
    if at and res["ratio_at_4096"] < FLOOR:
        sys.exit(f"ensemble below the {FLOOR:g}x floor at 4096 bars")


if __name__ == "__main__":
    main()
