"""Process schedules (tv_set_boundary, tv_set_schedule) and on-device run histories
(tv_history_open / _read, csrc/tv_history.hip) of ThermoViscoProblem on the GPU.

1. parity with the CPU oracle under a three-stage schedule (one stage empty), the oracle's
   thermal parameters set to the step's stage before each step: the tolerances, check_field
   calls and check_counts of tests/test_gpu_parity.py::test_time_steps_match_oracle, and for the
   general meshes those of tests/test_unstructured.py / test_unstructured_dg.py.  The oracle
   alone under this schedule leaves every dof of the 3D cases above |dT| = 1e-6 in the last step
   (fraction 1.0 against the cap 0.9; the 1D / 2D cases have no cap in those files);
2. the multigrid levels see the change;
3. bitwise contracts; 4. histories; 5. capacity and failure; 6. partitions.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tv_oracle as O
from parity_util import check_field, relerr
from problem_schedule_cases import (AFTER, AXES_2D, AXES_3D, CG, DG, HISTORY_CASES, N_STEPS, QUENCH, SCHEDULE, advance,
                                    all_fields, box_problem, check_record, gpu, history_case, nan_extrema,
                                    oracle_under_schedule, same_bits, same_extremum)
from test_gpu_parity import AXES, check_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- 1. parity with the oracle -------------------------------------------------------------------
BOX_CASES = {
    "1d_graded_cg": (AXES["1d_graded"], CG, CG),
    "1d_graded_dg_cg": (AXES["1d_graded"], DG, CG),
    "2d_cg": (AXES["2d"], CG, CG),
    "3d_cg": (AXES["3d"], CG, CG),
    "3d_dg": (AXES["3d"], DG, DG),
}


@functools.lru_cache(maxsize=None)
def box_oracle(name):
    axes, tf, sf = BOX_CASES[name]
    return oracle_under_schedule(O.OracleProblem(O.rectilinear_mesh(axes), (0.0, 1.0), 0.1, {"T": tf, "sigma": sf},
                                                 dict(O.MAIN_MODEL_PARAMS), linear="pcg"))


@functools.lru_cache(maxsize=None)
def jacobi_run(name):
    """the scheduled device run of a box case: T after every step and the counts"""
    axes, tf, sf = BOX_CASES[name]
    dev = box_problem(axes, tf, sf, schedule=SCHEDULE)
    dev.setup()
    Ts, its = [], []
    for _ in range(N_STEPS):
        advance(dev, 1, its)
        Ts.append(np.array(dev.functions_current["T"].x.array))
    out = {"T": Ts, "its": its, "phi": np.array(dev.functions["phi"].x.array),
           "Tf": np.array(dev.functions_current["Tf"].x.array), "xi": np.array(dev.functions["xi"].x.array),
           "sigma": np.array(dev.functions_next["sigma"].x.array), "dim": dev.dim,
           "model": (dev.physical_model.htc, dev.physical_model.T_ambient, dev.physical_model.epsilon)}
    dev.close()
    return out


@pytest.mark.parametrize("name", list(BOX_CASES))
def test_scheduled_steps_match_oracle(name):
    gpu()
    want, got = box_oracle(name), jacobi_run(name)
    for s in range(N_STEPS):
        eT = relerr(got["T"][s], want["T"][s])
        assert eT < 1e-10, (s, eT)
    check_counts(got["its"], want["history"])
    d2 = got["dim"] ** 2
    assert relerr(got["phi"], want["phi"]) < 1e-9
    assert relerr(got["Tf"], want["Tf"]) < 1e-10
    min_frac = 0.9 if got["dim"] == 3 else None
    check_field("xi", got["xi"], want["xi"], want["mT"], 1, min_frac=min_frac)
    check_field("sigma", got["sigma"], want["sigma"], want["mS"], d2, min_frac=min_frac)
    assert got["its"][-1][0] >= 2
    assert got["model"] == (AFTER["htc"], AFTER["T_ambient"], AFTER["epsilon"])  # physical_model follows the stage


@functools.lru_cache(maxsize=None)
def general_mesh():
    from tvfem import distorted_box_mesh
    return distorted_box_mesh([2, 1.5, 1], [4, 3, 2])


@pytest.mark.parametrize("fT", ["CG", "DG"])
def test_scheduled_steps_match_oracle_general_mesh(fT):
    gpu()
    from tvfem.problem import ThermoViscoProblem
    m = general_mesh()
    cfg = {"T": CG if fT == "CG" else DG, "sigma": CG}
    want = oracle_under_schedule(O.OracleProblem(O.Mesh(dim=m.dim, x=m.x[:, :m.dim].copy(), cells=m.cells.copy()),
                                                 (0.0, 1.0), 0.1, cfg, dict(O.MAIN_MODEL_PARAMS), linear="pcg"))
    dev = ThermoViscoProblem(m, (0.0, 1.0), 0.1, cfg, dict(O.MAIN_MODEL_PARAMS), verbose=False, schedule=SCHEDULE)
    dev.setup()
    its, errs = [], []
    for s in range(N_STEPS):
        advance(dev, 1, its)
        errs.append(relerr(dev.functions_current["T"].x.array, want["T"][s]))
    eTf = relerr(dev.functions_current["Tf"].x.array, want["Tf"])
    sigma = np.array(dev.functions_next["sigma"].x.array)
    dev.close()
    print(f"[schedule] general mesh {fT}/CG: T per step {['%.1e' % e for e in errs]}, Tf {eTf:.1e}, {its}")
    assert max(errs) < 1e-10, errs
    for (n_d, k_d), (n_r, k_r) in zip(its, want["history"]):
        assert n_d == n_r, (its, want["history"])
        assert abs(k_d - k_r) <= max(n_r, int(np.ceil(0.05 * k_r))), (its, want["history"])
    assert eTf < 1e-10
    check_field(f"sigma[general,{fT}/CG]", sigma, want["sigma"], want["mS"], 9, min_frac=0.9)


# ---- 2. multigrid levels see the change ----------------------------------------------------------
def test_gmg_levels_follow_the_schedule():
    """The smallest box of tests/test_multigrid.py's cases ("graded": 16 x 16 x 7 cells, a coarse
    level below the fine grid): the scheduled GMG run against the scheduled Jacobi run, T after
    every step within that file's 1e-10, equal Newton counts (the Krylov counts are printed)."""
    gpu()
    axes = [np.concatenate([np.linspace(0.0, 0.5, 9), np.linspace(0.5, 2.5, 9)[1:]]),
            np.linspace(0.0, 2.0, 17), np.linspace(0.0, 0.75, 8)]
    runs = {}
    for pc in ("jacobi", "gmg"):
        p = box_problem(axes, CG, CG, schedule=SCHEDULE, preconditioner=pc)
        p.setup()
        Ts, its = [], []
        for _ in range(N_STEPS):
            advance(p, 1, its)
            Ts.append(np.array(p.get_field("T")))
        p.close()
        runs[pc] = (Ts, its)
    for s in range(N_STEPS):
        assert relerr(runs["gmg"][0][s], runs["jacobi"][0][s]) < 1e-10, s
    assert [n for n, _ in runs["gmg"][1]] == [n for n, _ in runs["jacobi"][1]], runs
    kg, kj = sum(k for _, k in runs["gmg"][1]), sum(k for _, k in runs["jacobi"][1])
    print(f"[schedule] gmg Krylov {kg}, Jacobi {kj}")


# ---- 3. bitwise contracts ------------------------------------------------------------------------
BITWISE_CASES = {"2d_dg_cg": (AXES["2d"], DG, CG), "3d_cg": (AXES["3d"], CG, CG)}


def _run(case, parts, manual=None, **kw):
    """fields, per-step counts and (with a history) the records after the steps in `parts`, taken
    in that many calls with reads in between; manual: {step before which: set_boundary kwargs}"""
    axes, tf, sf = BITWISE_CASES[case]
    p = box_problem(axes, tf, sf, **kw)
    p.setup()
    its = []
    done = 0
    for n in parts:
        if manual and done in manual:
            p.set_boundary(**manual[done])
        advance(p, n, its)
        done += n
        p.get_field("T")  # a host read between the calls
        if kw.get("history"):
            p.get_history()
    out = (all_fields(p), its, p.get_history() if kw.get("history") else None)
    p.close()
    return out


def _assert_same(a, b):
    assert a[1] == b[1], (a[1], b[1])
    assert a[0].keys() == b[0].keys()
    for k in a[0]:
        assert same_bits(a[0][k], b[0][k]), k


@pytest.mark.parametrize("case", list(BITWISE_CASES))
def test_schedule_of_creation_values_is_no_schedule(case):
    gpu()
    mp = O.MAIN_MODEL_PARAMS
    own = dict(htc=mp["htc"], T_ambient=mp["T_ambient"], epsilon=mp["epsilon"])
    plain = _run(case, [4])
    same = _run(case, [4], schedule=[dict(until_step=2, **own), dict(until_step=2, **QUENCH), dict()])
    _assert_same(plain, same)


@pytest.mark.parametrize("case", list(BITWISE_CASES))
def test_schedule_equals_set_boundary_and_does_not_depend_on_the_split(case):
    gpu()
    hist = dict(dofs=[0, 3], every=1)
    whole = _run(case, [8], schedule=SCHEDULE, history=hist)
    split = _run(case, [3, 5], schedule=SCHEDULE, history=hist)
    _assert_same(whole, split)
    for k in whole[2]:
        assert same_bits(whole[2][k], split[2][k]), k
    assert whole[2]["step"].tolist() == list(range(1, 9))
    manual = _run(case, [3, 5], manual={0: QUENCH, 3: AFTER})
    _assert_same(whole, manual)
    # and the schedule did change the run
    plain = _run(case, [8])
    assert not same_bits(plain[0]["T"], whole[0]["T"])


def test_set_boundary_keeps_missing_values_and_refuses_bad_ones():
    gpu()
    from tvfem._native import NativeError, TV_ERR_ARG
    p = box_problem(AXES["2d"], CG, CG)
    p.setup()
    p.set_boundary(htc=900.0)
    pm = p.physical_model
    assert (pm.htc, pm.T_ambient, pm.epsilon) == (900.0, O.MAIN_MODEL_PARAMS["T_ambient"], O.MAIN_MODEL_PARAMS["epsilon"])
    for bad in (dict(htc=-1.0), dict(epsilon=-0.5), dict(T_ambient=float("nan")), dict(htc=float("inf"))):
        with pytest.raises(NativeError) as e:
            p.set_boundary(**bad)
        assert e.value.code == TV_ERR_ARG
    assert (pm.htc, pm.T_ambient, pm.epsilon) == (900.0, O.MAIN_MODEL_PARAMS["T_ambient"], O.MAIN_MODEL_PARAMS["epsilon"])
    p.close()


# ---- 4. histories --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HISTORY_CASES))
def test_history_records_equal_a_twin_read_every_two_steps(name):
    gpu()
    p, _, (h, dofs, its) = history_case(name)
    # the probes: the nearest dof of each space, the lowest index among ties
    pts = np.zeros((5, 3))
    raw = np.asarray(HISTORY_CASES[name][3], dtype=float)
    pts[:, :raw.shape[1]] = raw
    for space, key in ((0, "T"), (1, "sigma")):
        X = p._dof_coordinates(space)
        d2 = ((X[None] - pts[:, None]) ** 2).sum(axis=2)
        assert dofs[key].tolist() == [int(np.flatnonzero(row == row.min())[0]) for row in d2], key
    assert dofs["T"][0] == dofs["T"][4] and dofs["sigma"][0] == dofs["sigma"][4]  # the duplicate
    bs = p.dim ** 2
    p.close()
    q, _, (reads, its_twin) = history_case(name, record=False)
    q.close()
    assert its == its_twin
    assert h["step"].tolist() == [2, 4, 6] and np.allclose(h["t"], [0.2, 0.4, 0.6])
    assert h["T"].shape == (3, 5) and h["sigma"].shape == (3, 5, bs) and h["sigma_min"].shape == (3, bs)
    for r, (T, Tf, sigma) in enumerate(reads):
        check_record(h, r, T, Tf, sigma, dofs, bs)


def test_history_extrema_positions_and_a_grid_larger_than_one_pass():
    """Planted sigma, recorded by thermal-only steps (which record what the state holds).  449 x 449
    CG nodes = 201,601 dofs: the extrema pass runs its cap of kHistBlocks = 192 workgroups of 256
    threads per stream with 4 values per thread and trip, so one pass of the grid covers
    192 x 256 x 4 = 196,608 dofs and the rest is taken by the loop's tail.  Extrema at the first
    and the last dof, on both sides of a workgroup boundary (255 | 256), on both sides of the
    pass boundary (196,607 | 196,608), in the last component; NaNs, and one component all NaN."""
    gpu()
    n1 = 449
    axes = [np.linspace(0.0, 4.0, n1), np.linspace(0.0, 4.0, n1)]
    p = box_problem(axes, CG, CG, materialize=False, history=dict(dofs=[0, n1 * n1 - 1], every=1, max_records=2))
    p.setup()
    n = n1 * n1
    assert n > 192 * 256 * 4
    rng = np.random.default_rng(3)
    sig = rng.uniform(-1.0, 1.0, (n, 4))
    sig[rng.integers(0, n, 500), 0] = np.nan
    sig[0, 0], sig[n - 1, 0] = -5.0, 7.0           # first / last dof
    sig[255, 1], sig[256, 1] = -6.0, 8.0           # a workgroup boundary
    sig[:, 2] = np.nan                             # all NaN
    sig[rng.integers(0, n, 500), 3] = np.nan
    sig[196607, 3], sig[196608, 3] = 9.0, -9.5     # the pass boundary, last component
    p.set_field("sigma", sig)
    p.solve_timestep(thermal_only=True)
    sig2 = sig.copy()
    sig2[0, 0], sig2[n - 1, 0] = 7.5, -5.5         # the other way round
    sig2[255, 1], sig2[256, 1] = 8.5, -6.5
    sig2[:, 3] = -np.abs(sig[:, 3])                # (NaNs stay) all negative but two zeros:
    sig2[196607, 3], sig2[196608, 3] = -0.0, 0.0   # the maximum is a zero, and +0 must win
    p.set_field("sigma", sig2)
    p.solve_timestep(thermal_only=True)
    h = p.get_history()
    T, Tf = p.get_field("T"), p.get_field("Tf")
    assert same_bits(p.get_field("sigma"), sig2.reshape(-1))  # a thermal-only step leaves sigma alone
    check_record(h, 1, T, Tf, sig2.reshape(-1), p.history_dofs, 4)
    for r, s in enumerate((sig, sig2)):
        for q in range(4):
            mn, mx = nan_extrema(s[:, q])
            assert same_extremum(h["sigma_min"][r, q], mn) and same_extremum(h["sigma_max"][r, q], mx), (r, q)
    assert h["sigma_min"][0].tolist()[:2] == [-5.0, -6.0] and h["sigma_max"][0].tolist()[:2] == [7.0, 8.0]
    assert np.isnan(h["sigma_min"][:, 2]).all() and np.isnan(h["sigma_max"][:, 2]).all()
    assert (h["sigma_min"][0, 3], h["sigma_max"][0, 3]) == (-9.5, 9.0)
    assert h["sigma_max"][1, 3] == 0.0 and not np.signbit(h["sigma_max"][1, 3])
    p.close()


@pytest.mark.parametrize("tf", ["CG", "DG"])
def test_history_on_a_mesh_smaller_than_a_wave(tf):
    """1D, 2 cells: 3 CG dofs / 4 DG dofs, one partly filled wave per stream"""
    gpu()
    p = box_problem([np.linspace(0.0, 50.0, 3)], CG if tf == "CG" else DG, CG, schedule=SCHEDULE,
                    history=dict(points=[[0.0], [50.0], [25.0]], every=1))
    p.setup()
    reads = []
    for _ in range(3):
        advance(p, 1)
        reads.append(tuple(np.array(p.get_field(f)) for f in ("T", "Tf", "sigma")))
    h = p.get_history()
    assert h["T"].shape == (3, 3)
    for r, (T, Tf, sigma) in enumerate(reads):
        check_record(h, r, T, Tf, sigma, p.history_dofs, 1)
    p.close()


def test_history_of_a_paper_exact_run_is_finite():
    gpu()
    axes, tf, sf, points = HISTORY_CASES["3d_cg"]
    p = box_problem(axes, tf, sf, mp=dict(O.MAIN_MODEL_PARAMS, T_0=920.0), model_mode="paper", relaxation="exact",
                    schedule=SCHEDULE, history=dict(points=points, every=2))
    p.setup()
    advance(p, 4)
    h = p.get_history()
    assert h["step"].tolist() == [2, 4]
    for k in ("T", "Tf", "sigma", "T_min", "T_max", "sigma_min", "sigma_max"):
        assert np.all(np.isfinite(h[k])), k
    check_record(h, 1, p.get_field("T"), p.get_field("Tf"), p.get_field("sigma"), p.history_dofs, 9)
    assert np.abs(h["sigma"]).max() > 0.0
    p.close()


def test_history_open_refuses_out_of_range_dofs_and_reopens():
    gpu()
    from tvfem._native import NativeError, TV_ERR_ARG, TV_ERR_STATE
    p = box_problem(AXES_2D, DG, CG, history=dict(dofs=dict(T=[0, 4 * 12 * 4], sigma=[0, 1])))
    with pytest.raises(NativeError) as e:  # T dofs: [0, 192)
        p.setup()
    assert e.value.code == TV_ERR_ARG and "T dof 192" in str(e.value)
    p.close()
    p = box_problem(AXES_2D, DG, CG, history=dict(dofs=dict(T=[0, 191], sigma=[0, 13 * 5])))
    with pytest.raises(NativeError) as e:  # sigma dofs: [0, 65)
        p.setup()
    assert e.value.code == TV_ERR_ARG and "sigma dof 65" in str(e.value)
    # no history is open on this context: reading is a state error; n_probes == 0 is accepted
    assert p._lib.tv_history_read(p._ctx, None, 0, C.byref(C.c_int())) == TV_ERR_STATE
    assert p._lib.tv_history_open(p._ctx, 0, None, None, 1, 1) == 0
    p.close()


# ---- 5. capacity and failure ---------------------------------------------------------------------
def test_step_past_the_capacity_is_refused_before_anything_runs():
    gpu()
    from tvfem._native import NativeError, TV_ERR_STATE
    p = box_problem(AXES_3D, CG, CG, schedule=SCHEDULE, history=dict(dofs=[0], every=2, max_records=1))
    p.setup()
    advance(p, 2)
    assert p.step_count == 2
    before = all_fields(p)
    with pytest.raises(NativeError) as e:
        p.solve_timestep()
    assert e.value.code == TV_ERR_STATE and "max_records 1 x every 2" in str(e.value)
    assert p.step_count == 2
    after = all_fields(p)
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert p.get_history()["step"].tolist() == [2]
    # closing the history lifts the cap
    assert p._lib.tv_history_open(p._ctx, 0, None, None, 1, 1) == 0
    p.solve_timestep()
    assert p.step_count == 3
    p.setup()  # tv_set_initial_condition: the count restarts
    assert p.step_count == 0
    p.close()


def test_a_step_that_does_not_end_leaves_its_record_nan():
    """newton_max_it = 1 with error_on_nonconvergence off, as tests/test_solver_api.py makes a step
    fail: tv_step returns TV_OK without the step's end; the call is counted and its record stays NaN."""
    gpu()
    p = box_problem(AXES_3D, CG, CG, history=dict(dofs=[0, 5], every=1))
    p.setup()
    advance(p, 1)
    p.solver.max_it = 1
    p.solver.error_on_nonconvergence = False
    with pytest.raises(AssertionError):
        p.solve_timestep()
    assert p.step_count == 2
    p.solver.max_it = 50
    p.solver.error_on_nonconvergence = True
    advance(p, 1)
    h = p.get_history()
    assert h["step"].tolist() == [1, 2, 3]
    for k in ("T", "Tf", "sigma", "T_min", "T_max", "sigma_min", "sigma_max"):
        assert np.isnan(h[k][1]).all(), k
    assert np.isfinite(h["T"][[0, 2]]).all() and np.isfinite(h["T_min"][[0, 2]]).all()
    check_record(h, 2, p.get_field("T"), p.get_field("Tf"), p.get_field("sigma"), p.history_dofs, 9)
    p.close()


# ---- 6. partitions -------------------------------------------------------------------------------
def test_scheduled_partitioned_run_matches_single_partition():
    """tests/test_partition.py::test_partitioned_run_matches_single_partition's harness and
    criterion (world 2, host transport), the schedule handed to tests/schedule_part_check.py;
    each rank's recorded extrema are those of its own owned dofs."""
    gpu()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(29880 + os.getpid() % 50),
           os.path.join(ROOT, "tests", "schedule_part_check.py"), "--comm", "host", "--schedule", json.dumps(SCHEDULE)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("SCHEDULE_PART_CHECK ")]
    assert line, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(line[0].split(" ", 1)[1])
    print("[partition] " + json.dumps(res))
    assert res["T"] < 1e-12, res
    assert res["phi"] < 1e-11, res
    assert res["xi"] < 1e-6, res
    assert res["sigma"] < 1e-6, res
    for (n1, k1), (n2, k2) in zip(res["its_parts"], res["its_single"]):
        assert n1 == n2 and abs(k1 - k2) <= max(n1, 0.05 * k2), res
    assert res["schedule_changed_T"] > 1e-3, res       # the schedule was in force (against an unscheduled run)
    assert res["extrema_own"] == [True, True], res     # bitwise nanmin / nanmax of each rank's owned dofs
    assert res["records"] == [5, 5], res               # 4 steps and the one behind the planted hot spot
    assert res["ghosts_excluded"], res                 # rank 0's maximum stays below its ghost copy of the hot spot
