"""What the tests of ThermoViscoProblem's process schedules and run histories share
(tests/test_problem_schedule.py, tests/test_guard_bands_history.py,
tests/schedule_part_check.py).  A support module (pytest does not collect it).

The schedule of every case: a strong quench over steps 1-3, an empty stage that
also ends at step 3 (its values, far from the others, must never be used), and
a reheating / after-cooling stage from step 4 on.
"""
import warnings

import numpy as np
import pytest

from oracle import tv_oracle as O

CG = {"element": "CG", "degree": 1}
DG = {"element": "DG", "degree": 1}
N_STEPS = 8

QUENCH = dict(htc=900.0, T_ambient=293.0, epsilon=0.93)
EMPTY = dict(htc=5000.0, T_ambient=1000.0, epsilon=0.1)
AFTER = dict(htc=60.0, T_ambient=350.0, epsilon=0.5)
SCHEDULE = [dict(until_step=3, **QUENCH), dict(until=0.3, **EMPTY), dict(AFTER)]  # dt = 0.1: until 0.3 = step 3


def stage_of(step):
    """the values in force during the 1-based step"""
    return QUENCH if step <= 3 else AFTER


def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def oracle_under_schedule(ref, n_steps=N_STEPS):
    """The oracle's steps with its thermal parameters set to the step's stage before each
    one: T after every step, the last step's |dT| masks, phi, Tf, xi, sigma, the counts."""
    ref.setup()
    Ts = []
    for s in range(1, n_steps + 1):
        st = stage_of(s)
        ref.tp.htc, ref.tp.T_ambient, ref.tp.epsilon = st["htc"], st["T_ambient"], st["epsilon"]
        T_before = ref.functions_current["T"].copy()
        ref.solve_timestep()
        Ts.append(ref.functions_current["T"].copy())
    mT = np.abs(Ts[-1] - T_before) > 1e-6
    return {"T": Ts, "mT": mT, "mS": mT[ref._maps[("S", "T")]], "phi": ref.functions["phi"].copy(),
            "Tf": ref.functions_current["Tf"].copy(), "xi": ref.functions["xi"].copy(),
            "sigma": ref.functions_next["sigma"].copy(), "history": list(ref.newton_history)}


def box_problem(axes, tf, sf, mp=None, **kw):
    from tvfem import RectilinearMesh
    from tvfem.problem import ThermoViscoProblem
    return ThermoViscoProblem(RectilinearMesh(axes), (0.0, 1.0), 0.1, {"T": tf, "sigma": sf},
                              dict(O.MAIN_MODEL_PARAMS if mp is None else mp),
                              part_axis=len(axes) - 1 if len(axes) == 3 else -1, verbose=False, **kw)


def advance(p, n, its=None):
    """n steps as ThermoViscoProblem.solve takes them, keeping each step's (Newton, Krylov) counts"""
    for _ in range(n):
        p.t += p.dt
        p.solve_timestep(t=p.t)
        if its is not None:
            its.append((p.last_newton_iterations, p.last_krylov_iterations))


def all_fields(p):
    from tvfem._native import FIELDS, NativeError
    out = {}
    for f in FIELDS:
        try:
            out[f] = np.array(p.get_field(f))
        except NativeError:  # not materialised
            pass
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_extremum(got, want):
    """bitwise equal, or both NaN (an all-NaN stream: a NaN's payload is not a value; the library's is the
    all-ones pattern its buffers are opened with, numpy's the quiet NaN of its input)"""
    return same_bits(got, want) or bool(np.isnan(got) and np.isnan(want))


def nan_extrema(v):
    """(np.nanmin, np.nanmax) of a 1D array, NaN for an all-NaN one.  numpy's fmin / fmax leave
    open which zero they return when the extremum is 0 and both signs occur; the library fixes
    -0 < +0, so the expected zero is the one that order gives (no other value has two encodings)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "All-NaN slice"
        mn, mx = np.nanmin(v), np.nanmax(v)
    if mn == 0.0:
        mn = -0.0 if np.any((v == 0.0) & np.signbit(v)) else 0.0
    if mx == 0.0:
        mx = 0.0 if np.any((v == 0.0) & ~np.signbit(v)) else -0.0
    return mn, mx


def check_record(h, r, T, Tf, sigma, dofs, bs):
    """record r of get_history() against the fields (get_field layout) read at its step: bitwise"""
    dT, dS = dofs["T"], dofs["sigma"]
    sig = sigma.reshape(-1, bs)
    assert same_bits(h["T"][r], T[dT]), ("T", r)
    assert same_bits(h["Tf"][r], Tf[dT]), ("Tf", r)
    assert same_bits(h["sigma"][r], sig[dS]), ("sigma", r)
    mn, mx = nan_extrema(T)
    assert same_extremum(h["T_min"][r], mn) and same_extremum(h["T_max"][r], mx), ("T extrema", r, h["T_min"][r], mn)
    for q in range(bs):
        mn, mx = nan_extrema(sig[:, q])
        assert same_extremum(h["sigma_min"][r, q], mn), ("sigma_min", r, q, h["sigma_min"][r, q], mn)
        assert same_extremum(h["sigma_max"][r, q], mx), ("sigma_max", r, q, h["sigma_max"][r, q], mx)


# the history cases: probes at two corners, a face centre, an interior point and a duplicate
AXES_3D = [np.linspace(0.0, 2.0, 9), np.linspace(0.0, 2.0, 7), np.linspace(0.0, 1.0, 5)]
AXES_2D = [np.linspace(0.0, 3.0, 13), np.linspace(0.0, 1.0, 5)]
HISTORY_CASES = {
    "3d_cg": (AXES_3D, CG, CG, [[0, 0, 0], [2, 2, 1], [1, 1, 0], [1.0, 1.0, 0.5], [0, 0, 0]]),
    "2d_dg_cg": (AXES_2D, DG, CG, [[0, 0], [3, 1], [1.5, 0], [1.5, 0.5], [0, 0]]),
}


def history_case(name, record=True, steps=6, **kw):
    """The case stepped `steps` times under SCHEDULE.  record: with history every 2, returning
    (history, history_dofs, its); else the twin, read by get_field every two steps:
    ([(T, Tf, sigma), ...], its)."""
    axes, tf, sf, points = HISTORY_CASES[name]
    its = []
    if record:
        p = box_problem(axes, tf, sf, schedule=SCHEDULE, history=dict(points=points, every=2), **kw)
        p.setup()
        advance(p, steps, its)
        out = (p.get_history(), p.history_dofs, its)
    else:
        p = box_problem(axes, tf, sf, schedule=SCHEDULE, **kw)
        p.setup()
        reads = []
        for _ in range(steps // 2):
            advance(p, 2, its)
            reads.append(tuple(np.array(p.get_field(f)) for f in ("T", "Tf", "sigma")))
        out = (reads, its)
    lib = p._lib
    return p, lib, out
