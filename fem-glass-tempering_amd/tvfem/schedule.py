"""Process schedules as ``ThermoViscoEnsemble`` and ``ThermoViscoProblem`` take
them: a list of stage dicts, each with ``htc`` / ``T_ambient`` / ``epsilon``
(any subset) and, on every stage but the last, exactly one of ``until`` (a
time on the step grid) or ``until_step``.  Step s (1-based) belongs to the
first stage whose end is not before it, so equal ends give an empty stage.

An ensemble's values may be per-bar arrays (``n`` bars); a single problem is
one bar (``n = 1``) and takes scalars only.  Everything here is host-side
validation, done before any native object exists.
"""
from __future__ import annotations

import numpy as np

# what a schedule stage may change, and how it says where it ends
STAGE_KEYS = ("htc", "T_ambient", "epsilon")
STAGE_ENDS = ("until", "until_step")


def parse_stages(schedule):
    """The stages as dicts of scalars / 1D arrays, their keys checked (the sizes
    and the step grid are checked once n_bars and the time span are known)."""
    stages = [dict(st) for st in schedule]
    if not stages:
        raise ValueError("schedule: at least one stage")
    for j, st in enumerate(stages):
        unknown = set(st) - set(STAGE_KEYS) - set(STAGE_ENDS)
        if unknown:
            raise ValueError(f"schedule stage {j}: unknown key(s) {sorted(unknown)} "
                             f"({', '.join(STAGE_ENDS + STAGE_KEYS)})")
        n_ends = sum(k in st for k in STAGE_ENDS)
        if j == len(stages) - 1 and n_ends:
            raise ValueError("schedule: the last stage never ends (no until / until_step)")
        if j < len(stages) - 1 and n_ends != 1:
            raise ValueError(f"schedule stage {j}: exactly one of until / until_step (only the last stage has none)")
        for key, val in st.items():
            if np.ndim(val) > 1:
                raise ValueError(f"schedule stage {j}: {key} is a scalar or one value per bar")
            if np.ndim(val) == 1:
                st[key] = np.asarray(val, dtype=np.float64)
    return stages


def stage_tables(stages, n_bars, time0, dt, own):
    """(stage_end [n_stages-1][n_bars] or None, {key: [n_stages][n_bars]}) of the parsed
    stages; ``own[key]`` is the value (scalar or per-bar array) a stage without the key keeps."""
    nb, nst = n_bars, len(stages)
    end = np.zeros((nst - 1, nb), dtype=np.intc) if nst > 1 else None
    for j, st in enumerate(stages[:-1]):
        if "until_step" in st:
            k = np.broadcast_to(np.asarray(st["until_step"]), (nb,))
            if not np.all(np.isfinite(k)) or np.any(k != np.round(k)):
                raise ValueError(f"schedule stage {j}: until_step must be whole steps")
        else:
            x = (np.broadcast_to(np.asarray(st["until"], dtype=np.float64), (nb,)) - time0) / dt
            k = np.round(x)
            off = ~(np.abs(x - k) <= 1e-6)  # also catches NaN
            if off.any():
                b = int(np.argmax(off))
                raise ValueError(f"schedule stage {j}: until of bar {b} is not on the step grid "
                                 f"(time[0] + k dt within 1e-6 dt)")
        if np.any(k < 0) or np.any(k > np.iinfo(np.intc).max):
            raise ValueError(f"schedule stage {j}: the stage ends before the start (or out of range) "
                             f"for bar {int(np.argmax((k < 0) | (k > np.iinfo(np.intc).max)))}")
        end[j] = k
        if j and np.any(end[j] < end[j - 1]):
            b = int(np.argmax(end[j] < end[j - 1]))
            raise ValueError(f"schedule: the stage ends of bar {b} decrease at stage {j} "
                             f"({int(end[j - 1][b])} then {int(end[j][b])})")
    tabs = {}
    for key in STAGE_KEYS:
        if not any(key in st for st in stages):
            continue  # NULL table: the creation value in every stage
        tab = np.empty((nst, nb))
        for j, st in enumerate(stages):
            tab[j] = st.get(key, own[key])  # a missing key takes the bar's model_parameters value
        if not np.all(np.isfinite(tab)):
            raise ValueError(f"schedule: {key} is not finite")
        tabs[key] = tab
    return end, tabs
