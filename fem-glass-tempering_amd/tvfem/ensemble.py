"""``ThermoViscoEnsemble`` — thousands of independent 1D tempering bars in one
launch (the ``tv_ensemble_*`` entry points of libtvfem.so).

A parameter study of the reference's own workload (main.py: one
through-thickness bar): every bar has the same cell count and may have its
own node coordinates (thickness, grading) and its own ``htc``, ``T_0``,
``T_ambient``, ``epsilon``, ``alpha`` and ``f``; ``dt`` and every other model
parameter are shared.  ``config`` is CG1 temperature with
CG1 stress, or DG1 temperature with CG1 stress (main.py's own ``fe_config``: SIPG
on the interior nodes, two T dofs per cell numbered ``2 c + l``).  With DG
temperature the T-family fields (T, T_prev, Tf, Tf_partial, phi, xi) have
``n_dofs_T = 2 n_cells`` dofs per bar and the stress fields ``n_dofs_sigma =
n_cells + 1``; history probes stay mesh nodes, T and Tf being recorded at the
node's source dof (``2 i``, and ``2 n_cells - 1`` for the last node) and sigma at
the node.

    ens = ThermoViscoEnsemble(mesh, (0.0, 50.0), 0.1, fe_config,
                              dict(model_params, htc=np.linspace(50, 1000, 4096)))
    ens.setup()
    ens.solve()
    sigma = ens.get_field("sigma")        # (n_bars, n_dofs_sigma)

A process schedule lets ``htc``, ``T_ambient`` and ``epsilon`` of each bar change
at times of its own (a quench of per-bar length, then after-cooling), and a
probe history has the kernel record T, Tf and sigma at a few nodes while it
runs, so that a transient is read without cutting the run into calls:

    ens = ThermoViscoEnsemble(mesh, (0.0, 50.0), 0.1, fe_config, model_params,
            schedule=[dict(until=np.linspace(2.0, 10.0, 4096).round(1), htc=900.0, T_ambient=293.0),
                      dict(htc=60.0)],                      # last stage: no end
            history=dict(nodes=[0, 24, 48], every=5))
    ens.setup(); ens.solve()
    h = ens.get_history()   # {"step": (R,), "t": (R,), "T" / "Tf" / "sigma": (R, n_bars, n_probes)}

Every stage but the last carries exactly one of ``until`` (a time, on the step
grid) or ``until_step``; step s (1-based) belongs to the first stage whose end
is not before it, so equal ends give an empty stage.  The other keys are scalars
or per-bar arrays; a missing key keeps the bar's ``model_parameters`` value.

``model_mode="reference"`` (the default) computes what the reference code
computes, quirks included.  ``model_mode="paper"`` runs the model as the paper
states it, for either config, as ``ThermoViscoProblem(model_mode="paper")``:
Eq. 25 (with Tf) drives Eq. 24 instead of being overwritten by Eq. 5 (Q1); the
structural strain ``(alpha_liquid - alpha_solid) (Tf - Tf_prev)`` is kept (Q2);
Eq. 16 feeds the stress memory from the previous partial stresses, so the
stress has a history (Q3); and ``xi = dt/2 (phi_next + phi)``, so sigma is
finite where T has not moved (Q4).  The thermal problem does not see the mode.
A paper ensemble has two more state fields on the stress space, ``s_partial``
and ``sigma_partial`` (block size 6, zero after ``setup()``); on a reference
ensemble ``get_field`` / ``set_field`` of them raise (TV_ERR_STATE).

Both modes keep the reference's degree-2 Taylor exponential ``E = 1 - x + x^2/2``,
``x = xi / lambda``, which exceeds 1 when ``xi > 2 lambda``.  In paper mode ``xi``
is no longer tiny and the stress memory is multiplied by ``E`` every step: with
main.py's parameters and dt = 0.1 (smallest ``lambda_k`` 5.0e-5) a bar at
``T_0 = 800 K`` stays inside the limit (``xi`` peaks at 7.0e-5) and is stable
over 500 steps, while at 873 K ``xi`` is about 0.2 and sigma passes 1e23 after
five steps and reaches +-inf within 100.  That is the model as the reference
states it, not a defect of the kernel; with ``relaxation="taylor"`` (the
default) a sweep over ``T_0`` must stay below the limit.  Such a bar harms no
other bar of the ensemble.

``model_mode="paper", relaxation="exact"`` replaces the polynomial in the two
places it enters the stress update: ``E = exp(-x)`` multiplies the stress memory
(Eq. 16) and ``1 - E = -expm1(-x)`` scales the increment (Eq. 15 + 20).  ``E``
lies in (0, 1], so the memory cannot grow and a sweep may start above ``Tb``
(all ten test bars, up to 920 K, stay finite over 500 steps with surface sigma
0.02-0.21).  It also keeps the digits of ``1 - E`` for small ``x``: the Taylor
form subtracts and is exactly 0 once ``x < 1e-16`` (below roughly 575-650 K), so
with it the cold, elastic part of a quench adds no stress and the residual
stress is low by tens of percent even inside the limit.  Nothing else changes:
T, Tf, phi, xi, the Newton counts, the failure contract, schedules, histories
and the state fields are those of a paper ensemble; only ``sigma`` and the four
partial-stress fields differ.  ``relaxation="exact"`` with
``model_mode="reference"`` raises ``ValueError``; ``ens.relaxation`` holds the
choice.  The single-problem path has the same switch:
``ThermoViscoProblem(..., model_mode="paper", relaxation="exact")``.
"""
from __future__ import annotations

import ctypes as C
from math import ceil

import numpy as np

from . import _native as N
from .mesh import RectilinearMesh
# the schedule grammar is shared with ThermoViscoProblem
from .schedule import STAGE_ENDS, STAGE_KEYS, parse_stages as _parse_stages, stage_tables  # noqa: F401

# model parameters that may differ from bar to bar
PER_BAR_KEYS = ("htc", "T_0", "T_ambient", "epsilon", "alpha", "f")
# the state an ensemble keeps (names as ThermoViscoProblem.get_field) and its block size per dof
# (s_partial and sigma_partial: paper ensembles only)
STATE_FIELDS = {"T": 1, "T_prev": 1, "Tf": 1, "Tf_partial": 6, "phi": 1, "xi": 1, "sigma": 1,
                "s_tilde_partial": 6, "sigma_tilde_partial": 6, "s_partial": 6, "sigma_partial": 6}
# the fields that live on the stress space (every other state field lives on the temperature space)
SIGMA_FAMILY = ("sigma", "s_tilde_partial", "sigma_tilde_partial", "s_partial", "sigma_partial")
_FAMILIES = {"CG": N.TV_CG, "DG": N.TV_DG}


class ThermoViscoEnsemble:
    def __init__(self, meshes, time: tuple, dt: float, config: dict, model_parameters: dict, *,
                 n_bars: int | None = None, device: int = 0, model_mode: str = "reference",
                 relaxation: str = "taylor", newton_rtol: float | None = None, newton_atol: float | None = None,
                 newton_max_it: int | None = None, error_on_nonconvergence: bool = True,
                 schedule=None, history: dict | None = None) -> None:
        self._ens = None
        # ---- meshes: one 1D RectilinearMesh for all bars, or one per bar
        shared = isinstance(meshes, RectilinearMesh)
        mlist = [meshes] if shared else list(meshes)
        if not mlist or not all(isinstance(m, RectilinearMesh) and m.dim == 1 for m in mlist):
            raise TypeError("meshes must be a 1D tvfem.RectilinearMesh or a sequence of them")
        counts = {m.n_cells[0] for m in mlist}
        if len(counts) != 1:
            raise ValueError(f"every bar of an ensemble has the same cell count, got {sorted(counts)}")
        self.n_cells = counts.pop()
        # ---- parameters: the six per-bar keys may be arrays, nothing else
        mp = dict(model_parameters)
        arrays = {}
        for key, val in mp.items():
            if np.ndim(val) == 0:
                continue
            if key not in PER_BAR_KEYS:
                raise ValueError(f"model parameter {key!r} is shared by the ensemble and must be a scalar "
                                 f"(per-bar arrays: {', '.join(PER_BAR_KEYS)})")
            arrays[key] = np.ascontiguousarray(val, dtype=np.float64).reshape(-1)
        stages = _parse_stages(schedule) if schedule is not None else None
        sizes = {len(v) for v in arrays.values()}
        if stages is not None:
            sizes |= {len(v) for st in stages for v in st.values() if np.ndim(v) == 1}
        if not shared:
            sizes.add(len(mlist))
        if n_bars is not None:
            sizes.add(int(n_bars))
        if len(sizes) > 1:
            raise ValueError(f"inconsistent ensemble sizes {sorted(sizes)} among meshes, n_bars and per-bar arrays")
        self.n_bars = sizes.pop() if sizes else 1
        if self.n_bars < 1:
            raise ValueError("an ensemble has at least one bar")
        if model_mode not in ("reference", "paper"):
            raise ValueError("model_mode must be 'reference' or 'paper'")
        if relaxation not in ("taylor", "exact"):
            raise ValueError("relaxation must be 'taylor' (the reference's degree-2 polynomial) or 'exact'")
        if relaxation == "exact" and model_mode != "paper":
            raise ValueError("relaxation='exact' needs model_mode='paper' (reference mode is the reference's "
                             "code, its Taylor exponential included)")
        self.relaxation = relaxation
        self.dt = dt
        self.time = time
        self.t = self.time[0]
        self.n_steps = ceil((self.time[1] - self.time[0]) / self.dt)
        self.config = config
        self.model_mode = model_mode
        # DG1 temperature with CG1 stress has its own kernel and constructor; every other pairing goes to
        # tv_ensemble_create, which accepts CG1 / CG1 and refuses the rest
        self._dg = (config["T"]["element"] == "DG" and int(config["T"]["degree"]) == 1
                    and config["sigma"]["element"] == "CG" and int(config["sigma"]["degree"]) == 1)
        self.n_dofs_T = 2 * self.n_cells if self._dg else self.n_cells + 1
        self.n_dofs_sigma = self.n_cells + 1
        self.n_dofs = self.n_dofs_T
        self.coords = np.ascontiguousarray(np.stack([m.axes[0] for m in mlist]))
        self._arrays = arrays
        # ---- process schedule and probe history: everything is decided before anything is created
        self._schedule = None if stages is None else self._stage_tables(stages, mp)
        self._history = None if history is None else self._history_args(history)
        # ---- native handle
        lib = N.load_library()
        self._lib = lib
        desc = N.EnsembleDesc()
        desc.n_bars = self.n_bars
        desc.n_cells = self.n_cells
        desc.coords = self.coords.ctypes.data_as(C.POINTER(C.c_double))
        desc.coords_shared = 1 if shared else 0
        for key, arr in arrays.items():
            setattr(desc, key, arr.ctypes.data_as(C.POINTER(C.c_double)))
            mp[key] = float(arr[0])  # tv_params keeps a scalar; the array overrides it
        fe = N.FeConfig(_FAMILIES[config["T"]["element"]], int(config["T"]["degree"]),
                        _FAMILIES[config["sigma"]["element"]], int(config["sigma"]["degree"]))
        params = N.default_params(mp, dt)
        opts = N.default_options()
        if model_mode == "paper":
            opts.model_mode = N.TV_MODEL_PAPER_EXACT if relaxation == "exact" else N.TV_MODEL_PAPER
        else:
            opts.model_mode = N.TV_MODEL_REFERENCE
        if newton_rtol is not None:
            opts.newton_rtol = newton_rtol
        if newton_atol is not None:
            opts.newton_atol = newton_atol
        if newton_max_it is not None:
            opts.newton_max_it = newton_max_it
        opts.error_on_nonconvergence = 1 if error_on_nonconvergence else 0
        ens = C.c_void_p()
        # paper mode has one constructor for both pairings (the family is read from fe)
        if model_mode == "paper":
            create = lib.tv_ensemble_create_paper
        else:
            create = lib.tv_ensemble_create_dg if self._dg else lib.tv_ensemble_create
        N.check(create(C.byref(desc), C.byref(fe), C.byref(params), C.byref(opts), device, C.byref(ens)))
        self._ens = ens
        try:
            if self._schedule is not None:
                end, tabs = self._schedule
                sch = N.EnsembleSchedule()
                sch.n_stages = len(stages)
                if end is not None:
                    sch.stage_end = end.ctypes.data_as(C.POINTER(C.c_int))
                for key, tab in tabs.items():
                    setattr(sch, key, tab.ctypes.data_as(C.POINTER(C.c_double)))
                N.check(lib.tv_ensemble_set_schedule(ens, C.byref(sch)), ens)
            if self._history is not None:
                nodes, every, max_records = self._history
                N.check(lib.tv_ensemble_history_open(ens, len(nodes), nodes.ctypes.data_as(C.POINTER(C.c_int)),
                                                     every, max_records), ens)
        except Exception:
            self.close()
            raise

    def _stage_tables(self, stages, mp):
        """(stage_end [n_stages-1][n_bars] or None, {key: [n_stages][n_bars]}) of the parsed stages."""
        own = {key: self._arrays.get(key, mp[key]) for key in STAGE_KEYS}
        return stage_tables(stages, self.n_bars, self.time[0], self.dt, own)

    def _history_args(self, history):
        unknown = set(history) - {"nodes", "every", "max_records"}
        if unknown:
            raise ValueError(f"history: unknown key(s) {sorted(unknown)} (nodes, every, max_records)")
        if "nodes" not in history:
            raise ValueError("history: nodes is required")
        nodes = np.atleast_1d(np.asarray(history["nodes"]))
        if nodes.ndim != 1 or nodes.size == 0 or np.any(nodes != np.round(nodes)):
            raise ValueError("history: nodes is a non-empty list of dof numbers")
        if np.any(nodes < 0) or np.any(nodes > self.n_cells):
            raise ValueError(f"history: probe node outside [0, n_cells = {self.n_cells}]")
        every = int(history.get("every", 1))
        if every < 1:
            raise ValueError("history: every must be at least 1")
        max_records = int(history.get("max_records", max(self.n_steps // every, 1)))
        if max_records < 1:
            raise ValueError("history: max_records must be at least 1")
        return np.ascontiguousarray(nodes, dtype=np.intc), every, max_records

    # ---- reference-style driver -----------------------------------------------------------
    def setup(self) -> None:
        """Initial condition: T = T_prev = Tf = Tf_partial = each bar's own T_0."""
        N.check(self._lib.tv_ensemble_set_initial_condition(self._ens), self._ens)

    def solve(self, n_steps: int | None = None, thermal_only: bool = False) -> None:
        """``n_steps`` (default: the whole time span) steps of every bar.  Raises
        ``NativeError`` (TV_ERR_NOT_CONVERGED) after the steps have run if a bar's
        Newton solve failed and ``error_on_nonconvergence`` is set; the failed
        bars are frozen, the others have advanced either way."""
        n = self.n_steps if n_steps is None else int(n_steps)
        rc = self._lib.tv_ensemble_step(self._ens, n, 1 if thermal_only else 0)
        if rc in (N.TV_OK, N.TV_ERR_NOT_CONVERGED):
            self.t += n * self.dt
        N.check(rc, self._ens)

    def solve_timestep(self, thermal_only: bool = False) -> None:
        self.solve(1, thermal_only=thermal_only)

    # ---- state ---------------------------------------------------------------------------
    def get_field(self, name: str) -> np.ndarray:
        """(n_bars, dofs * bs) array, per bar the reference's interleaved layout; dofs is
        ``n_dofs_sigma`` for the stress fields and ``n_dofs_T`` for the others."""
        dofs = self.n_dofs_sigma if name in SIGMA_FAMILY else self.n_dofs_T
        out = np.empty((self.n_bars, dofs * STATE_FIELDS.get(name, 1)))
        N.check(self._lib.tv_ensemble_get_field(self._ens, N.FIELD_ID[name],
                                                out.ctypes.data_as(C.POINTER(C.c_double)), out.size), self._ens)
        return out

    def set_field(self, name: str, values) -> None:
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        N.check(self._lib.tv_ensemble_set_field(self._ens, N.FIELD_ID[name],
                                                v.ctypes.data_as(C.POINTER(C.c_double)), v.size), self._ens)

    def get_history(self) -> dict:
        """The probe records so far: ``step`` and ``t`` of shape (R,), ``T``, ``Tf`` and
        ``sigma`` of shape (R, n_bars, n_probes); record r is the state after step
        (r + 1) * every.  NaN where a bar had failed or the history was not yet open."""
        if self._history is None:
            raise ValueError("the ensemble was created without history=")
        nodes, every, _ = self._history
        n_rec = C.c_int(0)
        N.check(self._lib.tv_ensemble_history_read(self._ens, None, 0, C.byref(n_rec)), self._ens)
        out = np.empty((n_rec.value, 3, self.n_bars, len(nodes)))
        N.check(self._lib.tv_ensemble_history_read(self._ens, out.ctypes.data_as(C.POINTER(C.c_double)), out.size,
                                                   C.byref(n_rec)), self._ens)
        step = (np.arange(n_rec.value) + 1) * every
        return {"step": step, "t": self.time[0] + step * self.dt, "T": out[:, 0], "Tf": out[:, 1],
                "sigma": out[:, 2]}

    def _stats(self):
        its = np.zeros(self.n_bars, dtype=np.intc)
        failed = np.zeros(self.n_bars, dtype=np.intc)
        total = np.zeros(self.n_bars, dtype=np.int64)
        N.check(self._lib.tv_ensemble_stats(self._ens, its.ctypes.data_as(C.POINTER(C.c_int)),
                                            failed.ctypes.data_as(C.POINTER(C.c_int)),
                                            total.ctypes.data_as(C.POINTER(C.c_int64))), self._ens)
        return its, failed, total

    @property
    def newton_iterations(self) -> np.ndarray:
        """Newton iterations of each bar's last solve."""
        return self._stats()[0]

    @property
    def failed_step(self) -> np.ndarray:
        """Per bar: the step (1-based) whose Newton solve failed, 0 = none."""
        return self._stats()[1]

    @property
    def newton_total(self) -> np.ndarray:
        """Per bar: Newton iterations summed over every step so far."""
        return self._stats()[2]

    def close(self) -> None:
        if self._ens is not None:
            self._lib.tv_ensemble_destroy(self._ens)
            self._ens = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
