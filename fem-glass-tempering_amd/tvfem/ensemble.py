"""``ThermoViscoEnsemble`` — thousands of independent 1D tempering bars in one
launch (the ``tv_ensemble_*`` entry points of libtvfem.so).

A parameter study of the reference's own workload (main.py: one
through-thickness bar): every bar has the same cell count and may have its
own node coordinates (thickness, grading) and its own ``htc``, ``T_0``,
``T_ambient``, ``epsilon``, ``alpha`` and ``f``; ``dt`` and every other model
parameter are shared.  CG1 temperature and stress, reference model mode.

    ens = ThermoViscoEnsemble(mesh, (0.0, 50.0), 0.1, fe_config,
                              dict(model_params, htc=np.linspace(50, 1000, 4096)))
    ens.setup()
    ens.solve()
    sigma = ens.get_field("sigma")        # (n_bars, n_dofs)
"""
from __future__ import annotations

import ctypes as C
from math import ceil

import numpy as np

from . import _native as N
from .mesh import RectilinearMesh

# model parameters that may differ from bar to bar
PER_BAR_KEYS = ("htc", "T_0", "T_ambient", "epsilon", "alpha", "f")
# the state an ensemble keeps (names as ThermoViscoProblem.get_field) and its block size per dof
STATE_FIELDS = {"T": 1, "T_prev": 1, "Tf": 1, "Tf_partial": 6, "phi": 1, "xi": 1, "sigma": 1,
                "s_tilde_partial": 6, "sigma_tilde_partial": 6}
_FAMILIES = {"CG": N.TV_CG, "DG": N.TV_DG}


class ThermoViscoEnsemble:
    def __init__(self, meshes, time: tuple, dt: float, config: dict, model_parameters: dict, *,
                 n_bars: int | None = None, device: int = 0, model_mode: str = "reference",
                 newton_rtol: float | None = None, newton_atol: float | None = None,
                 newton_max_it: int | None = None, error_on_nonconvergence: bool = True) -> None:
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
        sizes = {len(v) for v in arrays.values()}
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
        self.dt = dt
        self.time = time
        self.t = self.time[0]
        self.n_steps = ceil((self.time[1] - self.time[0]) / self.dt)
        self.n_dofs = self.n_cells + 1
        self.config = config
        self.coords = np.ascontiguousarray(np.stack([m.axes[0] for m in mlist]))
        self._arrays = arrays
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
        opts.model_mode = N.TV_MODEL_PAPER if model_mode == "paper" else N.TV_MODEL_REFERENCE
        if newton_rtol is not None:
            opts.newton_rtol = newton_rtol
        if newton_atol is not None:
            opts.newton_atol = newton_atol
        if newton_max_it is not None:
            opts.newton_max_it = newton_max_it
        opts.error_on_nonconvergence = 1 if error_on_nonconvergence else 0
        ens = C.c_void_p()
        N.check(lib.tv_ensemble_create(C.byref(desc), C.byref(fe), C.byref(params), C.byref(opts), device,
                                       C.byref(ens)))
        self._ens = ens

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
        """(n_bars, n_dofs * bs) array, per bar the reference's interleaved layout."""
        out = np.empty((self.n_bars, self.n_dofs * STATE_FIELDS.get(name, 1)))
        N.check(self._lib.tv_ensemble_get_field(self._ens, N.FIELD_ID[name],
                                                out.ctypes.data_as(C.POINTER(C.c_double)), out.size), self._ens)
        return out

    def set_field(self, name: str, values) -> None:
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        N.check(self._lib.tv_ensemble_set_field(self._ens, N.FIELD_ID[name],
                                                v.ctypes.data_as(C.POINTER(C.c_double)), v.size), self._ens)

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
