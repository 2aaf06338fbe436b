"""The cases of the ThermoViscoEnsemble tests, once: the bars, the six (family, model)
cells, the ensemble builders and the CPU-oracle runs.  A support module (pytest does not
collect it); it imports from no test module.

A Cell is one of {CG1, DG1} temperature x {reference, paper, exact} model, all with CG1
stress: the kernels ensemble_bar<Fam, kExt, kModel> of csrc/tv_ensemble_step.h.  A test
written over a Cell runs the one shared step driver in that instantiation.

Tolerances (data of the cell's checker, `check_reference` or `check_paper`): T rel. L2 <=
1e-10 per bar after every compared step; in the paper cells Tf and Tf_partial <= 1e-10 and
phi and xi <= 1e-9 (the trapezoidal xi is a sum: no cancellation); everything else through
parity_util.check_field with its tolerances (1e-6 on the nodes whose source dof moved more
than 1e-6 K in the oracle's last step, an absolute bound on the rest), the deviatoric
partials measured against the volumetric scale.  The compared fraction `min_frac`, which
the oracle's T alone decides: reference CG 0.9; reference DG 0.9, and 0.5 for bars 0 and 3
at 16 cells, whose cores have not moved 1e-6 K after six steps (the oracle's own share
there is 0.62-0.71); paper and exact 0.9 (CG) and 0.6 (DG: 1.00 except bars 0 (0.71) and 3
(0.65) at 16 cells); None for the equilibrium bar 4, whose T never moves.  Newton counts
(reference cells): equal wherever the oracle's own decision was at least a decade from
flipping, within one elsewhere (the last iterations sit at rounding level).

The hot bars (T_0 >= 850 K) lie outside the Taylor limit xi <= 2 lambda of the degree-2
exponential: in the paper cells their stress grows to 5e60 within six steps, in the oracle
and on the device alike, and overflows later; the exact cells stay finite.

Oracle runs are computed once per session and shared: leave the records unchanged.
"""
import contextlib
import functools
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from exact_relaxation import exact_relaxation
from oracle import tv_oracle as O
from parity_util import check_field, cond_mask, relerr

CFGS = {"cg": {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}},
        "dg": {"T": {"element": "DG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}}
DT = 0.1
N_STEPS = 8  # of the scheduled cases
# htc, T_0, T_ambient, epsilon, L (odd bars graded); bar 4 starts in equilibrium (zero residual, xi = 0; in
# reference mode a NaN stress: Q5)
BARS = [
    (280.1, 800.0, 600.0, 0.93, 50.0),
    (50.0, 900.0, 300.0, 0.9, 4.0),
    (1000.0, 850.0, 293.0, 0.8, 6.0),
    (0.0, 800.0, 600.0, 0.93, 50.0),
    (400.0, 600.0, 600.0, 0.93, 10.0),
    (120.0, 873.0, 350.0, 0.5, 19.0),
    (800.0, 920.0, 293.0, 0.93, 3.0),
    (280.1, 800.0, 600.0, 0.0, 8.0),
    (280.1, 780.0, 500.0, 0.93, 12.0),
    (600.0, 890.0, 293.0, 0.85, 5.0),
]
# T_0, epsilon, L, graded, stages (last step, htc, T_ambient); the last stage never ends
SBARS = [
    (800.0, 0.93, 50.0, False, [(3, 280.1, 600.0), (5, 1000.0, 293.0), (None, 50.0, 293.0)]),
    (900.0, 0.9, 4.0, True, [(2, 50.0, 300.0), (2, 999.0, 999.0), (None, 600.0, 350.0)]),  # empty middle stage
    (850.0, 0.8, 6.0, False, [(0, 1.0, 1.0), (4, 1000.0, 293.0), (None, 0.0, 293.0)]),  # empty first stage
    (873.0, 0.5, 10.0, True, [(1, 120.0, 350.0), (7, 800.0, 293.0), (None, 120.0, 500.0)]),
    (920.0, 0.93, 3.0, False, [(6, 800.0, 293.0), (7, 400.0, 700.0), (None, 10.0, 293.0)]),  # a reheating stage
    (800.0, 0.93, 8.0, True, [(100, 280.1, 600.0), (200, 1.0, 1.0), (None, 1.0, 1.0)]),  # never leaves stage 0
]
HOT = [b for b in range(10) if BARS[b][1] >= 850.0]  # outside the Taylor limit
THERMAL = ["T", "T_prev"]
VISCO = ["Tf", "Tf_partial", "phi", "xi", "sigma", "s_tilde_partial", "sigma_tilde_partial"]
PAPER_ONLY = ["s_partial", "sigma_partial"]  # state of a paper handle
STRESS = ["sigma", "s_partial", "sigma_partial", "s_tilde_partial", "sigma_tilde_partial"]


def gpu():
    """The GPU skip."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def graded(L, is_graded, n_cells):
    g = 0.5 if is_graded else 0.0
    s = np.linspace(0.0, 1.0, n_cells + 1)
    return L * (g * (1.0 - np.cos(np.pi * s)) / 2.0 + (1.0 - g) * s)


def coords(bar, n_cells):
    return graded(BARS[bar][4], bar % 2 == 1, n_cells)


def params(bar):
    htc, T0, Ta, eps, _ = BARS[bar]
    return dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=T0, T_ambient=Ta, epsilon=eps)


def stage_of(stages, step):
    """Index of the stage that holds the 1-based step: the first whose end is not before it."""
    for j, (end, _, _) in enumerate(stages):
        if end is None or step <= end:
            return j
    raise AssertionError


def src(fam, n_cells):
    """sigma node -> T dof.  CG: the node itself; DG: 2 i, and 2 n_cells - 1 for the last node (the last
    cell in cell order wins)."""
    if fam == "cg":
        return np.arange(n_cells + 1)
    return np.append(2 * np.arange(n_cells), 2 * n_cells - 1)


# ---- the end-state checkers ------------------------------------------------------------------
def check_reference(cell, tag, got, row, n_cells, ref, min_frac):
    """Row `row` of the state `got` against the oracle record `ref`: T, then phi / Tf / xi on the T dofs and
    sigma on the nodes whose source dof moved."""
    end = ref["end"]
    e = relerr(got["T"][row], end["T"])
    print(f"[ensemble {cell.id}] {tag}: T rel {e:.2e}")
    assert e <= 1e-10, (tag, e)
    mT, mS = cond_mask(end["T"], ref["T_before"], src_map=src(cell.fam, n_cells))
    return [check_field(f"{tag} {name}", got[name][row], end[name], mS if name == "sigma" else mT, 1,
                        min_frac=min_frac) for name in ("phi", "Tf", "xi", "sigma")]


def check_paper(cell, tag, got, row, n_cells, ref, min_frac):
    """Row `row` of the state `got` against the paper-oracle record `ref` (module docstring)."""
    end = finite_end(ref)["end"]
    e = relerr(got["T"][row], end["T"])
    print(f"[ensemble {cell.id}] {tag}: T rel {e:.2e}")
    assert e <= 1e-10, (tag, e)
    for name, tol in (("Tf", 1e-10), ("Tf_partial", 1e-10), ("phi", 1e-9), ("xi", 1e-9)):
        assert np.all(np.isfinite(got[name][row])), (tag, name)
        e = relerr(got[name][row], end[name])
        print(f"[ensemble {cell.id}] {tag}: {name} rel {e:.2e}")
        assert e <= tol, (tag, name, e)
    _, mS = cond_mask(end["T"], ref["T_before"], src_map=src(cell.fam, n_cells))
    vol = float(np.linalg.norm(end["sigma_partial"]))
    recs = []
    for name in STRESS:
        # the deviatoric partial stresses are rounding noise (isotropic strain): measured against the
        # volumetric scale, as tests/test_paper_mode.py does
        scale = vol if name.startswith("s_") else None
        recs.append(check_field(f"{tag} {name}", got[name][row], end[name], mS, 1 if name == "sigma" else 6,
                                min_frac=min_frac, scale=scale))
    return recs


# ---- the six cells ---------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Cell:
    fam: str                    # "cg" | "dg": the temperature family (the stress is CG1)
    model: str                  # "reference" | "paper" | "exact"
    ens_kw: dict                # ThermoViscoEnsemble keywords
    oracle_kw: dict             # OracleProblem keywords
    exact_oracle: bool          # the oracle runs inside exact_relaxation()
    state: tuple                # the state fields: 9, or 11 on a paper handle
    finite_sigma: bool          # paper model: no NaN stress, and every compared oracle array is finite
    frac: float                 # min_frac of a bar whose T moves
    sched_min_frac: Optional[float]  # of the scheduled end state; None: T only is compared there
    check_end: Callable         # check_reference | check_paper
    history_surface_sigma: bool  # the surface sigma of a history record is compared with the oracle's

    @property
    def id(self):
        return f"{self.fam}-{self.model}"

    @property
    def cfg(self):
        return CFGS[self.fam]

    @property
    def paper(self):
        return self.model != "reference"

    def n_T(self, n_cells):
        return 2 * n_cells if self.fam == "dg" else n_cells + 1

    def min_frac(self, bar, n_cells):
        """Of the ten BARS after six to eight steps (module docstring)."""
        if bar == 4:
            return None
        if self.id == "dg-reference" and n_cells == 16 and bar in (0, 3):
            return 0.5
        return self.frac


def _cell(fam, model):
    paper = model != "reference"
    return Cell(fam=fam, model=model,
                ens_kw={"reference": {}, "paper": dict(model_mode="paper"),
                        "exact": dict(model_mode="paper", relaxation="exact")}[model],
                oracle_kw=dict(model_mode="paper") if paper else {},
                exact_oracle=model == "exact",
                state=tuple(THERMAL + VISCO + (PAPER_ONLY if paper else [])),
                finite_sigma=paper,
                frac=0.6 if (paper and fam == "dg") else 0.9,
                sched_min_frac=None if (fam, model) == ("dg", "reference") else (0.6 if fam == "dg" else 0.9),
                check_end=check_paper if paper else check_reference,
                history_surface_sigma=(fam, model) == ("cg", "reference"))


CELLS = [_cell(fam, model) for model in ("reference", "paper", "exact") for fam in ("cg", "dg")]
CELL = {c.id: c for c in CELLS}
REFERENCE_CELLS = [c for c in CELLS if c.model == "reference"]
PAPER_CELLS = [c for c in CELLS if c.paper]  # paper and exact: the handles with eleven state fields


def cells(which=CELLS):
    """parametrize over cells, the test id being the cell's."""
    return pytest.mark.parametrize("cell", which, ids=lambda c: c.id)


# ---- builders --------------------------------------------------------------------------------
def _make(cell, meshes, mp, **kw):
    from tvfem import ThermoViscoEnsemble
    ens = ThermoViscoEnsemble(meshes, (0.0, 50.0), DT, cell.cfg, mp, **dict(cell.ens_kw, **kw))
    ens.setup()
    return ens


def ensemble(cell, bars, n_cells, **kw):
    """Rows of BARS, in the order given."""
    from tvfem import RectilinearMesh
    mp = dict(O.MAIN_MODEL_PARAMS)
    for k, col in (("htc", 0), ("T_0", 1), ("T_ambient", 2), ("epsilon", 3)):
        mp[k] = np.array([BARS[b][col] for b in bars])
    return _make(cell, [RectilinearMesh([coords(b, n_cells)]) for b in bars], mp, **kw)


def scheduled(cell, rows, n_cells, schedule=True, **kw):
    """Rows of SBARS with their three stages (or without: schedule=False)."""
    from tvfem import RectilinearMesh
    bars = [SBARS[r] for r in rows]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=np.array([b[0] for b in bars]), epsilon=np.array([b[1] for b in bars]))
    sched = None
    if schedule:
        sched = []
        for j in range(3):
            st = dict(htc=np.array([b[4][j][1] for b in bars]), T_ambient=np.array([b[4][j][2] for b in bars]))
            if j < 2:
                st["until_step"] = np.array([b[4][j][0] for b in bars])
            sched.append(st)
    return _make(cell, [RectilinearMesh([graded(b[2], b[3], n_cells)]) for b in bars], mp, schedule=sched, **kw)


def own():
    """(htc, T_ambient, epsilon) of the ten BARS."""
    return tuple(np.array([b[c] for b in BARS]) for c in (0, 2, 3))


def ten(cell, n_cells, values=None, **kw):
    """The ten BARS; `values` replaces (htc, T_ambient, epsilon) of creation."""
    from tvfem import RectilinearMesh
    htc, Ta, eps = values if values is not None else own()
    mp = dict(O.MAIN_MODEL_PARAMS, htc=htc, T_0=np.array([b[1] for b in BARS]), T_ambient=Ta, epsilon=eps)
    return _make(cell, [RectilinearMesh([coords(i, n_cells)]) for i in range(10)], mp, **kw)


def state(ens, names=None):
    """The state fields of `ens` (by its own model mode: nine, or eleven on a paper handle)."""
    if names is None:
        names = THERMAL + VISCO + (PAPER_ONLY if ens.model_mode == "paper" else [])
    return {f: ens.get_field(f) for f in names}


def same(got, want, tag, names=None):
    for f in (names if names is not None else want):
        assert np.array_equal(got[f], want[f], equal_nan=True), (tag, f)


def plain_and_scheduled(cell, n_bars, n_cells, n_steps, every, finish):
    """What the red-zone tests compare between two runs: BARS and SBARS repeated into n_bars lanes, n_steps
    steps, plain and then with the three-stage schedule and a history of the two end probes; every state
    field, record and statistic.  finish(lib) is called while each handle is still live."""
    out = {}
    ens = ensemble(cell, [b % 10 for b in range(n_bars)], n_cells)
    ens.solve(n_steps)
    for f in cell.state:
        out["plain/" + f] = ens.get_field(f)
    out["plain/its"] = np.asarray(ens.newton_iterations)
    out["plain/total"] = np.asarray(ens.newton_total)
    out["plain/failed"] = np.asarray(ens.failed_step)
    finish(ens._lib)
    ens.close()
    ens = scheduled(cell, [b % 6 for b in range(n_bars)], n_cells, history=dict(nodes=[0, n_cells], every=every))
    ens.solve(n_steps)
    for f in cell.state:
        out["sched/" + f] = ens.get_field(f)
    h = ens.get_history()
    for k in ("step", "T", "Tf", "sigma"):
        out["hist/" + k] = np.asarray(h[k])
    out["sched/total"] = np.asarray(ens.newton_total)
    out["sched/failed"] = np.asarray(ens.failed_step)
    finish(ens._lib)
    ens.close()
    return out


# ---- the oracle ------------------------------------------------------------------------------
def newton_margin(form, T, Tp, rtol=1e-12, atol=1e-10, max_it=50):
    """oracle.newton_solve restated over HeatForm (T is a copy: the oracle's
    own state is untouched): the iteration count and how far, in decades, the
    nearest convergence decision of the solve was from flipping."""
    T = T.copy()
    it, conv, r0, margin = 0, False, 0.0, np.inf
    b = form.residual(T, Tp)
    with np.errstate(divide="ignore", invalid="ignore"):
        while not conv and it < max_it:
            dx = spla.spsolve(form.jacobian(T).tocsc(), b)
            T -= dx
            it += 1
            b = form.residual(T, Tp)
            r = np.linalg.norm(dx)
            if it == 1:
                r0 = r
                continue
            rel = r / r0 if r0 != 0.0 else (np.inf if r != 0.0 else np.nan)
            conv = bool(rel < rtol or r < atol)
            if conv:
                m = np.fmax(np.log10(rtol / rel), np.log10(atol / r))
            else:
                m = np.fmin(np.log10(rel / rtol), np.log10(r / atol))
            margin = min(margin, float(m))
    return it, margin


def oracle(cell, mesh_coords, mp, n_cells):
    ref = O.OracleProblem(O.rectilinear_mesh([mesh_coords]), (0.0, 50.0), DT, cell.cfg, mp, linear="direct",
                          **cell.oracle_kw)
    ref.setup()
    assert np.array_equal(ref._maps[("S", "T")], src(cell.fam, n_cells))
    return ref


def compared_state(ref, paper=True):
    """The fields of an oracle that the ensemble tests compare, as float64 copies."""
    fc, fn, f = ref.functions_current, ref.functions_next, ref.functions
    end = {"T": fc["T"], "Tf": fc["Tf"], "phi": f["phi"], "xi": f["xi"], "sigma": fn["sigma"]}
    if paper:
        end.update({k: fc[k] for k in ("Tf_partial", "s_partial", "sigma_partial", "s_tilde_partial",
                                       "sigma_tilde_partial")})
    return {k: np.array(v, dtype=np.float64) for k, v in end.items()}


def finite_end(ref):
    """Every compared array of the record is finite, so NaN == NaN hides nothing."""
    for k, v in ref["end"].items():
        assert np.all(np.isfinite(v)), f"the oracle's {k} is not finite"
    return ref


def _context(cell):
    return exact_relaxation() if cell.exact_oracle else contextlib.nullcontext()


@functools.lru_cache(maxsize=None)
def _oracle_run(cell, bar, n_cells, n_steps, keep_every_step):
    ref = oracle(cell, coords(bar, n_cells), params(bar), n_cells)
    Ts, hist = [], []
    T_before, first_nonfinite = None, None
    with _context(cell), np.errstate(all="ignore"):
        for step in range(1, n_steps + 1):
            if keep_every_step and not cell.paper:
                it, margin = newton_margin(ref.form, ref.functions_current["T"], ref.functions_previous["T"])
            T_before = ref.functions_current["T"].copy()
            ref.solve_timestep()
            if keep_every_step:
                Ts.append(ref.functions_current["T"].copy())
                if not cell.paper:
                    assert ref.newton_history[-1][0] == it  # the helper restates the oracle's loop
                    hist.append((it, margin))
            if cell.paper and first_nonfinite is None and \
                    not all(np.all(np.isfinite(v)) for v in compared_state(ref).values()):
                first_nonfinite = step
    return {"Ts": Ts, "hist": hist, "T_before": T_before, "end": compared_state(ref, cell.paper),
            "first_nonfinite": first_nonfinite}


def oracle_run(cell, bar, n_cells, n_steps, keep_every_step=False, finite=None):
    """Bar `bar` of BARS through the cell's oracle, once per session: T after every step (or only the last),
    the state at the end, T before the last step; in the reference cells per step (Newton count, decision
    margin); in the paper cells "first_nonfinite", the first step (1-based) after which a compared field is
    not finite, or None.  The end of a paper-cell run is asserted finite unless finite=False."""
    ref = _oracle_run(cell, bar, n_cells, n_steps, keep_every_step)
    return finite_end(ref) if (cell.finite_sigma if finite is None else finite) else ref


@functools.lru_cache(maxsize=None)
def _scheduled_oracle_run(cell, row, n_cells):
    T0, eps, L, is_graded, stages = SBARS[row]
    mp = dict(O.MAIN_MODEL_PARAMS, T_0=T0, epsilon=eps, htc=stages[0][1], T_ambient=stages[0][2])
    ref = oracle(cell, graded(L, is_graded, n_cells), mp, n_cells)
    out = {"Ts": [], "Tfs": [], "sigmas": [], "T_befores": []}
    with _context(cell), np.errstate(all="ignore"):
        for step in range(1, N_STEPS + 1):
            _, htc, Ta = stages[stage_of(stages, step)]
            ref.tp.htc, ref.tp.T_ambient, ref.tp.epsilon = htc, Ta, eps
            out["T_befores"].append(ref.functions_current["T"].copy())
            ref.solve_timestep()
            out["Ts"].append(ref.functions_current["T"].copy())
            out["Tfs"].append(ref.functions_current["Tf"].copy())
            out["sigmas"].append(ref.functions_next["sigma"].copy())
    out["T_before"] = out["T_befores"][-1]
    out["end"] = compared_state(ref, cell.paper)
    return out


def scheduled_oracle_run(cell, row, n_cells):
    """Bar `row` of SBARS through the cell's oracle, its ThermalParams set to the step's stage before each of
    the N_STEPS steps, once per session: T, Tf, sigma after every step, T before every step, the end state."""
    ref = _scheduled_oracle_run(cell, row, n_cells)
    return finite_end(ref) if cell.finite_sigma else ref
