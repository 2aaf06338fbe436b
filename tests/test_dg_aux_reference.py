"""CPU: the numpy restatement of the auxiliary-space multigrid for DG1 temperature
on general meshes (tests/dg_aux_reference.py, restating csrc/tv_umdg_aux.hip and
csrc/tv_amg.cpp aux_setup) is what a CG iteration needs and what the design
promises, on the oracle's own assembled operators:

  * the Galerkin operator P^T V_dg P of the injection P equals the oracle's CG1
    cell operator M + dt alpha K (continuous functions have no jumps: the SIPG
    terms vanish), to 1e-13 of its largest entry (measured <= 3.3e-15) -- so
    level 1 may be the CG path's own assembled V;
  * the cycle is symmetric (1e-12) and positive;
  * PCG on J(T) with the Newton right-hand side of the first step takes fewer
    iterations than the oracle's Jacobi-PCG: fewer than 2/3 on the two-level
    meshes (numpy model: 15 vs 29, 14 vs 28), fewer than 1/4 on `quad3`, whose
    dt alpha / h^2 ~ 54 makes the operator stiff (model: 21 vs 171).

Meshes: `quad` (72 cells) and `hex` (140 cells) of tests/test_unstructured_dg.py,
two levels; `quad3` (47 x 45 quadrilaterals, 2,208 vertices > 2000), three.
"""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

from dg_aux_reference import AuxCycle, aux_mesh, forms, injection, pcg
from oracle import tv_oracle as O

NAMES = ["quad", "hex", "quad3"]
LEVELS = {"quad": 2, "hex": 2, "quad3": 3}


def _T0(name):
    m = aux_mesh(name)
    return np.full(m.num_cells * 2 ** m.dim, float(O.ViscoParams(dict(O.MAIN_MODEL_PARAMS)).T_init))


@pytest.mark.parametrize("name", NAMES)
def test_galerkin_operator_is_the_cg_cell_operator(name):
    m = aux_mesh(name)
    dg, V = forms(name)
    mp = dict(O.MAIN_MODEL_PARAMS)
    # V_dg: the DG operator without its Robin terms (the same assembled form, the facet coefficients zeroed)
    cell = copy.copy(dg)
    cell.p = O.ThermalParams.from_dict({**mp, "epsilon": 0.0, "htc": 0.0})
    Vdg = sp.csr_matrix(cell.jacobian(_T0(name)))
    P = injection(m)
    G = sp.csr_matrix(P.T @ Vdg @ P)
    e = abs(G - V).max() / abs(V).max()
    print(f"[aux] {name}: |P^T V_dg P - V_cg| / max|V_cg| = {e:.2e}")
    assert e <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_cycle_is_symmetric_positive_and_cuts_the_iterations(name):
    dg, _ = forms(name)
    T = _T0(name)
    cyc = AuxCycle(name, T)
    assert cyc.n_levels == LEVELS[name]
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((2, T.size))
    bx, by = cyc.apply(x), cyc.apply(y)
    sym = abs(y @ bx - x @ by) / abs(y @ bx)
    assert sym <= 1e-12, sym
    assert x @ bx > 0 and y @ by > 0
    b = dg.residual(T, T)  # the Newton right-hand side of the first step
    _, kj = O.pcg_jacobi(cyc.J, b)
    _, ka = pcg(cyc.J, b, cyc.apply)
    print(f"[aux] {name}: {cyc.n_levels} levels {[lv[0].shape[0] for lv in cyc.levels]}, omega0 {cyc.omega0:.4f}, "
          f"symmetry {sym:.1e}, PCG iterations {ka} against Jacobi's {kj}")
    if name == "quad3":
        assert 4 * ka < kj, (ka, kj)
    else:
        assert 3 * ka < 2 * kj, (ka, kj)
