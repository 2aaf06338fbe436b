"""CPU: the numpy restatement of the box multigrid for a DG1 temperature
(tests/dg_gmg_reference.py, restating csrc/tv_dg.hip fdm_mul, csrc/tv_mg.hip
k_mg_dg_* and csrc/tv_mgsolve.cpp mg_cycle_box) is what the kernels' comments
promise and what a CG iteration needs, on the oracle's own assembled operators:

  * on a T that is constant on every exterior facet the facet mean is exact, so
    B_c is the diagonal block of J(T), to 1e-13 of the largest entry;
  * B_c = Mx (x) My (x) Mz + dt alpha (Ax (x) My (x) Mz + Mx (x) Ay (x) Mz +
    Mx (x) My (x) Az) from 1D 2 x 2 matrices, as the comment above fdm_mul states
    (A_k: stiffness, the SIPG self terms of the interior facets along k, the Robin
    term dt / (dt alpha) gbar on an exterior one), to 1e-13 -- at alpha = 1 and at
    alpha = 0.37, dt = 0.25, where dt / (dt alpha) != 1;
  * at a general T the blocks are symmetric positive definite and differ from the
    diagonal blocks of J(T) (so a 1e-10 comparison tells the two apart);
  * the cycle is symmetric (1e-13) and positive;
  * KSPCG with the cycle reaches the direct solution of J dx = F, in 6 iterations
    on the 315-cell grid against 35 with the block smoother alone (omega0 B^-1: what
    the cycle collapses to if its transfers are masked away) -- the count tells a
    working coarse correction from a missing one;
  * the weight omega0 follows the T it is estimated at by far more than the 1e-10
    at which the device is compared (the kept-weight test of test_multigrid_dg.py
    would show nothing otherwise).
"""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from dg_aux_reference import diagonal_blocks
from dg_gmg_reference import GRIDS, NL, DgBox, DgGmgCycle, block_mul, cg_depth, params
from krylov_reference import kspcg
from oracle import tv_oracle as O

CASES = {  # id: (grid, dt, alpha, mg_levels)
    "two_blocks": ("two_blocks", 0.1, None, 0),
    "graded_3": ("graded", 0.1, None, 3),
    "thin": ("thin", 0.1, None, 0),
    "graded_alpha": ("graded", 0.25, 0.37, 0),
}


@functools.lru_cache(maxsize=None)
def box(grid, dt=0.1, alpha=None):
    return DgBox(GRIDS[grid], dt, params(alpha))


def random_T(n, seed=11):
    return 700.0 + np.random.default_rng(seed).uniform(0.0, 150.0, n)


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("case", list(CASES))
def test_blocks_are_the_diagonal_blocks_at_facetwise_constant_T(case):
    grid, dt, alpha, _ = CASES[case]
    b = box(grid, dt, alpha)
    T = np.repeat(random_T(b.n // NL), NL)  # constant per cell, so on every exterior facet
    e = relmax(b.blocks(T), diagonal_blocks(b.jacobian(T), NL))
    print(f"[dg gmg ref] {case}: B_c vs diagonal blocks of J at facet-wise constant T {e:.1e}")
    assert e <= 1e-13
    # and at a general T they are not the diagonal blocks
    T = random_T(b.n)
    d = relmax(b.blocks(T), diagonal_blocks(b.jacobian(T), NL))
    print(f"[dg gmg ref] {case}: B_c vs diagonal blocks of J at T = 700 + U(0, 150) {d:.1e}")
    assert d > 1e-6


def kron_blocks(b, T):
    """the comment above fdm_mul, from 1D matrices"""
    axes, dt, alpha = b.axes, b.dt, b.mp["alpha"]
    da = dt * alpha
    cn = [len(a) - 1 for a in axes]
    h = [np.diff(a) for a in axes]
    f = b.form
    gbar = {}  # (cell, axis, side) -> the facet mean of dg(T)
    lfs = O._local_facets(3)
    for (cell, lf), nodes in zip(f.ext, b.facet_nodes):
        k, side, _ = lfs[lf]
        gbar[(int(cell), k, side)] = f._dg(T.reshape(-1, NL)[cell, nodes]).mean()
    out = np.zeros((b.n // NL, NL, NL))
    for cell in range(b.n // NL):
        ci = [cell % cn[0], (cell // cn[0]) % cn[1], cell // (cn[0] * cn[1])]
        hc = [h[k][ci[k]] for k in range(3)]
        M, A = [], []
        for k in range(3):
            hk = hc[k]
            M.append(hk / 6.0 * np.array([[2.0, 1.0], [1.0, 2.0]]))
            Ak = np.array([[1.0, -1.0], [-1.0, 1.0]]) / hk
            for side in (0, 1):
                nb = ci[k] + (1 if side else -1)
                if 0 <= nb < cn[k]:  # SIPG self terms: penalty / h('+'), '+' the cell of the lower index
                    hp = list(hc)
                    if not side:
                        hp[k] = h[k][nb]
                    pen = f.penalty / np.sqrt(sum(v * v for v in hp))
                    Ak[0, 1] += 0.5 / hk
                    Ak[1, 0] += 0.5 / hk
                    Ak[side, side] += pen - 1.0 / hk
                else:
                    Ak[side, side] += dt / da * gbar[(cell, k, side)]
            A.append(Ak)
        k3 = lambda z, y, x: np.kron(z, np.kron(y, x))  # noqa: E731  l = a + 2 b + 4 c
        out[cell] = k3(M[2], M[1], M[0]) + da * (k3(M[2], M[1], A[0]) + k3(M[2], A[1], M[0]) + k3(A[2], M[1], M[0]))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_blocks_are_the_kronecker_sum_of_1d_matrices(case):
    grid, dt, alpha, _ = CASES[case]
    b = box(grid, dt, alpha)
    T = random_T(b.n)
    B = b.blocks(T)
    e = relmax(B, kron_blocks(b, T))
    lo = np.linalg.eigvalsh(B)[:, 0].min()
    print(f"[dg gmg ref] {case}: B_c vs the Kronecker sum {e:.1e}, smallest eigenvalue {lo:.3e}")
    assert e <= 1e-13
    assert np.abs(B - B.transpose(0, 2, 1)).max() <= 1e-15 * np.abs(B).max()
    assert lo > 0.0


@pytest.mark.parametrize("case", list(CASES))
def test_cycle_is_symmetric_and_positive(case):
    grid, dt, alpha, levels = CASES[case]
    b = box(grid, dt, alpha)
    cyc = DgGmgCycle(b, random_T(b.n), mg_levels=levels)
    x, y = np.random.default_rng(0).standard_normal((2, b.n))
    bx, by = cyc.apply(x), cyc.apply(y)
    sym = abs(y @ bx - x @ by) / abs(y @ bx)
    print(f"[dg gmg ref] {case}: {cyc.cg_levels} CG levels, lambda {cyc.lam:.4f}, omega0 {cyc.omega0:.4f}, "
          f"symmetry {sym:.1e}")
    assert sym <= 1e-13, sym
    assert x @ bx > 0.0 and y @ by > 0.0


def test_depths():
    mp = params()
    assert cg_depth(GRIDS["two_blocks"], 0.1, mp["alpha"]) == 3
    assert [cg_depth(GRIDS["graded"], 0.1, 1.0, L) for L in (1, 2, 3, 4)] == [1, 1, 2, 3]


def test_weight_is_not_converged_and_follows_T():
    """30 power iterations are not converged (so the start vector's order is
    restated), and omega0 moves with T by far more than the comparison's 1e-10."""
    from dg_aux_reference import power_lambda
    b = box("two_blocks")
    Ta = random_T(b.n)
    Tb = Ta + 40.0
    ca = DgGmgCycle(b, Ta)
    l330 = power_lambda(ca.J, lambda r: block_mul(ca.Binv, r), 3, its=330)
    print(f"[dg gmg ref] lambda after 30 iterations {ca.lam:.4f}, after 330 {l330:.4f}")
    assert abs(l330 / ca.lam - 1.0) > 1e-3
    kept, fresh = DgGmgCycle(b, Tb, T_weight=Ta), DgGmgCycle(b, Tb)
    assert kept.omega0 == ca.omega0
    r = np.random.default_rng(1).standard_normal(b.n)
    zk, zf = kept.apply(r), fresh.apply(r)
    d = float(np.linalg.norm(zk - zf) / np.linalg.norm(zf))
    print(f"[dg gmg ref] omega0 at T_a {kept.omega0:.8f}, at T_b {fresh.omega0:.8f}: the cycles differ by {d:.2e}")
    assert d > 100 * 1e-10


@pytest.mark.parametrize("grid,k_cycle", [("dg", 6), ("dg-graded", 5)])
def test_kspcg_with_the_cycle(grid, k_cycle):
    """the systems of tests/test_krylov.py (state of test_krylov.state)"""
    import test_krylov as K
    s = K.system(grid, "DG")
    cyc = K.precond(grid, "DG", "gmg-dg")
    ref, _ = K.reference(grid, "DG", "gmg-dg")
    alone = kspcg(s["J"], s["F"], cyc.smooth)
    print(f"[dg gmg ref] {grid}: KSPCG iterations: the cycle {ref.its}, the block smoother alone {alone.its}")
    assert ref.reason == alone.reason == "CONVERGED_RTOL"
    assert ref.its == k_cycle and ref.its >= 3
    # no count may be marginal (test_krylov.end_reason_sequence refuses such a case on the GPU)
    ttol = max(1e-5 * ref.dp[0], 1e-50)
    assert min(abs(float(dp / ttol) - 1.0) for dp in ref.dp) >= 1e-3
    assert 3 * ref.its <= alone.its, (ref.its, alone.its)
    # to the direct solution
    tight = kspcg(s["J"], s["F"], cyc, rtol=1e-13, dtype=np.float64)
    x = spla.spsolve(s["J"].tocsc(), s["F"])
    e = float(np.linalg.norm(tight.x[-1] - x) / np.linalg.norm(x))
    print(f"[dg gmg ref] {grid}: KSPCG at rtol 1e-13 ({tight.its} iterations) vs spsolve {e:.1e}")
    assert tight.reason == "CONVERGED_RTOL"
    assert e <= 1e-10
