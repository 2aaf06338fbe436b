"""Numpy restatement of the auxiliary-space multigrid for DG1 temperature on
general meshes (options.preconditioner = TV_PC_AUX), for tests/test_dg_aux_reference.py,
tests/test_unstructured_dg_aux.py and tests/test_guard_bands_umdg_aux.py.  Test
infrastructure: never imported by the product path.

What it restates, step by step (fem-glass-tempering_amd/csrc):
  * tv_umdg_aux.hip k_umdg_binv: B_e = the diagonal NL x NL block of J(T) of cell e,
    Robin Jacobian of its exterior facets included -- here the diagonal blocks of
    the oracle's assembled DG `HeatForm.jacobian(T)`, inverted by numpy;
  * tv_mgsolve.cpp level0_lambda / level0_weight with B^-1 in the place of dinv:
    omega0 = 2 / (1.1 lambda), lambda = |B^-1 J x| after 30 power iterations from
    the xorshift start vector indexed by DEVICE dof l nc + e;
  * tv_amg.cpp aux_setup: level 1 = the CG1 cell operator V = M + dt alpha K of
    the same mesh (the oracle's CG HeatForm without Robin terms), dinv = 1 / diag V,
    omega1 = 2 / (1.1 lam_max(V, dinv, 20)); P copies the value of vertex
    cells[e][l] into DG dof (e, l), P^T sums the copies; below level 1
    `oracle.amg.build(V)` exactly as for a CG mesh; mg_levels counts the DG and
    the CG level (2: no aggregation level);
  * tv_amg.cpp amg_apply0 / amg_level, tv_umdg_aux.hip restrict / prolong0:
    apply(r) = omega0 B^-1 r + P V_1(P^T r), V_1 = `oracle.amg._level(levels, 1, .)`.

Vectors here are in the oracle's cell-major order (dof = cell 2^dim + l);
`test_unstructured_dg.device_layout` / `host_layout` convert to and from the
device's [l][cell].
"""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import amg as OA
from oracle import tv_oracle as O
from test_unstructured_dg import host_layout, mesh, oracle_mesh

DT = 0.1
QUAD3 = ((47, 45), (2.0, 2.0))  # 2,115 cells, 2,208 vertices (> 2000: one aggregation level below CG1)


@functools.lru_cache(maxsize=None)
def aux_mesh(name):
    if name == "quad3":
        from tvfem import distorted_box_mesh
        n, L = QUAD3
        return distorted_box_mesh(L, n, amp=0.2, seed=0, shuffle=True)
    return mesh(name)


@functools.lru_cache(maxsize=None)
def forms(name):
    """(the oracle's DG HeatForm, the CG1 cell operator V) of a mesh: assembled once, read only"""
    m = aux_mesh(name)
    om = oracle_mesh(m)
    mp = dict(O.MAIN_MODEL_PARAMS)
    dg = O.HeatForm(O.Space(om, "DG"), DT, O.ThermalParams.from_dict(mp))
    cg = O.HeatForm(O.Space(om, "CG"), DT, O.ThermalParams.from_dict({**mp, "epsilon": 0.0, "htc": 0.0}))
    V = sp.csr_matrix(cg.jacobian(np.full(m.num_vertices, 800.0)))  # T-independent without Robin terms
    return dg, V


def injection(m):
    """P: DG dof (e, l), cell-major, takes the value of vertex cells[e][l]"""
    nl = 2 ** m.dim
    n = m.num_cells * nl
    return sp.csr_matrix((np.ones(n), (np.arange(n), np.asarray(m.cells).reshape(-1))), shape=(n, m.num_vertices))


def diagonal_blocks(J, nl):
    """the nl x nl diagonal blocks of a cell-major DG matrix, (cells, nl, nl)"""
    Jb = sp.bsr_matrix(J, blocksize=(nl, nl))
    Jb.sort_indices()
    nc = J.shape[0] // nl
    B = np.zeros((nc, nl, nl))
    for e in range(nc):
        k = np.searchsorted(Jb.indices[Jb.indptr[e]:Jb.indptr[e + 1]], e)
        assert Jb.indices[Jb.indptr[e] + k] == e
        B[e] = Jb.data[Jb.indptr[e] + k]
    return B


def power_lambda(J, smooth, dim, its=30):
    """tv_mgsolve.cpp level0_lambda: |B^-1 J x| after `its` power iterations (not
    converged: the start vector is part of the result) from the xorshift start
    vector, which the device indexes by ITS dof l n_cells + cell; J and `smooth`
    (r -> B^-1 r) cell-major.  Shared with tests/dg_gmg_reference.py."""
    x = host_layout(dim, OA._xorshift_start(J.shape[0], 0x9E3779B97F4A7C15))  # started in device dof order
    x = x / np.sqrt(np.dot(x, x))
    lam = 0.0
    for _ in range(its):
        w = smooth(J @ x)
        lam = np.sqrt(np.dot(w, w))
        x = w / lam
    return lam


class AuxCycle:
    """The TV_PC_AUX preconditioner at temperature T (cell-major) on mesh `name`."""

    def __init__(self, name, T, mg_levels=0):
        m = aux_mesh(name)
        dg, V = forms(name)
        self.nl = 2 ** m.dim
        self.dim = m.dim
        self.J = sp.csr_matrix(dg.jacobian(T))
        self.B = diagonal_blocks(self.J, self.nl)
        self.Binv = np.linalg.inv(self.B)
        self.P = injection(m)
        self.V = V
        d1 = 1.0 / V.diagonal()
        max_levels = mg_levels if mg_levels > 0 else 12  # tv_amg.cpp amg_build: the DG level counts
        self.levels = [(V, self.P, sp.csr_matrix(self.P.T), d1, 2.0 / (1.1 * OA.lam_max_host(V, d1, 20)))]
        self.levels += OA.build(V, max_levels=max_levels - 1)
        self.omega0 = 2.0 / (1.1 * self._lambda())

    def smooth(self, r):
        return np.einsum("eij,ej->ei", self.Binv, r.reshape(-1, self.nl)).reshape(-1)

    def _lambda(self, its=30):
        return power_lambda(self.J, self.smooth, self.dim, its)

    @property
    def n_levels(self):
        return 1 + len(self.levels)

    def apply(self, r):
        return self.omega0 * self.smooth(r) + self.P @ OA._level(self.levels, 1, self.P.T @ r)


def pcg(A, b, apply, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000):
    """oracle pcg_jacobi (PETSc KSPCG, preconditioned norm, zero initial guess) with z = apply(r)"""
    x = np.zeros_like(b)
    r = b.copy()
    z = apply(r)
    dp = np.linalg.norm(z)
    rnorm0 = dp
    ttol = max(rtol * rnorm0, atol)
    if dp <= ttol:
        return x, 0
    beta = z @ r
    betaold = beta
    p = None
    for i in range(max_it):
        if beta == 0.0:
            return x, i
        p = z.copy() if i == 0 else z + (beta / betaold) * p
        w = A @ p
        dpi = p @ w
        betaold = beta
        if dpi <= 0.0:
            raise RuntimeError("KSP diverged: indefinite matrix")
        a = beta / dpi
        x += a * p
        r -= a * w
        z = apply(r)
        dp = np.linalg.norm(z)
        if dp <= ttol:
            return x, i + 1
        if dp >= dtol * rnorm0 or not np.isfinite(dp):
            raise RuntimeError("KSP diverged")
        beta = z @ r
    raise RuntimeError("KSP did not converge (max_it)")
