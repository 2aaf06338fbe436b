"""Numpy restatement of the box geometric multigrid for a DG1 temperature
(options.preconditioner = TV_PC_GMG on a rectilinear 3D mesh, the multigrid of
benchmark configuration C5), for tests/test_dg_gmg_reference.py,
tests/test_multigrid_dg.py and tests/test_krylov.py.  Test infrastructure: never
imported by the product path.

What it restates, step by step (fem-glass-tempering_amd/csrc):
  * tv_dg.hip fdm_mul / fdm2 / k_dg_gface: B_c, the 8 x 8 block of cell c the fast
    diagonalisation inverts.  It is NOT the diagonal block of J(T): the cell term
    and the SIPG self terms are (the diagonal blocks of the oracle's DG Jacobian
    assembled with epsilon = htc = 0), but the Robin weight dg(T) is taken constant
    over an exterior facet -- gbar, the mean of dg at the facet's 4 nodal values --
    so that the block stays a Kronecker sum: + dt gbar sum_q w_q phi_i phi_j per
    exterior facet (the form's ext, ef_w, ef_phi, _dg).  The kernel writes this
    term as dt alpha (dt / (dt alpha) gbar): at alpha != 1 the factor matters.
    B^-1 by numpy.linalg.inv;
  * tv_mgsolve.cpp level0_lambda / level0_weight: omega0 = 2 / (1.21 lambda),
    lambda = |B^-1 J x| after exactly 30 power iterations from the xorshift start
    vector in device dof order (dg_aux_reference.power_lambda) -- estimated ONCE, at
    the T of the first solve or PCApply, and kept: `T_weight`;
  * tv_mg.hip k_mg_dg_restrict / k_mg_dg_prolong / k_mg_dg_T: level 1 is the CG1
    space of the same box; P copies vertex cells[e][l] into dof (e, l), R = P^T
    sums the copies, level 1's T is the vertex mean of the DG copies;
  * tv_mgsolve.cpp mg_setup: the CG level is always there; mg_levels = L > 0 gives
    max(1, L - 1) CG levels, automatic min(auto_levels(axes, dt, alpha), 7); from
    level 1 down it is gmg_reference.vcycle_reference (the pre-smoothing formed by
    the restriction, the Gershgorin weights, the coarser levels);
  * mg_cycle_box: x = omega0 B^-1 r; x += P V_cg(P^T (r - J x));
    z = x + omega0 B^-1 (r - J x)  (k_dg_bsmooth / k_dg_bupdate, k_dg_bpost).

Vectors are in the oracle's cell-major order (dof = 8 cell + l);
`test_unstructured_dg.device_layout` / `host_layout` convert to and from the
device's [l][cell].
"""
import copy

import numpy as np
import scipy.sparse as sp

from dg_aux_reference import diagonal_blocks, power_lambda
from gmg_reference import auto_levels, vcycle_reference
from oracle import tv_oracle as O

NL = 8
GRIDS = {
    # 315 cells: one full 256-thread block and a partial one, no multiple of 64, odd counts on every
    # axis; the automatic depth gives three CG levels
    "two_blocks": [np.linspace(0.0, 2.25, 10), np.linspace(0.0, 1.75, 8), np.linspace(0.0, 1.25, 6)],
    # graded along x and z: the neighbours' lengths enter the SIPG penalty
    "graded": [np.array([0.0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 2.2]), np.linspace(0.0, 1.5, 6),
               np.array([0.0, 0.2, 0.5, 1.0])],
    # one cell along x (a Robin facet on both sides of the axis, both neighbour indices clamped)
    "thin": [np.array([0.0, 0.4]), np.linspace(0.0, 1.5, 4), np.array([0.0, 0.2, 0.5])],
}


def params(alpha=None):
    mp = dict(O.MAIN_MODEL_PARAMS)
    if alpha is not None:
        mp["alpha"] = alpha
    return mp


def injection(mesh):
    """P: DG dof (e, l), cell-major, takes the value of vertex cells[e][l]"""
    n = mesh.n_cells * NL
    return sp.csr_matrix((np.ones(n), (np.arange(n), mesh.cells.reshape(-1))), shape=(n, mesh.n_vertices))


def cg_depth(axes, dt, alpha, mg_levels=0):
    """the number of CG levels mg_setup builds below the DG level"""
    if mg_levels > 0:
        return max(1, mg_levels - 1)
    return min(auto_levels(axes, dt, alpha), 7)


class DgBox:
    """The T-independent part of a DG1 box problem: the oracle's form, the cell
    and SIPG-self blocks, the facet masses.  Read only once built."""

    def __init__(self, axes, dt=0.1, mp=None):
        self.axes = [np.asarray(a, dtype=float) for a in axes]
        assert len(self.axes) == 3
        self.dt = dt
        self.mp = params() if mp is None else dict(mp)
        self.mesh = O.rectilinear_mesh(self.axes)
        self.form = O.HeatForm(O.Space(self.mesh, "DG"), dt, O.ThermalParams.from_dict(self.mp))
        self.n = self.form.V.n
        bare = copy.copy(self.form)  # the same assembled form without its Robin terms
        bare.p = O.ThermalParams.from_dict({**self.mp, "epsilon": 0.0, "htc": 0.0})
        self.B0 = diagonal_blocks(sp.csr_matrix(bare.jacobian(np.zeros(self.n))), NL)
        f = self.form
        self.facet_mass = np.einsum("fq,fqi,fqj->fij", f.ef_w, f.ef_phi, f.ef_phi)  # sum_q w_q phi_i phi_j
        lfs = O._local_facets(3)
        self.facet_nodes = np.array([lfs[lf][2] for lf in f.ext[:, 1]])  # (facets, 4) local dofs on the facet
        self.P = injection(self.mesh)
        self.copies = np.asarray(self.P.sum(axis=0)).ravel()

    def jacobian(self, T):
        return sp.csr_matrix(self.form.jacobian(T))

    def blocks(self, T):
        """B_c at T, (cells, 8, 8)"""
        f = self.form
        cells = f.ext[:, 0]
        Tf = T.reshape(-1, NL)[cells[:, None], self.facet_nodes]
        gbar = f._dg(Tf).mean(axis=1)
        B = self.B0.copy()
        np.add.at(B, cells, self.dt * gbar[:, None, None] * self.facet_mass)
        return B

    def vertex_mean(self, T):
        """level 1's T (k_mg_dg_T)"""
        return (self.P.T @ T) / self.copies


class DgGmgCycle:
    """The TV_PC_GMG preconditioner of a DG1 box at temperature T (cell-major).
    T_weight: the temperature at which omega0 was estimated (the first solve's;
    default: T)."""

    def __init__(self, box, T, mg_levels=0, T_weight=None):
        self.box = box
        self.J = box.jacobian(T)
        self.Binv = np.linalg.inv(box.blocks(T))
        if T_weight is None or T_weight is T:
            Jw, Bw = self.J, self.Binv
        else:
            Jw, Bw = box.jacobian(T_weight), np.linalg.inv(box.blocks(T_weight))
        self.lam = power_lambda(Jw, lambda r: block_mul(Bw, r), 3)
        self.omega0 = 2.0 / (1.1 * 1.1 * self.lam)
        self.cg_levels = cg_depth(box.axes, box.dt, box.mp["alpha"], mg_levels)
        self.V = vcycle_reference(box.axes, box.vertex_mean(T), box.mp, box.dt, self.cg_levels)

    def smooth(self, r):
        """omega0 B^-1 r: the cycle without its coarse correction"""
        return self.omega0 * block_mul(self.Binv, r)

    def apply(self, r):
        P = self.box.P
        x = self.smooth(r)
        x = x + P @ self.V(P.T @ (r - self.J @ x))
        return x + self.smooth(r - self.J @ x)

    __call__ = apply


def block_mul(Binv, r):
    return np.einsum("eij,ej->ei", Binv, r.reshape(-1, NL)).reshape(-1)
