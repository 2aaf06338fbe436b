"""Facet analysis of general quadrilateral / hexahedral meshes (tv_um_facets,
UnstructuredMesh.facets): what the SIPG form of a DG temperature needs from the
mesh, on the host, against the oracle's facet_topology and its Newton inverse
map (oracle/tv_oracle.py HeatForm._inverse_map).

``orient`` lets the assembly place the '-' reference point of a '+' Gauss point
from the vertex correspondence alone: the trace of a Q1 map on a facet is the
bilinear map of the facet's own vertices, so on a conforming mesh the two
cells' maps agree on the facet once the tangential coordinates are matched.
Tolerances: the same physical point from both cells to 1e-14 x the mesh extent
(two bilinear interpolations of the same four vertices in float64); the
oracle's Newton iteration stops at |dxi| < 1e-15, its result is compared to
1e-12.
"""
import numpy as np
import pytest

from oracle import tv_oracle as O

MESHES = {
    "quad": ((9, 8), (3.0, 2.0), True),
    "hex": ((7, 5, 4), (2.0, 2.0, 1.0), True),
    # numbered plane by plane (not shuffled), as gmsh and the box meshes number them
    "hex_ordered": ((7, 5, 4), (2.0, 2.0, 1.0), False),
}


def make_mesh(name):
    from tvfem import distorted_box_mesh
    n, L, shuffle = MESHES[name]
    return distorted_box_mesh(L, n, amp=0.2, seed=0, shuffle=shuffle)


def oracle_mesh(m):
    return O.Mesh(dim=m.dim, x=m.x[:, :m.dim].copy(), cells=m.cells.copy())


def tangential(d, lf):
    return [a for a in range(d) if a != lf // 2]


def minus_points(d, lfp, lfm, orient, q):
    """Cell reference coordinates on both sides of facet points q (nq, d - 1) given
    in the '+' facet's tangential coordinates."""
    xp = O._facet_ref_points(d, lfp, q)
    xm = np.zeros_like(xp)
    xm[:, lfm // 2] = float(lfm % 2)
    tm = tangential(d, lfm)
    for k in range(d - 1):
        o = (orient >> (2 * k)) & 3
        xm[:, tm[o & 1]] = 1.0 - q[:, k] if o & 2 else q[:, k]
    return xp, xm


@pytest.mark.parametrize("name", list(MESHES))
def test_facets_match_oracle_topology_and_inverse_map(name):
    m = make_mesh(name)
    om = oracle_mesh(m)
    d = m.dim
    ext, inter = m.facets()
    o_ext, o_int = O.facet_topology(om)
    assert ext.dtype == np.int64 and ext.shape == o_ext.shape and np.array_equal(ext, o_ext)
    assert inter.shape == (len(o_int), 5)
    assert {tuple(r) for r in inter[:, :4].tolist()} == {tuple(r) for r in o_int.tolist()}
    assert len({tuple(r) for r in inter[:, :4].tolist()}) == len(inter)
    # ascending in (cell+, lf+), '+' the lower cell index
    key = inter[:, 0] * 8 + inter[:, 1]
    assert np.all(np.diff(key) > 0) and np.all(inter[:, 0] < inter[:, 2])
    form = O.HeatForm(O.Space(om, "CG"), 0.1, O.ThermalParams.from_dict(O.MAIN_MODEL_PARAMS))
    q, _ = O.tensor_rule(d - 1, 3)
    extent = float(np.ptp(om.x, axis=0).max())
    worst_x = worst_xi = 0.0
    for cp, lfp, cm, lfm, orient in inter.tolist():
        xp, xm = minus_points(d, lfp, lfm, orient, q)
        Xp = O.q1_basis(xp)[0] @ om.x[om.cells[cp]]
        Xm = O.q1_basis(xm)[0] @ om.x[om.cells[cm]]
        worst_x = max(worst_x, float(np.abs(Xp - Xm).max()))
        worst_xi = max(worst_xi, float(np.abs(form._inverse_map(cm, Xp, lfm) - xm).max()))
    print(f"[facets] {name}: {len(inter)} interior facets, physical points differ by {worst_x:.2e} "
          f"(extent {extent:g}), inverse map by {worst_xi:.2e}")
    assert worst_x <= 1e-14 * extent
    assert worst_xi <= 1e-12


def test_rectilinear_grid_pairs_opposite_facets_with_identity_orientation():
    from tvfem import RectilinearMesh, UnstructuredMesh
    axes = [np.linspace(0.0, 2.0, 9) ** 1.3, np.linspace(0.0, 1.5, 7), np.array([0.0, 0.2, 0.5, 1.0])]
    m = UnstructuredMesh.from_rectilinear(RectilinearMesh(axes))
    ext, inter = m.facets()
    n = [len(a) - 1 for a in axes]
    assert len(inter) == (n[0] - 1) * n[1] * n[2] + n[0] * (n[1] - 1) * n[2] + n[0] * n[1] * (n[2] - 1)
    assert len(ext) == 2 * (n[0] * n[1] + n[0] * n[2] + n[1] * n[2])
    a = inter[:, 1] // 2
    assert np.array_equal(inter[:, 1], 2 * a + 1) and np.array_equal(inter[:, 3], 2 * a)
    # identity: tangential axis 0 along axis 0, axis 1 along axis 1, neither reversed
    assert np.all(inter[:, 4] == 0b0100)
    stride = np.array([1, n[0], n[0] * n[1]])
    assert np.array_equal(inter[:, 2] - inter[:, 0], stride[a])


def test_three_cells_on_one_facet_are_refused_and_counts_work():
    import ctypes as C

    from tvfem import UnstructuredMesh
    from tvfem import _native as N
    m = make_mesh("hex")
    lib = N.load_library()

    def counts(mesh):
        desc = N.UMeshDesc()
        desc.dim = mesh.dim
        xyz, cells = np.ascontiguousarray(mesh.x), np.ascontiguousarray(mesh.cells, dtype=np.int64)
        desc.n_vertices, desc.n_cells = xyz.shape[0], cells.shape[0]
        desc.coords = xyz.ctypes.data_as(C.POINTER(C.c_double))
        desc.cells = cells.ctypes.data_as(C.POINTER(C.c_int64))
        ni, ne = C.c_int64(-1), C.c_int64(-1)
        rc = lib.tv_um_facets(C.byref(desc), C.byref(ni), None, C.byref(ne), None)
        return rc, ni.value, ne.value

    ext, inter = m.facets()
    assert counts(m) == (N.TV_OK, len(inter), len(ext))
    # an interior cell twice: each of its interior facets now belongs to three cells
    e = int(inter[len(inter) // 2, 0])
    bad = UnstructuredMesh(3, m.x, np.vstack([m.cells, m.cells[e:e + 1]]))
    rc, _, _ = counts(bad)
    assert rc == N.TV_ERR_ARG
    assert b"more than two cells" in lib.tv_last_error(None)
    with pytest.raises(N.NativeError) as ei:
        bad.facets()
    assert ei.value.code == N.TV_ERR_ARG
    # two cells glued at a facet's vertices with the facet twisted: not a facet of both
    c = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 7, 6, 8, 9, 10, 11]])
    x = np.zeros((12, 3))
    x[:, :] = [[i & 1, (i >> 1) & 1, i >> 2] for i in range(12)]
    with pytest.raises(N.NativeError) as ei:
        UnstructuredMesh(3, x, c).facets()
    assert ei.value.code == N.TV_ERR_ARG and "not a facet of both" in str(ei.value)
