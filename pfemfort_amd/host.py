"""Host-side bookkeeping of the PFEMFort drivers, through the C ABI (csrc/pfem_host.cpp).

numpy wrappers of the integer/mesh logic the drivers run before the element loop:
mesh files, the structured generator (genTetra.cpp), Dirichlet/DOF
numbering and partition renumbering (tetrapoissonparallelimpl1.F:316-367, 393-734) and
the per-element compat routines (MODULE ElementUtilitiesPoisson / ...Elasticity3D).
Arrays are column-major like the Fortran: ``xyz (ndim, nNode)``, ``conn (npElem, nElem)``,
``edof (nsize, nElem)``, 0-based, -1 = Dirichlet.
"""
from __future__ import annotations

import ctypes as C
import gzip
import os
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# REAL(4) literals of the drivers, widened to double (the reference is built without
# -fdefault-real-8): tetrapoissonparallelimpl1.F:822-823, tetraelasticityparallelimpl1.F:895-902
def _f32(v):
    return float(np.float32(v))


POISSON_ELEMDATA = np.array([1.0, 1.0, 1.0])
ELAST_ELEMDATA = np.array([_f32(240.565), _f32(0.3), 1.0, _f32(0.1), 0.0, 0.0])
TIMEDATA = np.array([0.0, 1.0, 0.0])
# triaelasticityparallelimpl1.F:907 sets only E and nu; thick / bforce are read uninitialised there
# (SURVEY 8f.1): the intended unit thickness and zero body force are used
ELAST2D_ELEMDATA = np.array([_f32(240.565), _f32(0.3), 1.0, 0.0, 0.0])


@dataclass
class Mesh:
    xyz: np.ndarray        # (ndim, nNode)
    conn: np.ndarray       # (npElem, nElem) int32, 0-based, OLD numbering
    bc_node: np.ndarray    # (nDBC,) int32 0-based
    bc_dof: np.ndarray     # (nDBC,) int32 0-based
    bc_val: np.ndarray     # (nDBC,)
    box: tuple | None = None   # (nEx, nEy, nEz) for generated meshes
    force_node: np.ndarray | None = None   # ForceBC file: node (0-based), dof (0-based), value
    force_dof: np.ndarray | None = None
    force_val: np.ndarray | None = None

    @property
    def nNode(self):
        return self.xyz.shape[1]

    @property
    def nElem(self):
        return self.conn.shape[1]


def read_table(path: str) -> np.ndarray:
    """One mesh file -> (rows, cols) float64, parsed by the library's multithreaded ASCII reader."""
    with (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")) as f:
        buf = f.read()
    rows = C.c_int64(0); cols = C.c_int(0)
    L.check(L.lib().pfem_text_table_shape(buf, len(buf), C.byref(rows), C.byref(cols)), f"pfem_text_table_shape({path})")
    out = np.empty((cols.value, rows.value))
    if rows.value == 0:
        return out.T
    L.check(L.lib().pfem_text_table_parse(buf, len(buf), rows.value, cols.value, _p(out)), f"pfem_text_table_parse({path})")
    return out.T


def read_mesh(prefix: str) -> Mesh:
    """``<prefix>-nodes.dat[.gz]``, ``-elems``, ``-DirichBC``: whitespace ASCII, 1-based
    (tetrapoissonparallelimpl1.F:216-355)."""
    def load(kind):
        for ext in (".dat.gz", ".dat"):
            path = f"{prefix}-{kind}{ext}"
            if os.path.exists(path):
                return read_table(path)
        raise FileNotFoundError(f"{prefix}-{kind}.dat[.gz]")
    nodes, elems, bcs = load("nodes"), load("elems"), load("DirichBC")
    # read_table hands back the transpose of a (columns, records) array: slice THAT, so every step below is a
    # contiguous pass (the other order costs seconds at millions of elements)
    conn = elems.T[1:].astype(np.int32)
    conn -= 1
    m = Mesh(np.ascontiguousarray(nodes.T[1:]), conn,
             (bcs[:, 0] - 1).astype(np.int32), (bcs[:, 1] - 1).astype(np.int32), bcs[:, 2].copy())
    try:                                    # optional 4th file (tetraelasticityparallelimpl1.F:207-214)
        fb = load("ForceBC")
        m.force_node, m.force_dof, m.force_val = (fb[:, 0] - 1).astype(np.int32), (fb[:, 1] - 1).astype(np.int32), fb[:, 2].copy()
    except FileNotFoundError:
        pass
    return m


def gen_box_tets(x0, x1, nEx, y0, y1, nEy, z0, z1, nEz, bc_mode=0, ndof=1, kz=None, nodes=True) -> Mesh:
    """genTetra.cpp: structured box, 6 tets per hex.  ``kz=(k0,k1)`` emits only the elements of
    hex layers [k0,k1) (one rank's slab); nodes always cover the full grid."""
    k0, k1 = (0, nEz) if kz is None else kz
    nNode = (nEx + 1) * (nEy + 1) * (nEz + 1)
    nElem = 6 * nEx * nEy * (k1 - k0)
    xyz = np.empty((3, nNode)) if nodes else None
    conn = np.empty((4, nElem), dtype=np.int32)
    n = C.c_int64(0)
    head = (x0, x1, nEx, y0, y1, nEy, z0, z1, nEz, k0, k1, bc_mode, ndof)
    L.check(L.lib().pfem_gen_box_tets(*head, None, None, C.byref(n), None, None, None), "pfem_gen_box_tets")
    bn = np.empty(n.value, np.int32); bd = np.empty(n.value, np.int32); bv = np.empty(n.value)
    L.check(L.lib().pfem_gen_box_tets(*head, _p(xyz), _p(conn), C.byref(n), _p(bn), _p(bd), _p(bv)), "pfem_gen_box_tets")
    return Mesh(xyz, conn, bn, bd, bv, box=(nEx, nEy, nEz))


def box_slab_sizes(nEx, nEy, nEz, bc_mode=0, ndof=1, nparts=1, part=0, axis=2):
    """Closed-form sizes of slab ``part`` of the generated box in the reference's numbering (pfem_box_slab_sizes_axis).
    ``axis``: 0 x, 1 y, 2 z (default), -1: the axis with the most hex layers; the dict also names the axis taken and the
    slab's hex layers."""
    v = [C.c_int64(0) for _ in range(5)]
    w = [C.c_int(0) for _ in range(3)]
    L.check(L.lib().pfem_box_slab_sizes_axis(nEx, nEy, nEz, bc_mode, ndof, axis, nparts, part, *[C.byref(x) for x in v + w]),
            "pfem_box_slab_sizes_axis")
    keys = ("size_global", "row_start", "size_local", "nNode_local", "nElem_local", "axis", "layer0", "layer1")
    return {k: x.value for k, x in zip(keys, v + w)}


def partition_box_slabs(nEx, nEy, nEz, nParts, elements=True, axis=2):
    """Deterministic stand-in for METIS_PartMeshNodal (:464) on generated boxes: slabs of hex layers along ``axis``
    (-1: the longest).  ``elements=False`` skips the (large) elem_proc_id array and returns None for it."""
    epid = np.empty(6 * nEx * nEy * nEz, np.int32) if elements else None
    npid = np.empty((nEx + 1) * (nEy + 1) * (nEz + 1), np.int32)
    L.check(L.lib().pfem_partition_box_slabs_axis(nEx, nEy, nEz, axis, nParts, _p(epid), _p(npid)), "pfem_partition_box_slabs_axis")
    return epid, npid


def partition_rcb(mesh, nParts):
    """(elem_proc_id, node_proc_id) by recursive coordinate bisection of the element centroids: a geometric stand-in
    for METIS_PartMeshNodal (:464) on any mesh with coordinates."""
    xyz = _f64(mesh.xyz); conn = _i32(mesh.conn)
    epid = np.empty(conn.shape[1], np.int32); npid = np.empty(xyz.shape[1], np.int32)
    L.check(L.lib().pfem_partition_rcb(xyz.shape[1], xyz.shape[0], _p(xyz), conn.shape[1], conn.shape[0], _p(conn), nParts,
                                       _p(epid), _p(npid)), "pfem_partition_rcb")
    return epid, npid


def read_metis_partition(prefix: str, nParts: int):
    """(elem_proc_id, node_proc_id) from the files METIS' ``mpmetis <mesh> nParts`` writes
    (``<prefix>.epart.<nParts>`` / ``<prefix>.npart.<nParts>``, one 0-based part per line): the
    file hook for ``METIS_PartMeshNodal`` (tetrapoissonparallelimpl1.F:464), which is not installed here."""
    out = []
    for kind in ("epart", "npart"):
        t = read_table(f"{prefix}.{kind}.{nParts}")
        if t.ndim != 2 or t.shape[1] != 1:
            raise ValueError(f"{prefix}.{kind}.{nParts}: expected one part id per line")
        ids = t[:, 0].astype(np.int32)
        if len(ids) and (ids.min() < 0 or ids.max() >= nParts or np.any(ids != t[:, 0])):
            raise ValueError(f"{prefix}.{kind}.{nParts}: part id out of range")
        out.append(ids)
    return out[0], out[1]


@dataclass
class DofMap:
    node_map_get_old: np.ndarray
    node_map_get_new: np.ndarray
    NodeDofArrayNew: np.ndarray     # (nNode, ndof) 0-based ids, -1 = Dirichlet
    solnApplied: np.ndarray         # (nNode*ndof,) by NEW node*ndof+d
    node_start: np.ndarray
    node_end: np.ndarray
    row_start: np.ndarray
    row_end: np.ndarray
    size_global: int


def dof_numbering(nNode, ndof, bc_node, bc_dof, bc_val, nParts=1, node_proc_id=None) -> DofMap:
    old = np.empty(nNode, np.int32); new = np.empty(nNode, np.int32)
    nda = np.empty((nNode, ndof), np.int32); sa = np.empty(nNode * ndof)
    ns, ne, rs, re = (np.zeros(nParts, np.int64) for _ in range(4))
    sg = C.c_int64(0)
    npid = None if node_proc_id is None else _i32(node_proc_id)
    L.check(L.lib().pfem_dof_numbering(nNode, ndof, len(bc_node), _p(_i32(bc_node)), _p(_i32(bc_dof)), _p(_f64(bc_val)),
                                       nParts, _p(npid), _p(old), _p(new), _p(nda), _p(sa), _p(ns), _p(ne), _p(rs),
                                       _p(re), C.byref(sg)), "pfem_dof_numbering")
    return DofMap(old, new, nda, sa, ns, ne, rs, re, sg.value)


def renumber_mesh(mesh, dm: DofMap):
    """Connectivity and coordinates in the NEW node numbering: ``elemNodeConn = node_map_get_new(.)``
    (tetrapoissonparallelimpl1.F:659-664) and ``coords(node_map_get_old(.))`` (:832-838)."""
    conn = _i32(mesh.conn); xyz = _f64(mesh.xyz)
    conn_new = np.empty(conn.shape, np.int32)
    xyz_new = np.empty(xyz.shape, np.float64)
    L.check(L.lib().pfem_renumber_mesh(xyz.shape[1], xyz.shape[0], conn.shape[1], conn.shape[0], _p(conn), _p(xyz),
                                       _p(_i32(dm.node_map_get_new)), _p(_i32(dm.node_map_get_old)), _p(conn_new),
                                       _p(xyz_new)), "pfem_renumber_mesh")
    return conn_new, xyz_new


def elem_dof_array(conn_new, NodeDofArrayNew):
    conn_new = _i32(conn_new)
    npE, nElem = conn_new.shape
    ndof = NodeDofArrayNew.shape[1]
    edof = np.empty((npE * ndof, nElem), np.int32)
    L.check(L.lib().pfem_elem_dof_array(nElem, npE, ndof, _p(conn_new), _p(_i32(NodeDofArrayNew)), _p(edof)),
            "pfem_elem_dof_array")
    return edof


def assy_for_soln(NodeDofArrayNew):
    nNode, ndof = NodeDofArrayNew.shape
    out = np.empty(int((NodeDofArrayNew >= 0).sum()), np.int32)
    L.check(L.lib().pfem_assy_for_soln(nNode, ndof, _p(_i32(NodeDofArrayNew)), _p(out)), "pfem_assy_for_soln")
    return out


# ---- per-element compat routines (one element per call, like the Fortran) -----------
def StiffnessResidualPoissonLinearTetra(xNode, yNode, zNode, elemData, timeData, valC, valDotC=None):
    """elementutilitiespoisson.F:107; returns (Klocal[4,4], Flocal[4])."""
    K = np.empty((4, 4), order="F"); F = np.empty(4)
    L.check(L.lib().pfem_poisson_tet_ke(_p(_f64(xNode)), _p(_f64(yNode)), _p(_f64(zNode)), _p(_f64(elemData)),
                                        _p(_f64(timeData)), _p(_f64(valC)), _p(K), _p(F)),
            "StiffnessResidualPoissonLinearTetra")
    return K, F


def StiffnessResidualPoissonLinearTria(xNode, yNode, elemData, timeData, valC, valDotC=None):
    """elementutilitiespoisson.F:23; returns (Klocal[3,3], Flocal[3])."""
    K = np.empty((3, 3), order="F"); F = np.empty(3)
    L.check(L.lib().pfem_poisson_tria_ke(_p(_f64(xNode)), _p(_f64(yNode)), _p(_f64(elemData)), _p(_f64(timeData)),
                                         _p(_f64(valC)), _p(K), _p(F)), "StiffnessResidualPoissonLinearTria")
    return K, F


def StiffnessResidualElasticityLinearTetra(xNode, yNode, zNode, elemData, timeData, valC, valDotC=None):
    """elementutilitieselasticity3D.F:248 (intended semantics); returns (Klocal[12,12], Flocal[12])."""
    K = np.empty((12, 12), order="F"); F = np.empty(12)
    L.check(L.lib().pfem_elast_tet_ke(_p(_f64(xNode)), _p(_f64(yNode)), _p(_f64(zNode)), _p(_f64(elemData)),
                                      _p(_f64(timeData)), _p(_f64(valC)), _p(K), _p(F)),
            "StiffnessResidualElasticityLinearTetra")
    return K, F


def StiffnessResidualElasticityLinearTria(xNode, yNode, elemData, timeData, valC, valDotC=None):
    """elementutilitieselasticity2D.F:23; returns (Klocal[6,6], Flocal[6])."""
    K = np.empty((6, 6), order="F"); F = np.empty(6)
    L.check(L.lib().pfem_elast_tria_ke(_p(_f64(xNode)), _p(_f64(yNode)), _p(_f64(elemData)), _p(_f64(timeData)),
                                       _p(_f64(valC)), _p(K), _p(F)), "StiffnessResidualElasticityLinearTria")
    return K, F


def ElementPost(kind, xNode, yNode, zNode, elemData, valC):
    """Post-processing of one element (pfem_elem_post; the grad u -> strain -> stress -> B^T sigma chain of
    ResidualElasticityLinearTetra, elementutilitieselasticity3D.F:575-723, consistent with Klocal): returns
    ``(grad[ng], flux[ng], scalar, fint[nsize])`` -- gradient / engineering Voigt strain, flux / stress, ``|q|`` / von Mises,
    internal nodal forces ``= Klocal @ valC`` to rounding.  ``zNode`` is None in 2-D."""
    ng = L.NG[kind]
    grad = np.empty(ng); flux = np.empty(ng); sc = C.c_double(0); fint = np.empty(L.NPELEM[kind] * L.NDOF[kind])
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    L.check(L.lib().pfem_elem_post(kind, _p(_f64(xNode)), _p(_f64(yNode)), _p(z), _p(ed), _p(_f64(valC)), _p(grad), _p(flux),
                                   C.byref(sc), _p(fint)), "pfem_elem_post")
    return grad, flux, sc.value, fint


def MassMatrixLinear(kind, xNode, yNode, zNode, elemData, density):
    """Lumped mass of one element (pfem_elem_lumped_mass; MassMatrixLinearTria / MassMatrixLinearTetra,
    elementutilitieselasticity2D.F:283, 3D.F:401): the row sums of the consistent mass at the one Gauss point, ``Mlocal[nsize]``.
    ``density`` is an argument of its own; ``elemData`` gives the thickness of ``ELAST_TRIA`` and may be None otherwise."""
    M = np.empty(L.NPELEM[kind] * L.NDOF[kind])
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    L.check(L.lib().pfem_elem_lumped_mass(kind, _p(_f64(xNode)), _p(_f64(yNode)), _p(z), _p(ed), float(density), _p(M)),
            "pfem_elem_lumped_mass")
    return M


def FaceLoad(kind, xNode, yNode, zNode, side, load=None, values=None, elemData=None):
    """One side of one element (pfem_face_load): side ``f`` is the face / edge opposite local node ``f``.  Returns
    ``(F[nsize], measure, normal[ndim])`` -- the consistent nodal load of ``values`` ((npe-1, ncomp), per side node in ascending
    local order; zeros at the opposite node's dofs), the side's area / length and the element's outward unit normal.  With
    ``load=None`` only the geometry is computed and ``F`` is None.  ``load``: ``LOAD_FLUX`` (Poisson kinds), ``LOAD_TRACTION``,
    ``LOAD_PRESSURE`` (elasticity kinds); ``elemData`` is read for the plane-stress triangle only (thickness).  ``zNode`` is
    None in 2-D."""
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    F = None if load is None else np.empty(L.NPELEM[kind] * L.NDOF[kind])
    v = None if values is None else _f64(values).ravel()
    meas = C.c_double(0); nrm = np.empty(L.NDIM[kind])
    L.check(L.lib().pfem_face_load(kind, _p(_f64(xNode)), _p(_f64(yNode)), _p(z), int(side), 0 if load is None else int(load),
                                   _p(v), _p(ed), _p(F), C.byref(meas), _p(nrm)), "pfem_face_load")
    return F, meas.value, nrm


def ThermalLoad(kind, xNode, yNode, zNode, elemData, alpha, theta):
    """Thermal load of one element of an elasticity kind (pfem_elem_thermal_load): ``theta (npe,)`` = T - T_ref at its nodes,
    the thermal strain ``e_th = alpha * sum_a N_a theta_a`` constant over the element.  Returns ``(F[nsize], sigma_th[ng])`` --
    ``dvol B^T D eps_th`` and ``D eps_th``.  ``zNode`` is None in 2-D."""
    if kind not in L.NG:                                     # the library says so
        L.check(L.lib().pfem_elem_thermal_load(int(kind), None, None, None, None, 0.0, None, None, None), "pfem_elem_thermal_load")
    F = np.empty(L.NPELEM[kind] * L.NDOF[kind]); sg = np.empty(L.NG[kind])
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    th = None if theta is None else _f64(theta).ravel()
    L.check(L.lib().pfem_elem_thermal_load(kind, _p(_f64(xNode)), _p(_f64(yNode)), _p(z), _p(ed), float(alpha), _p(th), _p(F), _p(sg)),
            "pfem_elem_thermal_load")
    return F, sg


def GeometricStiffness(kind, xNode, yNode, zNode, elemData, sigma):
    """Geometric stiffness of one element of an elasticity kind under the stress ``sigma`` (pfem_elem_geometric), in the order
    ``ElementPost`` returns ``flux``: the ``npe x npe`` scalars ``g[a, b] = dvol (grad N_a . sigma grad N_b)``;
    ``K_g[(a,i),(b,j)] = delta_ij g[a, b]``.  ``elemData`` gives the thickness of ``ELAST_TRIA`` and may be None for the tet."""
    npe = L.NPELEM.get(kind, 4)
    g = np.empty(npe * npe)
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    sg = None if sigma is None else _f64(sigma).ravel()
    L.check(L.lib().pfem_elem_geometric(int(kind), _p(_f64(xNode)), _p(_f64(yNode)), _p(z), _p(ed), _p(sg), _p(g)), "pfem_elem_geometric")
    return g.reshape(npe, npe).T                             # (g[a + npe b])


def ElementPostThermal(kind, xNode, yNode, zNode, elemData, valC, alpha, theta):
    """``ElementPost`` of an elasticity kind under a thermal state (pfem_elem_post_thermal): the stress is
    ``D (strain - eps_th)``, von Mises and ``fint`` are formed from it, ``grad`` stays the total strain."""
    ng = L.NG[kind]
    grad = np.empty(ng); flux = np.empty(ng); sc = C.c_double(0); fint = np.empty(L.NPELEM[kind] * L.NDOF[kind])
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    L.check(L.lib().pfem_elem_post_thermal(kind, _p(_f64(xNode)), _p(_f64(yNode)), _p(z), _p(ed), _p(_f64(valC)), float(alpha),
                                           _p(_f64(theta).ravel()), _p(grad), _p(flux), C.byref(sc), _p(fint)), "pfem_elem_post_thermal")
    return grad, flux, sc.value, fint


def PostScalar(kind, flux):
    """The scalar of ``ElementPost`` on any flux / stress vector(s) of the kind, ``(ng,)`` or ``(n, ng)`` in the stored Voigt
    order (pfem_post_scalar): ``|q|``, von Mises, the plane-stress form."""
    f = _f64(flux)
    rows = f.reshape(-1, L.NG[kind])
    out = np.empty(rows.shape[0])
    sc = C.c_double(0)
    for i, r in enumerate(rows):
        L.check(L.lib().pfem_post_scalar(kind, _p(np.ascontiguousarray(r)), C.byref(sc)), "pfem_post_scalar")
        out[i] = sc.value
    return float(out[0]) if f.ndim == 1 else out


def ElementRecoveryError(kind, xNode, yNode, zNode, elemData, valC, nodal_flux):
    """One element's share of the Zienkiewicz-Zhu indicator (pfem_elem_recovery_error): ``nodal_flux (npe, ng)`` are the
    recovered values at the element's nodes; returns ``(eta2, flux_norm2)``."""
    z = None if zNode is None else _f64(zNode)
    ed = None if elemData is None else _f64(elemData)
    nf = _f64(nodal_flux).ravel()
    assert nf.size == L.NPELEM[kind] * L.NG[kind]
    e2 = C.c_double(0); f2 = C.c_double(0)
    L.check(L.lib().pfem_elem_recovery_error(kind, _p(_f64(xNode)), _p(_f64(yNode)), _p(z), _p(ed), _p(_f64(valC)), _p(nf),
                                             C.byref(e2), C.byref(f2)), "pfem_elem_recovery_error")
    return e2.value, f2.value


def find_ghosts(edof, row_start, n_owned):
    """Ascending unique global dof ids of ``edof`` outside the owned block (host-only)."""
    e = _i32(edof).ravel()
    n = C.c_int64(0)
    L.check(L.lib().pfem_find_ghosts(e.size, _p(e), row_start, n_owned, C.byref(n), None), "pfem_find_ghosts")
    g = np.empty(n.value, np.int64)
    L.check(L.lib().pfem_find_ghosts(e.size, _p(e), row_start, n_owned, C.byref(n), _p(g)), "pfem_find_ghosts")
    return g


def neighbour_plan(rank, row_ranges, ghost_lists):
    """The neighbour plan of ``rank`` (include/pfem_amd.h, section 5; host-only integer logic):
    ``row_ranges[r] = (row_start, row_end)`` and ``ghost_lists[r]`` = ascending global ghost dof ids of rank r.
    Returns (peers int32[n], peer_off int64[n+1], shared_gid int64[peer_off[-1]])."""
    world = len(row_ranges)
    rs = np.ascontiguousarray([r[0] for r in row_ranges], dtype=np.int64)
    re = np.ascontiguousarray([r[1] for r in row_ranges], dtype=np.int64)
    lists = [np.ascontiguousarray(g, dtype=np.int64) for g in ghost_lists]
    off = np.zeros(world + 1, np.int64)
    off[1:] = np.cumsum([len(g) for g in lists])
    allg = np.ascontiguousarray(np.concatenate(lists + [np.empty(0, np.int64)]))
    npeers = C.c_int(0); total = C.c_int64(0)
    L.check(L.lib().pfem_neighbour_plan(world, rank, _p(rs), _p(re), _p(off), _p(allg), C.byref(npeers), C.byref(total),
                                        None, None, None), "pfem_neighbour_plan")
    peers = np.zeros(npeers.value, np.int32); poff = np.zeros(npeers.value + 1, np.int64); gid = np.zeros(total.value, np.int64)
    if npeers.value:
        L.check(L.lib().pfem_neighbour_plan(world, rank, _p(rs), _p(re), _p(off), _p(allg), C.byref(npeers), C.byref(total),
                                            _p(peers), _p(poff), _p(gid)), "pfem_neighbour_plan")
    return peers, poff, gid


def write_temp_dat(path, val, ii=None, ind=None):
    """The drivers' ``temp.dat`` dump (tetrapoissonparallelimpl1.F:935-942; value-only form :1031-1046 of the
    elasticity driver when ``ii``/``ind`` are None)."""
    val = _f64(val)
    if ii is not None:
        ii = np.ascontiguousarray(ii, dtype=np.int64); ind = np.ascontiguousarray(ind, dtype=np.int64)
    L.check(L.lib().pfem_write_temp_dat(str(path).encode(), val.size, _p(ii), _p(ind), _p(val)), "pfem_write_temp_dat")


def writeoutputvtk(ndim, coords, elemNodeConn, elem_procid, soln, fileName, ndof=None):
    """MODULE WriterVTK: writeoutputvtk (writervtk.F:33).  ``coords (ndim,nNode)``, ``elemNodeConn
    (npElem,nElem)`` 0-based, ``soln (nNode, ndof)`` or flat by node id."""
    coords = _f64(coords); conn = _i32(elemNodeConn); pid = _i32(elem_procid)
    soln = _f64(soln)
    nNode, nElem = coords.shape[1], conn.shape[1]
    if ndof is None:
        ndof = soln.size // nNode
    L.check(L.lib().pfem_write_vtk(str(fileName).encode(), ndim, nElem, nNode, conn.shape[0], ndof, _p(coords), _p(conn),
                                   _p(pid), _p(soln.ravel())), "writeoutputvtk")


def _vtk_array(name, a, n):
    """One extra array of the writer as (n, ncomp)."""
    a = _f64(a)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.shape[0] != n:
        raise ValueError(f"{name}: {a.shape[0]} items, expected {n}")
    return a


def voigt_to_tensor(v):
    """``(n, 6)`` [xx,yy,zz,xy,yz,zx] or ``(n, 3)`` [xx,yy,xy] (components as stored) -> ``(n, 9)`` symmetric 3x3, row-major."""
    v = _f64(v)
    t = np.zeros((v.shape[0], 9))
    if v.shape[1] == 6:
        xx, yy, zz, xy, yz, zx = v.T
        t[:, 0], t[:, 4], t[:, 8] = xx, yy, zz
        t[:, 1] = t[:, 3] = xy
        t[:, 5] = t[:, 7] = yz
        t[:, 2] = t[:, 6] = zx
    elif v.shape[1] == 3:
        t[:, 0], t[:, 4] = v[:, 0], v[:, 1]
        t[:, 1] = t[:, 3] = v[:, 2]
    else:
        raise ValueError("Voigt vectors have 3 or 6 components")
    return t


def writeoutputvtk_fields(ndim, coords, elemNodeConn, elem_procid, soln, fileName, ndof=None, cell_fields=None, point_fields=None,
                          voigt=()):
    """``writeoutputvtk``'s file with further arrays (pfem_write_vtk_fields): ``cell_fields`` / ``point_fields`` map a name to
    ``(n,)`` scalars, ``(n, 3)`` vectors (``(n, 2)``: padded with a zero), ``(n, 6)`` Voigt [xx,yy,zz,xy,yz,zx] -- written as a
    symmetric 3x3 tensor -- or ``(n, 9)``.  A name in ``voigt`` marks an ``(n, 3)`` array as plane Voigt [xx,yy,xy] instead of
    a vector.  Without fields the bytes are ``writeoutputvtk``'s."""
    coords = _f64(coords); conn = _i32(elemNodeConn); pid = _i32(elem_procid)
    soln = _f64(soln)
    nNode, nElem = coords.shape[1], conn.shape[1]
    if ndof is None:
        ndof = soln.size // nNode

    def pack(fields, n):
        names, ncomp, arrays = [], [], []
        for name, a in (fields or {}).items():
            a = _vtk_array(name, a, n)
            if a.shape[1] == 6 or (a.shape[1] == 3 and name in voigt):
                a = voigt_to_tensor(a)
            elif a.shape[1] == 2:
                a = np.concatenate([a, np.zeros((n, 1))], axis=1)
            names.append(str(name).encode()); ncomp.append(a.shape[1]); arrays.append(np.ascontiguousarray(a))
        k = len(names)
        return (k, (C.c_char_p * max(k, 1))(*names), (C.c_int * max(k, 1))(*ncomp),
                (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in arrays]), arrays)

    nc, cn, cc, cd, keep_c = pack(cell_fields, nElem)
    npt, pn, pc, pd, keep_p = pack(point_fields, nNode)
    L.check(L.lib().pfem_write_vtk_fields(str(fileName).encode(), ndim, nElem, nNode, conn.shape[0], ndof, _p(coords), _p(conn),
                                          _p(pid), _p(soln.ravel()), nc, C.cast(cn, C.c_void_p), C.cast(cc, C.c_void_p),
                                          C.cast(cd, C.c_void_p), npt, C.cast(pn, C.c_void_p), C.cast(pc, C.c_void_p),
                                          C.cast(pd, C.c_void_p)), "writeoutputvtk_fields")
