"""numpy mirror of the surface loads (pfem_mesh_boundary_faces / pfem_surface_geometry / pfem_face_load /
pfem_rhs_add_surface_load): boundary sides by counting sorted node tuples, geometry and consistent nodal loads in the written
order of operations of csrc/pfem_elem.hpp (numpy's elementwise double arithmetic does not contract, and its sqrt and division are
IEEE: the same bits where the library keeps its word), and the load vector in the free-dof numbering of ``drivers._setup``.

Side ``f`` of an element is the face (tets) / edge (triangles) opposite local node ``f``; its nodes are the element's other
local nodes in ascending local order."""
import numpy as np

EPS = np.finfo(np.float64).eps
LOAD_FLUX, LOAD_TRACTION, LOAD_PRESSURE = 1, 2, 3
UNIFORM, PER_FACE, PER_FACE_NODE = 0, 1, 2
NPE = {1: 3, 2: 4, 3: 4, 4: 3, 5: 3}
NDOF = {1: 1, 2: 1, 3: 3, 4: 1, 5: 2}


def side_local_nodes(npe):
    """(npe, npe-1): row f = the local nodes of side f, ascending."""
    return np.array([[a for a in range(npe) if a != f] for f in range(npe)])


def boundary_sides(conn):
    """``(elem, side)`` int32 of the sides whose sorted node tuple occurs exactly once, sorted by (element, side)."""
    npe, nElem = conn.shape
    loc = side_local_nodes(npe)
    tuples = np.sort(conn[loc], axis=1)                       # (npe sides, npe-1 nodes, nElem)
    flat = tuples.transpose(0, 2, 1).reshape(npe * nElem, npe - 1)
    _, inv, cnt = np.unique(flat, axis=0, return_inverse=True, return_counts=True)
    once = (cnt[inv.ravel()] == 1).reshape(npe, nElem)         # [side, elem]
    e, f = np.nonzero(once.T)                                 # ascending element, then side
    return e.astype(np.int32), f.astype(np.int32)


def geometry(xyz, conn, elem, side):
    """measure (n,), normal (ndim, n), nodes (npe-1, n), and what the error bounds are made of: ``mabs`` >= measure, the same
    expression over the absolute values of the products (the cross product's terms before they cancel).  Written order:
      tet   e1 = P1 - P0, e2 = P2 - P0, c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), len = sqrt((cx^2 + cy^2) + cz^2),
            measure = 0.5 len, d = ((Po - P0)x cx + (..)y cy) + (..)z cz
      tria  t = P1 - P0, c = (ty, -tx), len = sqrt(tx^2 + ty^2), measure = len, d = (Po - P0)x cx + (..)y cy
      n = c / len when d < 0, (-c) / len when d > 0 (away from the opposite node Po)."""
    elem = np.asarray(elem, np.int64); side = np.asarray(side, np.int64)
    npe = conn.shape[0]
    loc = side_local_nodes(npe)[side]                         # (n, npe-1)
    nodes = conn[loc.T, elem[None, :]]                        # (npe-1, n)
    P = xyz[:, nodes]                                         # (ndim, npe-1, n)
    Po = xyz[:, conn[side, elem]]                             # (ndim, n)
    if npe == 4:
        e1 = P[:, 1] - P[:, 0]; e2 = P[:, 2] - P[:, 0]
        cx = e1[1] * e2[2] - e1[2] * e2[1]
        cy = e1[2] * e2[0] - e1[0] * e2[2]
        cz = e1[0] * e2[1] - e1[1] * e2[0]
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        meas = 0.5 * ln
        w = Po - P[:, 0]
        d = (w[0] * cx + w[1] * cy) + w[2] * cz
        c = np.array([cx, cy, cz])
        ax = np.abs(e1[1] * e2[2]) + np.abs(e1[2] * e2[1])
        ay = np.abs(e1[2] * e2[0]) + np.abs(e1[0] * e2[2])
        az = np.abs(e1[0] * e2[1]) + np.abs(e1[1] * e2[0])
        mabs = 0.5 * np.sqrt(ax * ax + ay * ay + az * az)
    else:
        t = P[:, 1] - P[:, 0]
        c = np.array([t[1], -t[0]])
        ln = np.sqrt(t[0] * t[0] + t[1] * t[1])
        meas = ln
        w = Po - P[:, 0]
        d = w[0] * c[0] + w[1] * c[1]
        mabs = ln.copy()
    assert np.all(ln > 0) and np.all(d != 0), "a degenerate side"
    c = np.where(d > 0, -c, c)
    return meas, c / ln, nodes.astype(np.int32), mabs


def expand_values(values, layout, n, ns, ncomp):
    """values of any layout as (n, ns, ncomp)."""
    v = np.asarray(values, np.float64)
    if layout == UNIFORM:
        return np.broadcast_to(v.reshape(1, 1, ncomp), (n, ns, ncomp)).copy()
    if layout == PER_FACE:
        return np.broadcast_to(v.reshape(n, 1, ncomp), (n, ns, ncomp)).copy()
    return v.reshape(n, ns, ncomp).copy()


def load_components(kind, load):
    elast = kind in (3, 5)
    if load == LOAD_FLUX:
        return 0 if elast else 1
    if load == LOAD_TRACTION:
        return NDOF[kind] if elast else 0
    if load == LOAD_PRESSURE:
        return 1 if elast else 0
    return 0


def consistent_loads(kind, load, meas, normal, vals, thick=1.0):
    """``Fs (n, ns, ndof)`` and ``T (n, ns, ndof)``, the same expression over absolute values (the Sigma |terms| of the bounds):
      tet   F_a = (A * ((2 g_a + g_b) + g_c)) / 12        tria  F_a = ((L * thick) * (2 g_a + g_b)) / 6
    b, c the side's other nodes ascending; a pressure is the traction g_a,c = -(p_a n_c).  ``vals (n, ns, ncomp)``; ``thick``
    a scalar or (n,)."""
    npe, ndof = NPE[kind], NDOF[kind]
    ns = npe - 1
    n = len(meas)
    assert load_components(kind, load) == vals.shape[2] and vals.shape[:2] == (n, ns)
    if load == LOAD_PRESSURE:
        g = -(vals[:, :, 0][:, :, None] * normal.T[:, None, :])           # (n, ns, ndof)
    else:
        g = vals
    ga = np.abs(vals) if load != LOAD_PRESSURE else np.abs(vals[:, :, 0])[:, :, None] * np.ones((1, 1, ndof))
    m = meas if npe == 4 else meas * thick
    m = np.asarray(m)[:, None]
    Fs = np.empty((n, ns, ndof)); T = np.empty((n, ns, ndof))
    for a in range(ns):
        o = [b for b in range(ns) if b != a]
        s = 2.0 * g[:, a] + g[:, o[0]]
        sa = 2.0 * ga[:, a] + ga[:, o[0]]
        if ns == 3:
            s = s + g[:, o[1]]
            sa = sa + ga[:, o[1]]
        div = 12.0 if npe == 4 else 6.0
        Fs[:, a] = (m * s) / div
        T[:, a] = (np.abs(m) * sa) / div
    return Fs, T


def face_load(kind, x, y, z, side, load, values, thick=1.0):
    """pfem_face_load's outputs for one element: ``F[nsize]`` (zeros at the opposite node), measure, normal[ndim], and the
    bounds' ingredients ``T[nsize]`` and ``mabs``."""
    npe, ndof = NPE[kind], NDOF[kind]
    xyz = np.array([x, y] if z is None else [x, y, z], dtype=np.float64)
    conn = np.arange(npe).reshape(npe, 1)
    meas, nrm, nodes, mabs = geometry(xyz, conn, [0], [side])
    ncomp = load_components(kind, load)
    Fs, T = consistent_loads(kind, load, meas, nrm, np.asarray(values, np.float64).reshape(1, npe - 1, ncomp), thick)
    F = np.zeros(npe * ndof); Tf = np.zeros(npe * ndof)
    for a, nd in enumerate(nodes[:, 0]):
        F[nd * ndof:(nd + 1) * ndof] = Fs[0, a]
        Tf[nd * ndof:(nd + 1) * ndof] = T[0, a]
    return F, meas[0], nrm[:, 0], Tf, mabs[0]


def rollers(xyz):
    """(bc_node, bc_dof, bc_val): u_d = 0 on the plane x_d = 0 for every axis d -- the symmetry planes of a uniaxial or
    hydrostatic state."""
    bn, bd = [], []
    for d in range(xyz.shape[0]):
        on = np.nonzero(xyz[d] == 0.0)[0]
        bn.append(on); bd.append(np.full(len(on), d))
    bn = np.concatenate(bn).astype(np.int32); bd = np.concatenate(bd).astype(np.int32)
    return bn, bd, np.zeros(len(bn))


def jiggle_interior(xyz, amount, seed):
    """Move the nodes strictly inside the bounding box off their lattice sites (the boundary planes stay planes)."""
    rng = np.random.default_rng(seed)
    inside = np.all((xyz > xyz.min(1)[:, None]) & (xyz < xyz.max(1)[:, None]), axis=0)
    out = xyz.copy()
    out[:, inside] += rng.uniform(-amount, amount, (xyz.shape[0], inside.sum()))
    return out


def tria_strip(nx, ny, lx, ly, seed=3):
    """(xyz (2, nNode), conn (3, nElem)): nx x ny cells on [0, lx] x [0, ly], two counter-clockwise triangles a cell with the
    diagonal alternating, interior nodes jiggled by a fifth of a cell."""
    xs, ys = np.meshgrid(np.linspace(0.0, lx, nx + 1), np.linspace(0.0, ly, ny + 1), indexing="ij")
    xyz = np.array([xs.ravel(), ys.ravel()])
    nid = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    tris = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = nid[i, j], nid[i + 1, j], nid[i + 1, j + 1], nid[i, j + 1]
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return jiggle_interior(xyz, 0.2 * min(lx / nx, ly / ny), seed), np.array(tris, np.int32).T.copy()


def load_vector(kind, xyz, conn, edof, N, elem, side, load, values, layout, thick=1.0):
    """``b (N,)``: what pfem_rhs_add_surface_load adds, in the free-dof numbering of ``edof`` (``drivers._setup``: xyz, conn in
    the NEW node numbering, edof (nsize, nElem) with -1 = constrained), and ``babs (N,)`` = the sum of |contribution| per dof.
    ``thick``: scalar or per ELEMENT (nElem,).  Constrained dofs get nothing; a side given twice adds twice."""
    elem = np.asarray(elem, np.int64); side = np.asarray(side, np.int64)
    npe, ndof = NPE[kind], NDOF[kind]
    ns = npe - 1
    n = len(elem)
    meas, nrm, _, _ = geometry(xyz, conn, elem, side)
    vals = expand_values(values, layout, n, ns, load_components(kind, load))
    th = np.asarray(thick, np.float64)
    th = th[elem] if th.ndim == 1 else th
    Fs, _ = consistent_loads(kind, load, meas, nrm, vals, th)
    loc = side_local_nodes(npe)[side]                                      # (n, ns) local nodes of every side
    b = np.zeros(N); babs = np.zeros(N)
    for a in range(ns):
        for c in range(ndof):
            r = edof[loc[:, a] * ndof + c, elem]
            ok = r >= 0
            np.add.at(b, r[ok], Fs[ok, a, c])
            np.add.at(babs, r[ok], np.abs(Fs[ok, a, c]))
    return b, babs
