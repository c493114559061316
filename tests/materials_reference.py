"""numpy reference of an assembly with one material per element (pfem_mesh_set_materials): the element matrices from the
unchanged oracle, called once per material on that material's elements, and a plain mirror of the oracle's serial assembly
loop (orc_assemble) that adds them in ascending element order -- the order the device's gather form promises bit for bit."""
from dataclasses import dataclass

import numpy as np

from oracle import pfem_oracle as O

EPS = np.finfo(np.float64).eps


def eval_elems(kind, xyz, conn, table, elem_mat):
    """K (nElem, nsize, nsize) with K[e][i, j] = Klocal(i, j) and F (nElem, nsize): the oracle's eval_elems per material."""
    table = np.atleast_2d(np.asarray(table, dtype=np.float64))
    elem_mat = np.asarray(elem_mat)
    ns = O.NPELEM[kind] * O.NDOF[kind]
    nElem = conn.shape[1]
    K = np.empty((nElem, ns, ns)); F = np.empty((nElem, ns))
    for m in np.unique(elem_mat):
        sel = np.nonzero(elem_mat == m)[0]
        K[sel], F[sel] = O.eval_elems(kind, xyz, np.ascontiguousarray(conn[:, sel]), table[m])
    return K, F


def assemble(K, F, conn, edof, solnApplied, ndof, rowptr, cols):
    """orc_assemble with the element matrices given: per element, ascending --
      vals[(idx[ii], idx[jj])] += Klocal(jj, ii)            (MatSetValues: row-major read of the column-major block)
      F[jj] = F[jj] - Klocal(jj, ii) * fact                  (lifting, over the constrained ii ascending)
      rhs[idx[ii]] += F[ii]
    np.add.at applies its updates one after the other in index order, so the flattened element-major index arrays below give
    every slot its contributions in the order of the serial loop."""
    nElem, ns = F.shape
    N = len(rowptr) - 1
    idx = np.ascontiguousarray(edof.T).astype(np.int64)                       # [e, ii]
    rows_of = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    keys = rows_of * N + cols                                                # ascending: rows ascending, columns ascending in a row
    r = np.broadcast_to(idx[:, :, None], (nElem, ns, ns))                    # [e, ii, jj] -> idx[ii]
    c = np.broadcast_to(idx[:, None, :], (nElem, ns, ns))                    # [e, ii, jj] -> idx[jj]
    free = (r >= 0) & (c >= 0)
    q = (r * N + c)[free]
    pos = np.searchsorted(keys, q)
    assert np.array_equal(keys[pos], q), "an element entry outside the pattern"
    vals = np.zeros(len(cols))
    np.add.at(vals, pos, K.transpose(0, 2, 1)[free])                          # [e, ii, jj] -> Klocal(jj, ii)
    F = F.copy()
    sa = np.asarray(solnApplied, dtype=np.float64)
    for ii in range(ns):
        fixed = idx[:, ii] == -1
        if not fixed.any():
            continue
        fact = sa[conn[ii // ndof].astype(np.int64) * ndof + ii % ndof]
        for jj in range(ns):
            m = fixed & (idx[:, jj] != -1)
            F[m, jj] = F[m, jj] - K[m, jj, ii] * fact[m]
    rhs = np.zeros(N)
    fr = idx >= 0
    np.add.at(rhs, idx[fr], F[fr])
    return vals, rhs


@dataclass
class Problem:
    kind: int
    dm: object
    xyz_new: np.ndarray
    conn_new: np.ndarray
    edof: np.ndarray
    rowptr: np.ndarray
    cols: np.ndarray
    vals: np.ndarray
    rhs: np.ndarray
    K: np.ndarray
    F: np.ndarray


def setup_problem(kind, mesh, table, elem_mat):
    """O.setup_problem with a table of elemData rows and one row number per element (the mesh's element order)."""
    ndof = O.NDOF[kind]
    dm = O.dof_numbering(mesh.xyz.shape[1], ndof, mesh.bc_node, mesh.bc_dof, mesh.bc_val)
    conn_new = dm.node_map_get_new[mesh.conn].astype(np.int32)
    xyz_new = np.ascontiguousarray(mesh.xyz[:, dm.node_map_get_old])
    edof = O.elem_dof_array(conn_new, dm.NodeDofArrayNew)
    rowptr, cols = O.csr_pattern(edof, dm.size_global)
    K, F = eval_elems(kind, xyz_new, conn_new, table, elem_mat)
    vals, rhs = assemble(K, F, conn_new, edof, dm.solnApplied, ndof, rowptr, cols)
    return Problem(kind, dm, xyz_new, conn_new, edof, rowptr, cols, vals, rhs, K, F)


def direct_solve(p):
    """The mirror system through scipy's sparse LU."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    N = len(p.rowptr) - 1
    A = sp.csr_matrix((p.vals, p.cols, p.rowptr), shape=(N, N)).tocsc()
    return spl.splu(A).solve(p.rhs)


def full_field(p, u_free):
    """(nNode, ndof) by NEW node id: the solution at the free dofs, solnApplied at the constrained ones."""
    nda = p.dm.NodeDofArrayNew
    full = p.dm.solnApplied.reshape(nda.shape).copy()
    full[nda >= 0] = u_free[nda[nda >= 0]]
    return full


# ---- the two-E bar: elastic tet box [0,2] x [0,1]^2, E = 100 for centroids x < 1 and 400 beyond, nu = 0, no body force, all
# dofs fixed at x = 0, u_x = delta at x = 2.  Exact in the P1 space: sigma_xx = delta / (1/100 + 1/400), u_x piecewise linear.
BAR_E = (100.0, 400.0)


def bar(H, delta=1.0):
    """(mesh, table, elem_mat, sigma, u_x(x)) of the two-material bar on 4 x 2 x 2 cells; ``H`` = pfemfort_amd.host."""
    m = H.gen_box_tets(0.0, 2.0, 4, 0.0, 1.0, 2, 0.0, 1.0, 2, bc_mode=1, ndof=3)
    x = m.xyz[0]
    left = np.nonzero(x == 0.0)[0].astype(np.int32)
    right = np.nonzero(x == 2.0)[0].astype(np.int32)
    assert len(left) == 9 and len(right) == 9
    bn = np.concatenate([np.repeat(left, 3), right])
    bd = np.concatenate([np.tile(np.arange(3, dtype=np.int32), len(left)), np.zeros(len(right), np.int32)])
    bv = np.concatenate([np.zeros(3 * len(left)), np.full(len(right), delta)])
    mesh = H.Mesh(m.xyz, m.conn, bn.astype(np.int32), bd.astype(np.int32), bv)
    table = np.array([[BAR_E[0], 0.0, 1.0, 0.0, 0.0, 0.0], [BAR_E[1], 0.0, 1.0, 0.0, 0.0, 0.0]])
    elem_mat = (m.xyz[0][m.conn].mean(0) > 1.0).astype(np.int32)
    sigma = delta / (1.0 / BAR_E[0] + 1.0 / BAR_E[1])

    def ux(xx):
        return np.where(xx <= 1.0, sigma * xx / BAR_E[0], sigma / BAR_E[0] + sigma * (xx - 1.0) / BAR_E[1])
    return mesh, table, elem_mat, sigma, ux
