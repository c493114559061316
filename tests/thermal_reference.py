"""numpy mirror of the thermal strains of the elasticity kinds (pfem_elem_thermal_load, pfem_rhs_add_thermal_load and the
post-processing under a thermal state): the written-down sequences of IEEE operations of csrc/pfem_elem.hpp (thermal_strain,
elem_thermal_load, elast_*_post_t<true>), vectorised over the elements, and np.add.at sums in ascending element order -- the
order the device's gather form promises.  Element weights are post_reference.element_weights', the assembled system
materials_reference's.

Geometry: the shape-function gradients are written without the element routines' literal products by 0 and 1; every nonzero
entry has the same bits (pfem_elem.hpp: tet_geometry_lean), a zero entry may differ in its sign, which no comparison sees.
Element kinds: 3 = elastic tet, 5 = plane-stress triangle (include/pfem_amd.h)."""
import numpy as np

import post_reference as PR

EPS = np.finfo(np.float64).eps
ELAST_TET, ELAST_TRIA = 3, 5
GAUSS_PT_TRIA = float(np.float32(1.0) / np.float32(3.0))      # the triangle's REAL(4) Gauss point


def shape_values(kind):
    """N at the one Gauss point, in the element routines' own arithmetic."""
    if kind == ELAST_TET:
        return [0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25]
    return [1.0 - GAUSS_PT_TRIA - GAUSS_PT_TRIA, GAUSS_PT_TRIA, GAUSS_PT_TRIA]


def geometry(kind, xyz, conn):
    """g[d][a] (arrays over the elements) = dN_a / dx_d and the Jacobian, in the order of tet_geometry / tria_geometry."""
    X = xyz[:, conn]                                          # [dim, a, e]
    if kind == ELAST_TET:
        x, y, z = X
        b11, b21, b31 = x[0] - x[2], x[1] - x[2], x[3] - x[2]
        b12, b22, b32 = y[0] - y[2], y[1] - y[2], y[3] - y[2]
        b13, b23, b33 = z[0] - z[2], z[1] - z[2], z[3] - z[2]
        jac = b11 * (b22 * b33 - b23 * b32)
        jac = jac + b12 * (b23 * b31 - b21 * b33)
        jac = jac + b13 * (b21 * b32 - b22 * b31)
        di = 1.0 / jac
        i11 = +di * (b22 * b33 - b23 * b32); i21 = -di * (b21 * b33 - b23 * b31); i31 = +di * (b21 * b32 - b22 * b31)
        i12 = -di * (b12 * b33 - b13 * b32); i22 = +di * (b11 * b33 - b13 * b31); i32 = -di * (b11 * b32 - b12 * b31)
        i13 = +di * (b12 * b23 - b13 * b22); i23 = -di * (b11 * b23 - b13 * b21); i33 = +di * (b11 * b22 - b12 * b21)
        g = [[i11, i12, (-i11 - i12) - i13, i13], [i21, i22, (-i21 - i22) - i23, i23], [i31, i32, (-i31 - i32) - i33, i33]]
        return g, jac
    x, y = X[0], X[1]
    b11, b21, b12, b22 = x[1] - x[0], x[2] - x[0], y[1] - y[0], y[2] - y[0]
    jac = b11 * b22 - b12 * b21
    di = 1.0 / jac
    i11, i12, i21, i22 = b22 * di, -b12 * di, -b21 * di, b11 * di
    return [[-i11 - i12, i11, i12], [-i21 - i22, i21, i22]], jac


def material(kind, rows):
    """(d11, d12, shear) per element from its elemData row: elast_material / elast2d_material."""
    E, nu = rows[:, 0], rows[:, 1]
    if kind == ELAST_TET:
        b1 = E / ((1.0 + nu) * (1.0 - 2.0 * nu))
        b2 = (1.0 - 2.0 * nu) / 2.0
        return b1 * (1.0 - nu), b1 * nu, b1 * b2
    b1 = E / (1.0 - nu * nu)
    return b1, b1 * nu, b1 * (1.0 - nu)


def dvol(kind, xyz, conn, rows):
    return PR.element_weights(xyz, conn, rows[:, 2] if kind == ELAST_TRIA else 1.0)


def rows_of(ed, nElem, elem_mat=None):
    """Every element's own elemData row: one vector for all, or table[elem_mat]."""
    ed = np.asarray(ed, dtype=np.float64)
    return np.broadcast_to(ed, (nElem, ed.size)).copy() if elem_mat is None else ed[np.asarray(elem_mat)]


def alpha_of(alpha, nElem, elem_mat=None):
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    return np.full(nElem, a[0]) if elem_mat is None else a[np.asarray(elem_mat)]


def thermal_strain(kind, alpha_e, theta, conn):
    """e_th = alpha * (sum over a ascending of N_a theta_a, from 0.0) per element."""
    N = shape_values(kind)
    tb = np.zeros(conn.shape[1])
    for a in range(conn.shape[0]):
        tb = tb + N[a] * theta[conn[a]]
    return alpha_e * tb


def element_loads(kind, xyz, conn, rows, eth):
    """F (nElem, nsize) = dvol (g_d[a] s) and sig (ng, nElem) = D eps_th row by row, as elem_thermal_load."""
    g, jac = geometry(kind, xyz, conn)
    assert np.all(jac > 0)
    dv = dvol(kind, xyz, conn, rows)
    d11, d12, _ = material(kind, rows)
    npe, nd = conn.shape[0], len(g)
    if kind == ELAST_TET:
        s = (d11 * eth + d12 * eth) + d12 * eth
        sig = np.stack([s, (d12 * eth + d11 * eth) + d12 * eth, (d12 * eth + d12 * eth) + d11 * eth] + [np.zeros_like(s)] * 3)
    else:
        s = d11 * eth + d12 * eth
        sig = np.stack([s, d12 * eth + d11 * eth, np.zeros_like(s)])
    F = np.empty((conn.shape[1], npe * nd))
    for a in range(npe):
        for d in range(nd):
            F[:, nd * a + d] = dv * (g[d][a] * s)
    return F, sig


def element_post(kind, xyz, conn, rows, eth, u):
    """(grad, flux, scalar, fint) of every element under the thermal strain eth (eth = 0.0: the plain routine's bits):
    elast_tet_post_t / elast_tria_post_t.  u (nNode, ndof)."""
    g, jac = geometry(kind, xyz, conn)
    assert np.all(jac > 0)
    dv = dvol(kind, xyz, conn, rows)
    d11, d12, dsh = material(kind, rows)
    nE, npe = conn.shape[1], conn.shape[0]
    z = np.zeros(nE)
    if kind == ELAST_TET:
        gx, gy, gz = g
        exx, eyy, ezz, gxy, gyz, gzx = z, z, z, z, z, z
        for a in range(4):
            uu, vv, ww = u[conn[a], 0], u[conn[a], 1], u[conn[a], 2]
            exx = exx + gx[a] * uu
            eyy = eyy + gy[a] * vv
            ezz = ezz + gz[a] * ww
            gxy = (gxy + gy[a] * uu) + gx[a] * vv
            gyz = (gyz + gz[a] * vv) + gy[a] * ww
            gzx = (gzx + gz[a] * uu) + gx[a] * ww
        mxx, myy, mzz = exx - eth, eyy - eth, ezz - eth
        sxx = (d11 * mxx + d12 * myy) + d12 * mzz
        syy = (d12 * mxx + d11 * myy) + d12 * mzz
        szz = (d12 * mxx + d12 * myy) + d11 * mzz
        txy, tyz, tzx = dsh * gxy, dsh * gyz, dsh * gzx
        d0, d1, d2 = sxx - syy, syy - szz, szz - sxx
        sc = np.sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((txy * txy + tyz * tyz) + tzx * tzx))
        fint = np.empty((nE, 12))
        for a in range(4):
            fint[:, 3 * a + 0] = dv * ((gx[a] * sxx + gy[a] * txy) + gz[a] * tzx)
            fint[:, 3 * a + 1] = dv * ((gy[a] * syy + gx[a] * txy) + gz[a] * tyz)
            fint[:, 3 * a + 2] = dv * ((gz[a] * szz + gy[a] * tyz) + gx[a] * tzx)
        return np.stack([exx, eyy, ezz, gxy, gyz, gzx]), np.stack([sxx, syy, szz, txy, tyz, tzx]), sc, fint
    gx, gy = g
    exx, eyy, gxy = z, z, z
    for a in range(3):
        uu, vv = u[conn[a], 0], u[conn[a], 1]
        exx = exx + gx[a] * uu
        eyy = eyy + gy[a] * vv
        gxy = (gxy + gy[a] * uu) + gx[a] * vv
    mxx, myy = exx - eth, eyy - eth
    sxx, syy, txy = d11 * mxx + d12 * myy, d12 * mxx + d11 * myy, dsh * gxy
    sc = np.sqrt(((sxx * sxx - sxx * syy) + syy * syy) + 3.0 * (txy * txy))
    fint = np.empty((nE, 6))
    for a in range(3):
        fint[:, 2 * a] = dv * (gx[a] * sxx + gy[a] * txy)
        fint[:, 2 * a + 1] = dv * (gy[a] * syy + gx[a] * txy)
    return np.stack([exx, eyy, gxy]), np.stack([sxx, syy, txy]), sc, fint


def body_loads(kind, xyz, conn, rows):
    """F_e (nElem, nsize) of the stiffness routines: dvol N_a bforce_d (0.0 + b4 * bforce)."""
    dv = dvol(kind, xyz, conn, rows)
    N = shape_values(kind)
    npe = conn.shape[0]
    nd = 3 if kind == ELAST_TET else 2
    F = np.empty((conn.shape[1], npe * nd))
    for a in range(npe):
        for d in range(nd):
            F[:, nd * a + d] = 0.0 + (dv * N[a]) * rows[:, 3 + d]
    return F


def load_vector(conn, edof, N, F):
    """b (N,) = sum_e F_e at the free dofs and babs = sum_e |F_e|, every row in ascending element order (np.add.at applies its
    updates one after the other; a node meets an element once)."""
    idx = np.ascontiguousarray(edof.T).astype(np.int64)          # [e, i]
    fr = idx >= 0
    b, babs = np.zeros(N), np.zeros(N)
    np.add.at(b, idx[fr], F[fr])
    np.add.at(babs, idx[fr], np.abs(F[fr]))
    return b, babs


def node_sums(conn, ndof, nNode, Fe):
    """(nNode, ndof) = sum over the elements of the per-element vectors Fe (nElem, npe * ndof), ascending element order."""
    idx = (conn.T[:, :, None].astype(np.int64) * ndof + np.arange(ndof)).reshape(conn.shape[1], -1)
    out = np.zeros(nNode * ndof)
    np.add.at(out, idx, Fe)
    return out.reshape(nNode, ndof)
