"""numpy reference of the nodal recovery and the Zienkiewicz-Zhu indicator (pfem_post_nodal_recovery /
pfem_post_error_indicator): element weights from the coordinates, np.add.at sums, the closed form of the indicator."""
import functools

import numpy as np

GAUSS_WT_TET = float(np.float32(1.0) / np.float32(6.0))      # the element routines' REAL(4) Gauss weight


def element_weights(xyz, conn, thick=1.0):
    """dvol of the element routines (volume; area; area x thickness), in their own order of operations: the same bits."""
    X = xyz[:, conn]                                         # [dim, a, e]
    if conn.shape[0] == 4:
        (b11, b12, b13), (b21, b22, b23), (b31, b32, b33) = X[:, 0] - X[:, 2], X[:, 1] - X[:, 2], X[:, 3] - X[:, 2]
        jac = b11 * (b22 * b33 - b23 * b32)
        jac = jac + b12 * (b23 * b31 - b21 * b33)
        jac = jac + b13 * (b21 * b32 - b22 * b31)
        return GAUSS_WT_TET * jac
    jac = (X[0, 1] - X[0, 0]) * (X[1, 2] - X[1, 0]) - (X[1, 1] - X[1, 0]) * (X[0, 2] - X[0, 0])
    return 0.5 * (jac * thick)


def recover(conn, w, f, nNode):
    """f (ng, nElem) -> nodal (nNode, ng) = sum w f / sum w, weight (nNode,), B = sum w |f| / sum w, cnt (nNode,)."""
    ng = f.shape[0]
    num, mag, den, cnt = np.zeros((nNode, ng)), np.zeros((nNode, ng)), np.zeros(nNode), np.zeros(nNode, np.int64)
    for a in range(conn.shape[0]):
        np.add.at(num, conn[a], (w * f).T)
        np.add.at(mag, conn[a], (w * np.abs(f)).T)
        np.add.at(den, conn[a], w)
        np.add.at(cnt, conn[a], 1)
    safe = np.where(cnt > 0, den, 1.0)[:, None]
    return num / safe, den, mag / safe, cnt


def indicator(conn, w, f, nodal):
    """eta2 (nElem,), fnorm2 (nElem,): V / ((d+1)(d+2)) sum_c [sum_a d_ac^2 + (sum_a d_ac)^2] with d_ac = nodal - f, V sum_c f_c^2."""
    npe = conn.shape[0]                                      # d + 1
    d = nodal[conn.T] - f.T[:, None, :]                      # [e, a, c]
    return w / (npe * (npe + 1)) * ((d * d).sum(1) + d.sum(1) ** 2).sum(1), w * (f * f).sum(0)


@functools.lru_cache(maxsize=None)
def exact_box(n):
    """The reference on gen_box_tets(-1,1,n, ...) with u = x^2+y^2+z^2 and unit conductivity: fluxes from H.ElementPost, the
    indicator, and the 'true' error with the exact q = -2x at the nodes through the same closed form."""
    from pfemfort_amd import _lib as L
    from pfemfort_amd import host as H
    m = H.gen_box_tets(-1, 1, n, -1, 1, n, -1, 1, n)
    u = (m.xyz ** 2).sum(0)
    f = np.empty((3, m.nElem))
    for e in range(m.nElem):
        nd = m.conn[:, e]
        f[:, e] = H.ElementPost(L.POISSON_TET, m.xyz[0, nd], m.xyz[1, nd], m.xyz[2, nd], H.POISSON_ELEMDATA, u[nd])[1]
    w = element_weights(m.xyz, m.conn)
    nodal, weight, _, _ = recover(m.conn, w, f, m.nNode)
    eta2, fn2 = indicator(m.conn, w, f, nodal)
    true2, _ = indicator(m.conn, w, f, -2.0 * m.xyz.T)
    return {"mesh": m, "u": u, "flux": f, "nodal": nodal, "weight": weight, "eta2": eta2, "eta2_total": eta2.sum(),
            "fnorm2_total": fn2.sum(), "eta": np.sqrt(eta2.sum()), "true": np.sqrt(true2.sum())}
