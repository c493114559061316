"""numpy mirror of the linear buckling analysis (pfem_elem_geometric, pfem_buckling_setup, pfem_buckling_solve; DESIGN.md section
15): the geometric stiffness of the elasticity kinds in the written-down order of csrc/pfem_elem.hpp (elem_geometric), vectorised
over the elements; its assembly on K's pattern in ascending element order; and LOBPCG on the pencil K_g phi = theta K phi -- the
scheme of tests/modal_reference.py with K S where that one has m o S, A = K_g, the same block size, hashed start block and
Rayleigh-Ritz step (reused from there).  The critical load factors of (K + lambda K_g) phi = 0 are lambda = -1 / theta for
theta < 0; a pair with theta >= 0 does not buckle in the load's direction: lambda = inf.

Element kinds: 3 = elastic tet, 5 = plane-stress triangle (include/pfem_amd.h).  Geometry and dvol are thermal_reference's (the
shape-function gradients without the literal products by 0 and 1: every nonzero entry has the element routines' bits)."""
import numpy as np

import modal_reference as MO
import thermal_reference as TR
from modal_reference import threadpool_limits

EPS = np.finfo(np.float64).eps
ELAST_TET, ELAST_TRIA = 3, 5
REFRESH = MO.REFRESH


def element_g(kind, xyz, conn, rows, sig):
    """g (nElem, npe, npe), g[e, a, b] = dvol (grad N_a . sig grad N_b) in elem_geometric's order; sig (ng, nElem) in the order of
    the flux of the post-processing, rows (nElem, >= 3) the elements' elemData (the triangle's thickness)."""
    gr, jac = TR.geometry(kind, xyz, conn)
    assert np.all(jac > 0)
    dv = TR.dvol(kind, xyz, conn, rows)
    npe = conn.shape[0]
    g = np.empty((conn.shape[1], npe, npe))
    if kind == ELAST_TET:
        gx, gy, gz = gr
        sxx, syy, szz, sxy, syz, szx = sig
        for b in range(4):
            tx = (sxx * gx[b] + sxy * gy[b]) + szx * gz[b]
            ty = (sxy * gx[b] + syy * gy[b]) + syz * gz[b]
            tz = (szx * gx[b] + syz * gy[b]) + szz * gz[b]
            for a in range(4):
                g[:, a, b] = dv * ((gx[a] * tx + gy[a] * ty) + gz[a] * tz)
        return g
    gx, gy = gr
    sxx, syy, sxy = sig
    for b in range(3):
        tx = sxx * gx[b] + sxy * gy[b]
        ty = sxy * gx[b] + syy * gy[b]
        for a in range(3):
            g[:, a, b] = dv * (gx[a] * tx + gy[a] * ty)
    return g


def assemble(g, edof, ndof, rowptr, cols):
    """K_g's values on the pattern (rowptr, cols): entry (row = dof(b, i), col = dof(a, i)) += g[e, a, b] for every component i
    whose two dofs are free, the elements in ascending order (np.add.at applies its updates one after the other; an element
    meets an entry once).  Returns (vals, sabs, count): the sums, the sums of |g| and the number of contributions per entry --
    what bounds a sum of `count` terms taken in any order: (count - 1) eps sabs."""
    nElem, npe, _ = g.shape
    N = len(rowptr) - 1
    idx = np.ascontiguousarray(edof.T).astype(np.int64).reshape(nElem, npe, ndof)      # [e, a, d]
    shape = (nElem, npe, npe, ndof)                                                      # [e, a, b, d]
    r = np.broadcast_to(idx[:, None, :, :], shape)
    c = np.broadcast_to(idx[:, :, None, :], shape)
    v = np.broadcast_to(g[:, :, :, None], shape)
    free = (r >= 0) & (c >= 0)
    rows_of = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    keys = rows_of * N + cols
    q = (r * N + c)[free]
    pos = np.searchsorted(keys, q)
    assert np.array_equal(keys[pos], q), "an element entry outside the pattern"
    vals, sabs, count = np.zeros(len(cols)), np.zeros(len(cols)), np.zeros(len(cols), np.int64)
    np.add.at(vals, pos, v[free])
    np.add.at(sabs, pos, np.abs(v[free]))
    np.add.at(count, pos, 1)
    return vals, sabs, count


def factors(theta):
    """lambda = -1 / theta for theta < 0, else inf"""
    theta = np.asarray(theta, dtype=np.float64)
    out = np.full(theta.shape, np.inf)
    neg = theta < 0.0
    out[neg] = -1.0 / theta[neg]
    return out


def normalise(X, KX):
    """phi^T K phi = 1 and the entry of largest magnitude positive (the lowest index on ties), column by column"""
    X = X / np.sqrt((X * KX).sum(0))[None, :]
    big = np.abs(X).argmax(0)
    return X * np.where(X[big, np.arange(X.shape[1])] < 0.0, -1.0, 1.0)[None, :]


def residuals(GX, KX, theta):
    R = GX - KX * theta[None, :]
    den = np.sqrt((GX * GX).sum(0)) + np.abs(theta) * np.sqrt((KX * KX).sum(0))
    return R, np.sqrt((R * R).sum(0)) / den


def lobpcg(*args, **kw):
    with threadpool_limits(limits=1):
        return _lobpcg(*args, **kw)


def _lobpcg(Kg, K, n_modes, tol=1e-6, max_iterations=1000, block=0, x0=None, T=None, refresh=REFRESH, eig=None):
    """The lowest n_modes pairs of (Kg, K), K SPD.  T: R -> W on a block (None: the point Jacobi of K).  Returns theta, factors,
    modes (n, n_modes), residuals, iterations, restarts, reason (1 converged, -1 max_iterations, -2 breakdown), block."""
    n = K.shape[0]
    mb = MO.block_size(n_modes, block, n)
    if not (tol > 0.0) or not np.isfinite(tol) or max_iterations < 1:
        raise ValueError("tol > 0 and max_iterations >= 1")
    if T is None:
        dinv = 1.0 / K.diagonal()
        T = lambda R: dinv[:, None] * R           # noqa: E731
    X = MO.start_block(n, mb) if x0 is None else np.array(x0, dtype=np.float64).reshape(n, mb)
    KX, GX = K @ X, Kg @ X
    theta = np.zeros(mb)
    P = KP = GP = None
    restarts, reason, its = 0, -1, 0
    rr = MO.rayleigh_ritz(MO.upper_mirrored(X.T @ GX), MO.upper_mirrored(X.T @ KX), mb, eig=eig)
    if rr is None:
        reason = -2
    else:
        theta, C = rr
        X, KX, GX = X @ C, KX @ C, GX @ C
        while True:
            R, res = residuals(GX, KX, theta)
            if (res[:n_modes] <= tol).all():
                reason = 1
                break
            if its >= max_iterations:
                reason = -1
                break
            its += 1
            W = T(R)
            KW, GW = K @ W, Kg @ W
            have_p = P is not None
            S = np.hstack([X, W] + ([P] if have_p else []))
            KS = np.hstack([KX, KW] + ([KP] if have_p else []))
            GS = np.hstack([GX, GW] + ([GP] if have_p else []))
            GA = MO.upper_mirrored(S.T @ GS)
            GB = MO.upper_mirrored(S.T @ KS)
            rr = MO.rayleigh_ritz(GA, GB, mb, eig=eig)
            if rr is None and have_p:                 # drop P: a restart
                restarts += 1
                S, KS, GS = S[:, :2 * mb], KS[:, :2 * mb], GS[:, :2 * mb]
                rr = MO.rayleigh_ritz(GA[:2 * mb, :2 * mb], GB[:2 * mb, :2 * mb], mb, eig=eig)
            if rr is None:
                reason = -2
                break
            theta, C = rr
            P, KP, GP = S[:, mb:] @ C[mb:], KS[:, mb:] @ C[mb:], GS[:, mb:] @ C[mb:]
            X, KX, GX = X @ C[:mb] + P, KX @ C[:mb] + KP, GX @ C[:mb] + GP
            if its % refresh == 0:
                KX, GX = K @ X, Kg @ X
    order = np.argsort(theta, kind="stable")
    theta, X = theta[order], X[:, order]
    KX = K @ X
    _, res = residuals(Kg @ X, KX, theta)
    return MO.Result(theta=theta[:n_modes], factors=factors(theta[:n_modes]), modes=normalise(X[:, :n_modes], KX[:, :n_modes]),
                     residuals=res[:n_modes], iterations=its, restarts=restarts, reason=reason, block=mb)


def dense_pairs(Kg, K):
    """all pairs of Kg phi = theta K phi by scipy's dense eigh, theta ascending, phi^T K phi = 1"""
    import scipy.linalg as sl
    return sl.eigh(Kg.toarray(), K.toarray())


def theta_error(theta, dense):
    """largest |theta - theta_dense| relative to |theta_1|, the lowest dense eigenvalue"""
    k = len(theta)
    return float(np.abs(theta - dense[:k]).max() / abs(dense[0]))
