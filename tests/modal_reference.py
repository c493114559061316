"""numpy mirror of the modal analysis (pfem_modal_solve): the lowest eigenpairs of K phi = omega^2 M phi,
M = diag(m), by LOBPCG without soft locking.  The mirror fixes the scheme and the device follows it step by step: the block
size, the hash that sets X0 (the same integers, so both sides start from the same bits), one Rayleigh-Ritz on X0, then per
iteration the residual block with its three column norms, W = T R, the Gram matrices of S = [X W P] from their upper triangles,
the scaled-Cholesky Rayleigh-Ritz (pfem_dense_sym_geneig; here numpy's eigh stands for its Jacobi sweeps), the update
P' = W C_W + P C_P, X' = X C_X + P' with the same coefficients on the K-blocks, and an explicit K X every 10th iteration."""
import contextlib

import numpy as np
import scipy.linalg as sl

try:                     # the blocks are tall and thin: BLAS threads cost several times what they save
    from threadpoolctl import threadpool_limits
except ImportError:      # pragma: no cover
    threadpool_limits = lambda limits: contextlib.nullcontext()      # noqa: E731

EPS = np.finfo(np.float64).eps
FLOOR = 1e-12            # smallest squared pivot of the scaled Gram matrix's Cholesky factor before P is dropped
REFRESH = 10             # every REFRESH-th iteration K X is formed explicitly
MAX_MODES = 12
_MASK = (1 << 64) - 1


def block_size(n_modes, block=0, n=None):
    """MB in {4, 8, 16}: the smallest that holds n_modes with room to spare (<= 2 -> 4, <= 6 -> 8, <= 12 -> 16), or ``block`` if
    that is one of the three and no smaller.  ValueError where the library answers PFEM_ERR_ARG."""
    if n_modes < 1 or n_modes > MAX_MODES:
        raise ValueError("n_modes must be 1..12")
    auto = 4 if n_modes <= 2 else 8 if n_modes <= 6 else 16
    if block not in (0, 4, 8, 16) or (block and block < auto):
        raise ValueError("block must be 0, 4, 8 or 16 and hold n_modes")
    mb = max(auto, block)
    if n is not None and mb > n:
        raise ValueError("the block is wider than the matrix")
    return mb


def splitmix64(x):
    """splitmix64 of Python integers or of an array of them, as exact 64-bit arithmetic."""
    x = np.asarray(x, dtype=object)
    z = (x + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def start_block(n, mb):
    """X0 (n, mb): entry (i, j) = (splitmix64(i mb + j) >> 11) 2^-52 - 1, in [-1, 1); i the GLOBAL free dof."""
    z = splitmix64(np.arange(n * mb, dtype=object))
    top = np.array([int(v) >> 11 for v in z.ravel()], dtype=np.float64)           # < 2^53: exact
    return (top * 2.0 ** -52 - 1.0).reshape(n, mb)


def upper_mirrored(G):
    """the upper triangle of G with its mirror image below: how both sides symmetrise a Gram matrix"""
    U = np.triu(G)
    return U + np.triu(G, 1).T


def rayleigh_ritz(GK, GM, keep, floor=FLOOR, eig=None):
    """The lowest ``keep`` pairs of GK c = theta GM c: scale both by diag(GM)^-1/2, Cholesky of the scaled GM, the standard
    problem L^-1 GK L^-T, C = D L^-T Z.  None when the factorisation fails or its smallest pivot^2 is below ``floor``."""
    d = np.diag(GM)
    if not (d > 0.0).all() or not np.isfinite(d).all():
        return None
    D = 1.0 / np.sqrt(d)
    A = D[:, None] * GK * D[None, :]
    B = D[:, None] * GM * D[None, :]
    try:
        L = np.linalg.cholesky(B)
    except np.linalg.LinAlgError:
        return None
    if not (np.diag(L) ** 2 >= floor).all():
        return None
    Y = _trtrs(L, A)
    St = _trtrs(L, Y.T)
    St = upper_mirrored(St)
    w, Z = (eig or np.linalg.eigh)(St)
    order = np.argsort(w, kind="stable")[:keep]
    C = D[:, None] * _trtrs(L, Z[:, order], trans=1)
    return w[order], C


def _trtrs(L, B, trans=0):
    """L^-1 B (trans = 1: L^-T B) by LAPACK's triangular solve, without scipy's per-call checks"""
    X, info = sl.lapack.dtrtrs(L, np.asfortranarray(B), lower=1, trans=trans)
    assert info == 0
    return X


class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def normalise(X, m):
    """phi^T M phi = 1 and the entry of largest magnitude positive (the lowest index on ties), column by column"""
    X = X / np.sqrt((m[:, None] * X * X).sum(0))[None, :]
    big = np.abs(X).argmax(0)                     # (argmax: the first of equal maxima)
    return X * np.where(X[big, np.arange(X.shape[1])] < 0.0, -1.0, 1.0)[None, :]


def residuals(KX, X, m, theta):
    MX = m[:, None] * X
    R = KX - MX * theta[None, :]
    res = np.sqrt((R * R).sum(0)) / (np.sqrt((KX * KX).sum(0)) + np.abs(theta) * np.sqrt((MX * MX).sum(0)))
    return R, res


def lobpcg(*args, **kw):
    with threadpool_limits(limits=1):
        return _lobpcg(*args, **kw)


def _lobpcg(A, m, n_modes, tol=1e-6, max_iterations=1000, block=0, x0=None, T=None, refresh=REFRESH, eig=None):
    """The lowest n_modes pairs of (A, diag(m)).  T: R -> W, the preconditioner on a block (None: point Jacobi, R / diag(A)).
    Returns omega2, modes (n, n_modes), residuals, iterations, restarts, reason (1 converged, -1 max_iterations, -2 breakdown)."""
    n = A.shape[0]
    mb = block_size(n_modes, block, n)
    if not (tol > 0.0) or not np.isfinite(tol) or max_iterations < 1:
        raise ValueError("tol > 0 and max_iterations >= 1")
    if not (m > 0.0).all():
        raise ValueError("every mass must be positive")
    if T is None:
        dinv = 1.0 / A.diagonal()
        T = lambda R: dinv[:, None] * R           # noqa: E731
    X = start_block(n, mb) if x0 is None else np.array(x0, dtype=np.float64).reshape(n, mb)
    KX = A @ X
    theta = np.zeros(mb)
    P = KP = None
    restarts, reason, its = 0, -1, 0
    rr = rayleigh_ritz(upper_mirrored(X.T @ KX), upper_mirrored(X.T @ (m[:, None] * X)), mb, eig=eig)
    if rr is None:
        reason = -2
    else:
        theta, C = rr
        X, KX = X @ C, KX @ C
        while True:
            R, res = residuals(KX, X, m, theta)
            if (res[:n_modes] <= tol).all():
                reason = 1
                break
            if its >= max_iterations:
                reason = -1
                break
            its += 1
            W = T(R)
            KW = A @ W
            S = [X, W] + ([P] if P is not None else [])
            KS = [KX, KW] + ([KP] if P is not None else [])
            S, KS = np.hstack(S), np.hstack(KS)
            GK = upper_mirrored(S.T @ KS)
            GM = upper_mirrored(S.T @ (m[:, None] * S))
            rr = rayleigh_ritz(GK, GM, mb, eig=eig)
            if rr is None and P is not None:          # drop P: a restart
                restarts += 1
                S, KS = S[:, :2 * mb], KS[:, :2 * mb]
                rr = rayleigh_ritz(GK[:2 * mb, :2 * mb], GM[:2 * mb, :2 * mb], mb, eig=eig)
            if rr is None:
                reason = -2
                break
            theta, C = rr
            P = S[:, mb:] @ C[mb:]
            KP = KS[:, mb:] @ C[mb:]
            X = X @ C[:mb] + P
            KX = KX @ C[:mb] + KP
            if its % refresh == 0:
                KX = A @ X
    order = np.argsort(theta, kind="stable")
    theta, X = theta[order], X[:, order]
    _, res = residuals(A @ X, X, m, theta)
    return Result(omega2=theta[:n_modes], modes=normalise(X[:, :n_modes], m), residuals=res[:n_modes], iterations=its,
                  restarts=restarts, reason=reason, block=mb)


# ---- what the tests measure, on both sides ---------------------------------------------------------------------------------------
def lowest_modes(A, m, k):
    """The lowest k pairs of (A, diag(m)) by shift-invert Lanczos about 0 (scipy's eigsh on a sparse LU of A, to its full
    accuracy, from a fixed start vector): eigenvalues ascending and M-orthonormal vectors.  The reference where the dense eigh
    of dynamics_reference.modes is out of reach."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    lam, V = spl.eigsh(sp.csc_matrix(A), k=k, M=sp.diags(m).tocsc(), sigma=0, which="LM", v0=np.ones(A.shape[0]))
    order = np.argsort(lam)
    lam, V = lam[order], V[:, order]
    return lam, V / np.sqrt((m[:, None] * V * V).sum(0))[None, :]


def eig_error(omega2, lam):
    """largest relative error of the eigenvalues against the dense ones"""
    k = len(omega2)
    return float((np.abs(omega2 - lam[:k]) / np.abs(lam[:k])).max())


def subspace_distance(Phi, V, m):
    """M-distance of span(Phi) from span(V), both M-orthonormal: the largest M-norm of a column of Phi - V (V^T M Phi)"""
    E = Phi - V @ (V.T @ (m[:, None] * Phi))
    return float(np.sqrt((m[:, None] * E * E).sum(0)).max())


def orthonormality(Phi, m):
    return float(np.abs(Phi.T @ (m[:, None] * Phi) - np.eye(Phi.shape[1])).max())


def jacobi_eigh(S, sweeps=60):
    """cyclic Jacobi on a symmetric matrix, row by row: the plain restatement of what pfem_dense_sym_geneig runs (small n only)"""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    V = np.eye(n)
    for _ in range(sweeps):
        off = np.sqrt((np.triu(A, 1) ** 2).sum())
        if off <= EPS * np.sqrt((np.diag(A) ** 2).sum()) or off == 0.0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0.0:
                    continue
                tau = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                J = np.array([[c, s], [-s, c]])
                A[[p, q], :] = J.T @ A[[p, q], :]
                A[:, [p, q]] = A[:, [p, q]] @ J
                V[:, [p, q]] = V[:, [p, q]] @ J
    w = np.diag(A).copy()
    order = np.argsort(w, kind="stable")
    return w[order], V[:, order]
