"""References for the pieces of -pc_type gamg, checked on the CPU by test_amg_reference.py and used by test_gpu_amg_pieces.py.

* ``galerkin_reference``: a coarse operator P^T A P formed the way the oracle's ``amg_cycle`` forms it, with the two matrices a
  derived entrywise tolerance needs (|P^T| |A| |P| and the number of summed terms).
* ``cycle_ld``: ``oracle.amg_cycle`` restated with the level matrices GIVEN (data, the same for every evaluation) and every
  vector and product in ``np.longdouble`` (x86-64: 64-bit mantissa).  With ``dtype=np.float64`` the same statements run in
  double precision: the evaluation the sensitivity test mutates.
* ``e64``: how far a correct fp64 evaluation of a cycle (``oracle.amg_cycle``) is from the extended one: the rounding level
  a tolerance on one application z = M^-1 r is a multiple of.

A plain module (no fixtures, no pytest settings): imported like test_gpu_amg_tail.py imports from test_gpu_parity.py.
"""
import numpy as np
import scipy.sparse as sp

from oracle import pfem_oracle as O

EPS = float(np.finfo(np.float64).eps)
KNOBS = dict(cheb_degree=2, fine_degree=1, eig_ratio=8.0, coarse_scale=1.5, dense_limit=128, coarsest_sweeps=8, gamma=1, gamma_from=1,
             gamma_to=99)


def prolongator(transfer, n_fine=None):
    """P of one transfer as scipy CSR: an explicit prolongator as it is, aggregates as the piecewise-constant one."""
    if sp.issparse(transfer):
        return transfer.tocsr()
    agg = np.asarray(transfer, dtype=np.int64)
    assert n_fine is None or len(agg) == n_fine
    return sp.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)), shape=(len(agg), int(agg.max()) + 1))


def _pattern(M):
    M = M.tocsr()
    return sp.csr_matrix((np.ones(len(M.data)), M.indices, M.indptr), shape=M.shape)


def galerkin_reference(A, transfer):
    """(Ac, Aabs, K) for one transfer (aggregates or an explicit prolongator):
    Ac = P^T A P in fp64 by the statements of ``oracle.amg_cycle`` (same bits), with the unit diagonal on the idle rotation dofs
    of a rigid-body level; Aabs = |P^T| |A| |P|; K = the same product over the 0/1 patterns of the stored entries: how many
    terms every coarse entry sums.  scipy's product drops sums that are exactly zero, so Ac may lack entries K counts."""
    A = A.tocsr()
    P = prolongator(transfer, A.shape[0])
    Ac = (P.T @ A @ P).tocsr()
    if sp.issparse(transfer):
        dg = Ac.diagonal()
        if (dg == 0.0).any():
            Ac = (Ac + sp.diags((dg == 0.0).astype(np.float64))).tocsr()
    Aabs = (abs(P).T @ abs(A) @ abs(P)).tocsr()
    K = (_pattern(P).T @ _pattern(A) @ _pattern(P)).tocsr()
    return Ac, Aabs, K


def gershgorin(A, rbm=False):
    """The bound ``amg_cycle`` takes for a level: max_i sum_j |a_ij| / a_ii, and -- hierarchies with rigid-body modes -- the smaller
    of it and the same bound on D^-1/2 A D^-1/2."""
    A = A.tocsr()
    d = A.diagonal()
    lam = float((abs(A) @ np.ones(A.shape[0]) / d).max())
    if rbm:
        sq = 1.0 / np.sqrt(d)
        lam = min(lam, float(((abs(A) @ sq) * sq).max()))
    return lam


class _Mat:
    """A CSR matrix as data of a given precision; y = A x by one multiply and one segmented sum."""

    def __init__(self, M, dtype):
        M = M.tocsr()
        M.sort_indices()
        self.shape = M.shape
        self.rowptr = M.indptr.astype(np.int64)
        self.cols = M.indices.astype(np.int64)
        self.vals = M.data.astype(dtype)
        self.dtype = dtype
        self.empty = np.diff(self.rowptr) == 0          # (reduceat hands back the next row's first term for an empty row)

    def dot(self, x):
        if len(self.vals) == 0:
            return np.zeros(self.shape[0], self.dtype)
        start = np.minimum(self.rowptr[:-1], len(self.vals) - 1)
        y = np.add.reduceat(self.vals * x[self.cols], start)
        if self.empty.any():
            y[self.empty] = 0
        return y

    def diagonal(self):
        rows = np.repeat(np.arange(self.shape[0]), np.diff(self.rowptr))
        d = np.zeros(self.shape[0], self.dtype)
        on = rows == self.cols
        d[rows[on]] = self.vals[on]
        return d


def _lu(Ad):
    """Gauss elimination with partial pivoting, in place, in the precision of ``Ad`` (at most 128 rows); returns (LU, perm)."""
    n = Ad.shape[0]
    assert n <= 128
    perm = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(Ad[k:, k])))
        assert Ad[p, k] != 0
        if p != k:
            Ad[[k, p]] = Ad[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        if k + 1 < n:
            Ad[k + 1:, k] = Ad[k + 1:, k] / Ad[k, k]
            Ad[k + 1:, k + 1:] = Ad[k + 1:, k + 1:] - np.outer(Ad[k + 1:, k], Ad[k, k + 1:])
    return Ad, perm


def _lu_solve(LU, perm, b):
    n = LU.shape[0]
    y = b[perm].copy()
    for k in range(1, n):
        y[k] = y[k] - np.sum(LU[k, :k] * y[:k])
    for k in range(n - 1, -1, -1):
        y[k] = (y[k] - np.sum(LU[k, k + 1:] * y[k + 1:])) / LU[k, k]
    return y


def cycle_ld(A0, levels, transfers, lam, knobs=None, dtype=np.longdouble, restrictions=None):
    """r -> z = M^-1 r: ``oracle.amg_cycle`` with the coarse matrices ``levels`` (level 1, 2, ...) and the bounds ``lam`` (level 0,
    1, ...) given, every vector, product and scalar in ``dtype``.  ``transfers`` as ``amg_cycle`` takes them; ``knobs`` overrides
    KNOBS; ``restrictions[l]`` replaces P_l^T (the sensitivity test's mutation)."""
    if dtype is np.longdouble:
        assert np.finfo(np.longdouble).eps < 2e-19, \
            "np.longdouble is not the x87 80-bit format here (eps %g): cycle_ld would be no more exact than fp64" % np.finfo(np.longdouble).eps
    k = dict(KNOBS, **(knobs or {}))
    mats = [A0.tocsr()] + [M.tocsr() for M in levels]
    nl = len(mats)
    assert len(transfers) == nl - 1 and len(lam) == nl
    Ps = [prolongator(t, mats[l].shape[0]) for l, t in enumerate(transfers)]
    for l, P in enumerate(Ps):
        assert P.shape == (mats[l].shape[0], mats[l + 1].shape[0])
    A = [_Mat(M, dtype) for M in mats]
    P = [_Mat(Pl, dtype) for Pl in Ps]
    R = [_Mat(Pl.T, dtype) for Pl in Ps]
    for l, Rl in (restrictions or {}).items():
        R[l] = _Mat(Rl, dtype)
    one, two, half = dtype(1), dtype(2), dtype(0.5)
    dinv = [one / Al.diagonal() for Al in A]
    lam = [dtype(v) for v in lam]
    ratio, scale = dtype(k["eig_ratio"]), dtype(k["coarse_scale"])
    dense = nl > 1 and mats[-1].shape[0] <= k["dense_limit"]
    if dense:
        LU, perm = _lu(mats[-1].toarray().astype(dtype))

    def smooth(l, x, rhs, deg):
        Al, d = A[l], dinv[l]
        lmax = lam[l]
        lmin = lmax / ratio
        theta, delta = half * (lmax + lmin), half * (lmax - lmin)
        sigma = theta / delta
        rho = one / sigma
        r = rhs.copy() if x is None else rhs - Al.dot(x)
        dd = d * r / theta
        x = dd.copy() if x is None else x + dd
        for _ in range(1, deg):
            r = r - Al.dot(dd)
            rho_new = one / (two * sigma - rho)
            dd = rho_new * rho * dd + (two * rho_new / delta) * (d * r)
            x = x + dd
            rho = rho_new
        return x

    def cycle(l, rhs):
        if l == nl - 1:
            if dense:
                return _lu_solve(LU, perm, rhs)
            return smooth(l, None, rhs, k["cheb_degree"] if nl == 1 else k["coarsest_sweeps"])
        deg = k["fine_degree"] if (l == 0 and k["fine_degree"]) else k["cheb_degree"]
        x = smooth(l, None, rhs, deg)
        rc = R[l].dot(rhs - A[l].dot(x))
        xc = cycle(l + 1, rc)
        for _ in range(1, k["gamma"] if (k["gamma_from"] <= l + 1 <= k["gamma_to"] and l + 2 < nl) else 1):
            xc = xc + cycle(l + 1, rc - A[l + 1].dot(xc))
        x = x + scale * P[l].dot(xc)
        return smooth(l, x, rhs, deg)

    return lambda r: cycle(0, np.asarray(r, dtype=np.float64).astype(dtype))


def oracle_levels(A0, transfers):
    """The coarse matrices ``oracle.amg_cycle`` forms for these transfers (the same statements: the same bits)."""
    out, A = [], A0.tocsr()
    for t in transfers:
        A = galerkin_reference(A, t)[0]
        out.append(A)
    return out


def oracle_cycle(A0, transfers, knobs=None, lam_given=None):
    """``oracle.amg_cycle`` for a scipy matrix and a dict of knobs."""
    k = dict(KNOBS, **(knobs or {}))
    A0 = A0.tocsr()
    return O.amg_cycle(A0.indptr, A0.indices, A0.data, transfers, k["cheb_degree"], k["eig_ratio"], k["coarse_scale"], k["dense_limit"],
                       k["coarsest_sweeps"], k["fine_degree"], lam_given, k["gamma"], k["gamma_from"], k["gamma_to"])


def _rel_inf(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def e64(case, vectors):
    """max_v |amg_cycle(v) - cycle_ld(v)|_inf / |cycle_ld(v)|_inf for ``case`` = (A0, transfers, knobs): the oracle's fp64 cycle
    against the extended evaluation of the same levels and bounds.  From the oracle alone: no device figure enters."""
    A0, transfers, knobs = case
    M64 = oracle_cycle(A0, transfers, knobs)
    Mld = cycle_ld(A0, oracle_levels(A0, transfers), transfers, M64.lam_true, knobs)
    return max(_rel_inf(M64(np.asarray(v, dtype=np.float64)).astype(np.longdouble), Mld(v)) for v in vectors)


def apply_tolerance(e):
    """Tolerance of one application against ``cycle_ld``: 32 x e64, at least 64 eps.  Two fp64 evaluations of one operator differ by
    at least twice the rounding level; 32 leaves room for other summation orders and contracted multiply-adds."""
    return max(32.0 * e, 64.0 * EPS)
