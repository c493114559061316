"""The numpy mirror of the solve for several right-hand sides (pfem_solver_solve_multi).

One column is one preconditioned CG iteration: ``pcg`` is the two-reduction KSPCG recurrence of the library's single solve --
x = 0, the norm ||z|| against ttol = max(rtol ||z0||, abstol), the step of an iteration applied before its test, the tests in
the order 2, -4, -8, -3 and -10 for (p, Kp) <= 0 -- with any callable T, in float64 or longdouble.  It mirrors the semantics,
not the order of the device's sums.

The per-operation functions below it evaluate one launch of each kernel on panels (n x mb, row-major): the vector outputs by
the device's written-down float64 sequence, bit for bit (``fma`` is an exact fused multiply-add), the sums as terms in
longdouble for the any-order bound, the one-block kernels (start, verdict) in the device's own order of additions."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
BLOCK = 256                  # threads of a block
VEC_BLOCKS = 1024            # most blocks of a vector kernel
FOLD = 32                    # rows of folded product partials
IDLE, GOES_ON, LAST_STEP, BROKE = 0, 1, 2, 3


# ---- one column ----------------------------------------------------------------------------------------------------------------
def matvec_of(rowptr, cols, vals, dtype=np.float64):
    """x -> K x with the products and the row sums formed in ``dtype`` (scipy has no longdouble)"""
    v = np.asarray(vals).astype(dtype)
    rowptr = np.asarray(rowptr)
    starts = rowptr[:-1]
    empty = np.diff(rowptr) == 0

    def mv(x):
        prod = v * x[cols]
        if prod.size == 0:
            return np.zeros(len(starts), dtype)
        y = np.add.reduceat(prod, np.minimum(starts, prod.size - 1))
        y[empty] = 0
        return y
    return mv


def jacobi_of(rowptr, cols, vals, dtype=np.float64):
    """r -> r / K_ii (a row without a diagonal entry counts as 1, as on the device); the float64 form multiplies by the float64
    reciprocal like the kernels do"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    d = np.zeros(n)
    on = rows == cols
    d[rows[on]] = np.asarray(vals)[on]
    if dtype is np.float64:
        dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    else:
        dinv = np.where(d != 0.0, LD(1) / np.where(d != 0.0, d, 1.0).astype(LD), LD(1))
    return lambda r: r * dinv


def pcg(matvec, b, T, rtol=1e-5, abstol=1e-50, dtol=1e5, maxits=10000, dtype=np.float64, keep=False):
    """One column.  Returns a namespace: x, hist (||z|| of every iterate, hist[0] = ||z0||), its, reason, ttol and, with
    ``keep``, xs: the iterates x_1, x_2, ..."""
    b = np.asarray(b).astype(dtype)
    x = np.zeros_like(b)
    r = b.copy()
    z = T(r).astype(dtype)
    p = z.copy()
    rz, zz = r @ z, z @ z
    rn0 = np.sqrt(zz)
    ttol = max(dtype(rtol) * rn0, dtype(abstol))
    out = SimpleNamespace(x=x, hist=[rn0], its=0, reason=0, ttol=ttol, xs=[])
    if rn0 <= abstol:
        out.reason = 3
    elif rz < 0:
        out.reason = -8
    beta, it = rz, 0
    while out.reason == 0:
        w = matvec(p)
        pw = p @ w
        out.its = it + 1
        if not pw > 0:
            out.reason = -10
            break
        alpha = beta / pw
        r = r - alpha * w
        z = T(r).astype(dtype)
        rz, zz = r @ z, z @ z
        rn = np.sqrt(zz)
        x = x + alpha * p
        out.hist.append(rn)
        if keep:
            out.xs.append(x.copy())
        if rn <= ttol:
            out.reason = 3 if rn <= abstol else 2
        elif rn >= dtol * rn0:
            out.reason = -4
        elif rz < 0:
            out.reason = -8
        elif it + 1 >= maxits:
            out.reason = -3
        if out.reason == 0:
            p = z + (rz / beta) * p
            beta = rz
        it += 1
    out.x = x
    out.hist = np.array(out.hist, dtype=dtype)
    return out


def first_at_or_below(hist, level):
    """the first index k with hist[k] <= level, or None"""
    k = np.flatnonzero(np.asarray(hist) <= level)
    return int(k[0]) if k.size else None


# ---- an exact fused multiply-add -----------------------------------------------------------------------------------------------
def fma(a, b, c):
    """round(a b + c) entry by entry, one rounding.  longdouble holds 64 bits of the sum; where that leaves the nearest float64
    in doubt -- the value within its own error of the middle between two float64 -- the entry is formed in exact rationals."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    prod = a.astype(LD) * b.astype(LD)
    y_ld = prod + c.astype(LD)
    y = y_ld.astype(np.float64)
    below, above = np.nextafter(y, -np.inf).astype(LD), np.nextafter(y, np.inf).astype(LD)
    slack = np.minimum(y_ld - (below + y.astype(LD)) / 2, (above + y.astype(LD)) / 2 - y_ld)       # to the nearer middle
    err = (np.abs(prod) + np.abs(y_ld)) * LD(2.0) ** -62
    y = y.copy()
    for i in zip(*np.nonzero(slack <= err)):
        y[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return y


# ---- one launch of each kernel -------------------------------------------------------------------------------------------------
def vec_grid(n, mb):
    return min(VEC_BLOCKS, max(1, -(-n * mb // BLOCK)))


def block_of_entry(n, mb):
    """the block of a vector kernel's grid that handles entry e of a panel, for every e"""
    return (np.arange(n * mb) // BLOCK) % vec_grid(n, mb)


def block_partials(terms, dtype=None):
    """part[block][mb]: what each block of a vector kernel adds up of an n x mb panel of terms, whatever the order
    (longdouble for rounding data; integer-valued float64 data below 2^53 is exact in any)"""
    n, mb = terms.shape
    g = vec_grid(n, mb)
    dtype = terms.dtype if dtype is None else dtype
    part = np.zeros((g, mb), dtype)
    np.add.at(part, (block_of_entry(n, mb), np.arange(n * mb) % mb), terms.astype(dtype).ravel())
    return part


def product_partials(terms, dtype=None):
    """part_pw[block][mb] of k_spmm_dot: block b takes rows 256 b .. 256 b + 255"""
    n, mb = terms.shape
    nb = -(-n // BLOCK)
    dtype = terms.dtype if dtype is None else dtype
    t = np.zeros((nb * BLOCK, mb), dtype)
    t[:n] = terms
    return t.reshape(nb, BLOCK, mb).sum(axis=1)


def fold_chunks(part_pw, dtype=None):
    """fold_pw[32][mb] of k_mcg_fold: block b sums rows b chunk .. b chunk + chunk - 1"""
    nb, mb = part_pw.shape
    dtype = part_pw.dtype if dtype is None else dtype
    chunk = -(-nb // FOLD)
    out = np.zeros((FOLD, mb), dtype)
    for b in range(FOLD):
        out[b] = part_pw[b * chunk:min(nb, (b + 1) * chunk)].astype(dtype).sum(axis=0)
    return out


def folded(fold_pw):
    """(p, Kp) per column as k_mcg_update reads it: the 32 rows added in index order, in float64"""
    a = np.zeros(fold_pw.shape[1])
    for row in np.asarray(fold_pw, np.float64):
        a = a + row
    return a


def init_op(B, dinv=None):
    """X, R, P and Z of k_mcg_init (P = Z = dinv o R; without dinv P and Z are None)"""
    Z = None if dinv is None else B * dinv[:, None]
    return np.zeros_like(B), B.copy(), Z, Z


def dot_terms(R, Z, dtype=LD):
    """the terms of (r,z) and (z,z) per column from float64 panels"""
    r, z = R.astype(dtype), Z.astype(dtype)
    return r * z, z * z


def finish(part):
    """tot[2][mb] of the one-block kernels from part[nparts][2][mb], in their order: thread t adds the rows t // (2 mb),
    t // (2 mb) + 256 / (2 mb), ... of entry t % (2 mb), then thread c < 2 mb adds those sums in thread order -- float64"""
    nparts, _, mb = part.shape
    w = 2 * mb
    ng = BLOCK // w
    flat = np.asarray(part, np.float64).reshape(nparts, w)
    sm = np.zeros((ng, w))
    for g in range(ng):
        for row in flat[g::ng]:
            sm[g] = sm[g] + row
    tot = np.zeros(w)
    for g in range(ng):
        tot = tot + sm[g]
    return tot.reshape(2, mb)


def new_ctl(mb):
    c = {f: np.zeros(mb) for f in ("rn0", "ttol", "rn", "alpha", "bb")}
    c.update({f: np.zeros(mb, np.int32) for f in ("flag", "its", "verdict")})
    c["beta"] = np.zeros((mb, 2))
    c["running"], c["step"] = 0, 0
    return c


def copy_ctl(c):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def start_op(tot, rtol, abstol):
    """k_mcg_start from the finished sums tot[2][mb]"""
    mb = tot.shape[1]
    c = new_ctl(mb)
    rz, zz = tot
    rn0 = np.sqrt(zz)
    c["beta"][:, 0] = rz
    c["rn0"][:] = rn0
    c["rn"][:] = rn0
    c["ttol"][:] = np.maximum(rtol * rn0, abstol)
    c["flag"][:] = np.where(rn0 <= abstol, 3, np.where(rz < 0.0, -8, 0))
    c["running"] = int((c["flag"] == 0).sum())
    return c


def update_op(ctl, fold_pw, W, R, dinv=None):
    """k_mcg_update: (ctl', R', broke) -- alpha of the running columns, R' = fma(-alpha, W, R) there, every other column as it
    was; broke: the running columns whose (p, Kp) is not positive (they keep R and get the -1 marker)"""
    c = copy_ctl(ctl)
    mb = R.shape[1]
    out = R.copy()
    broke = np.zeros(mb, bool)
    if c["running"] == 0:
        return c, out, broke
    pw = folded(fold_pw)
    for j in np.flatnonzero(c["flag"] == 0):
        if not pw[j] > 0.0:
            broke[j] = True
            continue
        c["alpha"][j] = c["beta"][j][c["step"] & 1] / pw[j]
        out[:, j] = fma(-c["alpha"][j], W[:, j], R[:, j])
    return c, out, broke


def verdict_op(ctl, tot, dtol, maxits):
    """k_mcg_verdict from the finished sums tot[2][mb]"""
    c = copy_ctl(ctl)
    mb = tot.shape[1]
    if c["running"] == 0:
        c["verdict"][:] = IDLE
        return c
    it = c["step"]
    for j in range(mb):
        if c["flag"][j] != 0:
            c["verdict"][j] = IDLE
            continue
        rz, zz = tot[0][j], tot[1][j]
        c["its"][j] = it + 1
        if zz < 0.0:
            c["flag"][j], c["verdict"][j] = -10, BROKE
            continue
        rn = np.sqrt(zz)
        flag = 0
        if rn <= c["ttol"][j]:
            flag = 2
        elif rn >= dtol * c["rn0"][j]:
            flag = -4
        elif rz < 0.0:
            flag = -8
        elif it + 1 >= maxits:
            flag = -3
        with np.errstate(divide="ignore", invalid="ignore"):
            c["bb"][j] = rz / c["beta"][j][it & 1]
        c["beta"][j][(it + 1) & 1] = rz
        c["rn"][j] = rn
        c["flag"][j] = flag
        c["verdict"][j] = LAST_STEP if flag != 0 else GOES_ON
    c["running"] = int((c["flag"][:mb] == 0).sum())
    c["step"] = it + 1
    return c


def direction_op(ctl, R, P, X, dinv=None, Z=None):
    """k_mcg_direction: (P', X') -- X' = fma(alpha, P, X) in the columns whose verdict is 1 or 2, P' = fma(bb, P, z) with
    z = R dinv (float64 product) or the stored Z in those whose verdict is 1"""
    P2, X2 = P.copy(), X.copy()
    for j in range(R.shape[1]):
        v = ctl["verdict"][j]
        if v not in (GOES_ON, LAST_STEP):
            continue
        X2[:, j] = fma(ctl["alpha"][j], P[:, j], X[:, j])
        if v == GOES_ON:
            z = R[:, j] * dinv if dinv is not None else Z[:, j]
            P2[:, j] = fma(ctl["bb"][j], P[:, j], z)
    return P2, X2
