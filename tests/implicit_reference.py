"""numpy mirror of the implicit time stepping (pfem_dynamics_run_implicit): Newmark (beta, gamma) in increment form and the
theta-method on a lumped mass, each step one solve (K + sigma diag(m)) d = b from d = 0 -- by sparse LU, or by the Jacobi-PCG
the device runs (two-reduction KSPCG, preconditioner 1 / (K_ii + sigma m_i), the norm ||z|| relative to ||z_0||, the same
stopping rule).  Outside the solve every value is formed by the sequence of operations the library documents.  K, the load
curve and the modes are dynamics_reference's."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from dynamics_reference import csr, load_factor, modes      # noqa: F401  (re-exported: the mirror's K, lambda(t) and modes)

EPS = np.finfo(np.float64).eps


def pcg_shifted(A, sm, dinv, b, rtol=1e-5, abstol=1e-50, dtol=1e5, maxits=10000):
    """(d, iterations, reason) of Jacobi-PCG on (A + diag(sm)) d = b from d = 0: KSPCG's order -- the update, then the test on
    ||z|| -- with reasons 2 / 3 (converged), -3 (maxits), -4 (dtol), -8 (indefinite pc), -10 (indefinite matrix)."""
    d = np.zeros_like(b)
    r = b.copy()
    z = r * dinv
    p = z.copy()
    beta = r @ z
    rn0 = np.sqrt(z @ z)
    if rn0 <= abstol:
        return d, 0, 3
    if beta < 0.0:
        return d, 0, -8
    ttol = max(rtol * rn0, abstol)
    for it in range(maxits):
        w = A @ p
        pw = p @ w + (sm * p) @ p
        if not pw > 0.0:
            return d, it + 1, -10
        a = beta / pw
        r = r - a * (w + sm * p)
        z = r * dinv
        rz, rn = r @ z, np.sqrt(z @ z)
        d = d + a * p
        if rn <= ttol:
            return d, it + 1, 2
        if rn >= dtol * rn0:
            return d, it + 1, -4
        if rz < 0.0:
            return d, it + 1, -8
        if it + 1 >= maxits:
            return d, it + 1, -3
        p = z + (rz / beta) * p
        beta = rz
    return d, 0, -3            # (maxits = 0)


class ImplicitStepper:
    """scheme "newmark" (beta, gamma, damping alpha M; started from a_0 = (lambda(t0) f - alpha m v0 - K u0) / m):
        ut = (u + dt v) + dt^2 (1/2 - beta) a,  vt = v + dt (1 - gamma) a,  sigma = (1 + gamma dt alpha) / (beta dt^2),
        b = lambda(t_{n+1}) f - alpha (m vt) - K ut,  u' = ut + d,  a' = d / (beta dt^2),  v' = vt + (gamma dt) a'
    scheme "theta":
        sigma = 1 / (theta dt),  b = [theta lambda(t_{n+1}) + (1 - theta) lambda(t_n)] f - K u,  u' = u + d / theta,
        v' = (u' - u) / dt.
    t_n = t0 + n dt.  A row with m = 0 stays put: b = 0 and its shifted diagonal counts as 1.  ``solve``: "lu" (splu of the
    shifted matrix) or "pcg" (``pcg_shifted`` with rtol, abstol, dtol, maxits).  ``A`` may be dynamics_reference.csr's reversed
    matrix: the products then add a row's terms in the other order.  ``iterations`` collects the count of every step."""

    def __init__(self, A, f, m, dt, scheme="newmark", beta=0.25, gamma=0.5, theta=1.0, alpha=0.0, t0=0.0, u0=None, v0=None, curve=None,
                 solve="lu", rtol=1e-5, abstol=1e-50, dtol=1e5, maxits=10000):
        if scheme not in ("newmark", "theta"):
            raise ValueError(scheme)
        self.A, self.f, self.m, self.dt, self.t0, self.curve, self.scheme = A, f, m, dt, t0, curve, scheme
        self.alpha, self.theta, self.solve = alpha, theta, solve
        self.tol = dict(rtol=rtol, abstol=abstol, dtol=dtol, maxits=maxits)
        N = A.shape[0]
        self.has_m = m > 0.0
        self.u = np.zeros(N) if u0 is None else np.array(u0, dtype=np.float64)
        self.v = np.zeros(N) if v0 is None else np.array(v0, dtype=np.float64)
        if scheme == "newmark":
            if not (beta > 0.0 and gamma >= 0.5):
                raise ValueError("beta > 0 and gamma >= 1/2")
            self.bdt2 = beta * (dt * dt)
            self.gdt = gamma * dt
            self.sigma = (1.0 + self.gdt * alpha) / self.bdt2
            self.cu = (dt * dt) * (0.5 - beta)
            self.cv = dt * (1.0 - gamma)
            num = (load_factor(curve, t0) * f - alpha * (m * self.v)) - A @ self.u
            self.a = np.where(self.has_m, num / np.where(self.has_m, m, 1.0), 0.0)
        else:
            if not (0.0 < theta <= 1.0) or alpha != 0.0:
                raise ValueError("theta in (0, 1] and alpha = 0")
            self.sigma = 1.0 / (theta * dt)
        self.sm = self.sigma * m
        diag = A.diagonal()
        self.dinv = np.where(self.has_m, 1.0 / np.where(self.has_m, diag + self.sm, 1.0), 1.0)
        self._lu = None
        self.n = 0
        self.iterations = []
        self.reason = 0

    @property
    def t(self):
        return self.t0 + float(self.n) * self.dt

    def _solve(self, b):
        if self.solve == "lu":
            if self._lu is None:
                shift = np.where(self.has_m, self.sm, 1.0)
                self._lu = spl.splu(sp.csc_matrix(sp.csr_matrix(self.A) + sp.diags(shift)))
            self.iterations.append(0)
            return self._lu.solve(b)
        d, its, reason = pcg_shifted(self.A, self.sm, self.dinv, b, **self.tol)
        self.reason = reason
        if reason < 0:
            raise RuntimeError(f"step {self.n}: reason {reason} after {its} iterations")
        self.iterations.append(its)
        return d

    def step(self):
        A, f, m, dt = self.A, self.f, self.m, self.dt
        t1 = self.t0 + float(self.n + 1) * dt
        if self.scheme == "newmark":
            ut = (self.u + dt * self.v) + self.cu * self.a
            vt = self.v + self.cv * self.a
            b = (load_factor(self.curve, t1) * f - self.alpha * (m * vt)) - A @ ut
            d = self._solve(np.where(self.has_m, b, 0.0))
            self.u = ut + d
            self.a = d / self.bdt2
            self.v = vt + self.gdt * self.a
            kin = self.v
        else:
            lam = self.theta * load_factor(self.curve, t1)
            if 1.0 - self.theta != 0.0:
                lam = lam + (1.0 - self.theta) * load_factor(self.curve, self.t)
            b = lam * f - A @ self.u
            d = self._solve(np.where(self.has_m, b, 0.0))
            un = self.u + d / self.theta
            self.v = (un - self.u) / dt
            self.u = un
            kin = self.u
        self.n += 1
        w = A @ self.u
        T, S, W = 0.5 * np.sum(m * (kin * kin)), 0.5 * (self.u @ w), f @ self.u
        self.magnitudes = (T, 0.5 * (np.abs(self.u) @ np.abs(w)), np.abs(f) @ np.abs(self.u))
        return self.t, T, S, W

    def run(self, n_steps, sample_every=0, magnitudes=False):
        """The rows [t, T, S, W] of the sampled steps; ``magnitudes``: three more columns, the sums of the absolute values of
        the terms of T, S and W."""
        rows = []
        for k in range(1, n_steps + 1):
            r = self.step()
            if sample_every and k % sample_every == 0:
                rows.append(r + self.magnitudes if magnitudes else r)
        return np.array(rows).reshape(-1, 7 if magnitudes else 4)


# ---- one launch of each kernel of a step, operation by operation (tests/test_gpu_stepper_kernels.py) --------------------------
from fractions import Fraction      # noqa: E402

from dynamics_reference import LD, block_sums      # noqa: E402,F401


class Par:
    """The parameter block of a run, by ImplicitStepper's arithmetic (which is the library's)."""

    def __init__(self, scheme, dt, beta=0.25, gamma=0.5, theta=1.0, alpha=0.0):
        self.scheme, self.dt, self.alpha, self.theta = scheme, dt, alpha, theta
        if scheme == "newmark":
            self.bdt2 = beta * (dt * dt)
            self.gdt = gamma * dt
            self.sigma = (1.0 + self.gdt * alpha) / self.bdt2
            self.cu = (dt * dt) * (0.5 - beta)
            self.cv = dt * (1.0 - gamma)
        else:
            self.sigma = 1.0 / (theta * dt)


def predict(P, u, v, a):
    """(ut, vt) in float64, the kernel's order"""
    return (u + P.dt * v) + P.cu * a, v + P.cv * a


def rhs_load_factor(P, curve, t_base, step):
    """lambda of the right-hand side of step `step`: Newmark lambda(t_{n+1}); theta-method theta lambda(t_{n+1}) +
    (1 - theta) lambda(t_n), the second term only where 1 - theta is not zero"""
    tn0, tn1 = t_base + float(step) * P.dt, t_base + float(step + 1) * P.dt
    if P.scheme == "newmark":
        return 1.0 * load_factor(curve, tn1)
    ln0 = 1.0 - P.theta
    lam = P.theta * load_factor(curve, tn1)
    return lam + ln0 * load_factor(curve, tn0) if ln0 != 0.0 else lam


def rhs(P, lam, f, m, vt, w, dinv):
    """(b, z) in float64: r = b, p = z, d = 0"""
    load = lam * f - P.alpha * (m * vt) if P.scheme == "newmark" else lam * f
    b = np.where(m > 0.0, load - w, 0.0)
    return b, b * dinv


def dot_terms(P, r, dinv, m, p, dtype=LD):
    """the terms of (r, z), (z, z) with z = r dinv, and of sum sigma m p^2 with the float64 product sigma m, formed in
    `dtype` from float64 vectors"""
    r_, q_, p_ = r.astype(dtype), dinv.astype(dtype), p.astype(dtype)
    z = r_ * q_
    return r_ * z, z * z, ((P.sigma * m).astype(dtype) * p_) * p_


def update(P, alpha, p, w, m, r, dtype=LD):
    """r' = r - alpha ((sigma m) p + w) in `dtype`, and the magnitude |alpha| (|sigma m p| + |w|) + |r'| its rounding is
    measured against (two fma: at most eps / 2 of each part)"""
    sm = (P.sigma * m).astype(dtype)
    t = sm * p.astype(dtype)
    out = r.astype(dtype) - dtype(alpha) * (t + w.astype(dtype))
    return out, abs(dtype(alpha)) * (np.abs(t) + np.abs(w.astype(dtype))) + np.abs(out)


def direction(alpha, bb, r, dinv, p, d, dtype=LD):
    """d' = d + alpha p (in longdouble: to well below eps |d'| in every row, see below); p' = bb p + (r dinv) with the float64
    product r dinv; and the magnitude |bb p| + |r dinv| + |p'|"""
    z = (r * dinv).astype(dtype)
    t = dtype(bb) * p.astype(dtype)
    ap = dtype(alpha) * p.astype(dtype)
    d2 = d.astype(dtype) + ap
    if dtype is LD:
        # d' is measured against |d'| alone, and the product alpha p holds 106 bits, 64 of which longdouble keeps: where the sum
        # cancels more than 2^8-fold the rounded product would spend the bound, so those rows are formed in exact rationals
        for i in np.flatnonzero(np.abs(ap) > 256.0 * np.abs(d2)):
            x = Fraction(float(alpha)) * Fraction(float(p[i])) + Fraction(float(d[i]))
            hi = float(x)
            d2[i] = LD(hi) + LD(float(x - Fraction(hi)))
    p2 = t + z
    return d2, p2, np.abs(t) + np.abs(z) + np.abs(p2)


def correct(P, d, u=None, ut=None, vt=None):
    """(u, v, a) in float64, the kernel's order; the theta-method has no a"""
    if P.scheme == "newmark":
        a = d / P.bdt2
        return ut + d, vt + P.gdt * a, a
    x = u + d / P.theta
    return x, (x - u) / P.dt, None


def energy_terms(P, f, m, u, v, w, dtype=LD):
    """the terms of T (theta-method: m u^2), S and W"""
    k = (v if P.scheme == "newmark" else u).astype(dtype)
    return m.astype(dtype) * (k * k), u.astype(dtype) * w.astype(dtype), f.astype(dtype) * u.astype(dtype)
