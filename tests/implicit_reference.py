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
