"""numpy mirror of the explicit dynamics (pfem_elem_lumped_mass, pfem_dynamics_*): the element lumped mass in the reference's
order of operations, the nodal sum in ascending element order, the central-difference recurrence on the K and load of
materials_reference.setup_problem, the sums T, S, W, the load curve and the Gershgorin step -- each in the order of operations
the library documents, so that everything but the product K u (whose order of summation belongs to the SpMV form) can be
matched bit for bit."""
import numpy as np
import scipy.sparse as sp

from oracle import pfem_oracle as O
from post_reference import element_weights

EPS = np.finfo(np.float64).eps
GAUSS_PT_TRIA = float(np.float32(1.0) / np.float32(3.0))      # the triangle routines' REAL(4) Gauss point


def shape_values(npe):
    """N at the one Gauss point: 1/4 each for the tet, (1 - xi - xi, xi, xi) with the REAL(4) xi for the triangle."""
    if npe == 4:
        return np.array([0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25])
    xi = GAUSS_PT_TRIA
    return np.array([1.0 - xi - xi, xi, xi])


def element_lumped_mass(xyz, conn, dens, thick=1.0):
    """(npe, nElem): Mn[a] = sum over j ascending of ((dens * dvol) * N[a]) * N[j], from 0.0 -- MassMatrixLinearTria /
    MassMatrixLinearTetra with the structural zeros left out.  dens and thick: numbers or one per element."""
    dvol = element_weights(xyz, conn, thick)
    N = shape_values(conn.shape[0])
    c = dens * dvol
    out = np.empty((conn.shape[0], conn.shape[1]))
    for a in range(conn.shape[0]):
        b4 = c * N[a]
        fact = np.zeros(conn.shape[1])
        for j in range(conn.shape[0]):
            fact = fact + b4 * N[j]
        out[a] = fact
    return out


def nodal_mass(conn, Mn, nNode):
    """Sum of the nodes' shares in ascending element order (np.add.at applies its updates one after the other), and the
    number of elements at every node."""
    m = np.zeros(nNode)
    cnt = np.zeros(nNode, np.int64)
    np.add.at(m, conn.T.ravel(), Mn.T.ravel())
    np.add.at(cnt, conn.T.ravel(), 1)
    return m, cnt


def free_dof_mass(p, dens, thick=1.0):
    """(m per free dof, elements at that dof's node, nodal masses) for a materials_reference.Problem; dens / thick per element
    or numbers."""
    Mn = element_lumped_mass(p.xyz_new, p.conn_new, dens, thick)
    mn, cnt = nodal_mass(p.conn_new, Mn, p.xyz_new.shape[1])
    nda = p.dm.NodeDofArrayNew
    N = len(p.rowptr) - 1
    m, k = np.zeros(N), np.zeros(N, np.int64)
    node = np.broadcast_to(np.arange(nda.shape[0])[:, None], nda.shape)
    m[nda[nda >= 0]] = mn[node[nda >= 0]]
    k[nda[nda >= 0]] = cnt[node[nda >= 0]]
    return m, k, mn


def csr(p, reverse=False):
    """K as scipy CSR, the entries of a row in ascending column order -- or, ``reverse``, in descending order: scipy's product
    adds a row's terms in the stored order."""
    N = len(p.rowptr) - 1
    if not reverse:
        return sp.csr_matrix((p.vals, p.cols, p.rowptr), shape=(N, N))
    rows = np.repeat(np.arange(N), np.diff(p.rowptr))
    perm = p.rowptr[rows + 1] - 1 - (np.arange(len(p.cols)) - p.rowptr[rows])
    A = sp.csr_matrix((p.vals[perm], p.cols[perm], p.rowptr), shape=(N, N))
    A.has_sorted_indices = False
    return A


def gershgorin_dt(A, m):
    """2 / sqrt(max_i (sum_j |K_ij|) / m_i), a row's entries added in ascending column order."""
    rowsum = abs(A) @ np.ones(A.shape[0])
    minv = np.where(m > 0.0, 1.0 / np.where(m > 0.0, m, 1.0), 0.0)
    return 2.0 / np.sqrt((rowsum * minv).max())


def load_factor(curve, t):
    """lambda(t): piecewise linear through (ct[k], cl[k]), constant outside; ``None``: 1."""
    if curve is None:
        return 1.0
    ct, cl = (np.asarray(a, dtype=np.float64) for a in curve)
    if t <= ct[0]:
        return float(cl[0])
    if t >= ct[-1]:
        return float(cl[-1])
    lo = int(np.searchsorted(ct, t, side="right")) - 1
    return float(cl[lo] + (cl[lo + 1] - cl[lo]) * ((t - ct[lo]) / (ct[lo + 1] - ct[lo])))


def modes(A, m):
    """omega (ascending) and the eigenvectors phi of M^-1 K (columns), by dense eigh of M^-1/2 K M^-1/2."""
    d = 1.0 / np.sqrt(m)
    lam, V = np.linalg.eigh(d[:, None] * A.toarray() * d[None, :])
    return np.sqrt(np.maximum(lam, 0.0)), d[:, None] * V


class Stepper:
    """The recurrence of pfem_dynamics_run, divided through by m:
        u_{n+1} = [ c0 (2 u_n - u_{n-1}) + c1 u_{n-1} + (lambda(t_n) f - K u_n) / m ] / (c0 + c1),
    c0 = 1 / dt^2, c1 = alpha / (2 dt), t_n = t0 + n dt, started from u_{-1} = (u0 - dt v0) + (dt^2 / 2) a0 with
    a0 = (lambda(t0) f - K u0) / m.  ``step`` returns (t_{n+1}, T, S, W) with T = 1/2 sum m v^2, v = (u_{n+1} - u_n) / dt,
    S = 1/2 u_{n+1} . K u_n, W = f . u_{n+1}."""

    def __init__(self, A, f, m, dt, alpha=0.0, t0=0.0, u0=None, v0=None, curve=None):
        self.A, self.f, self.m, self.dt, self.t0, self.curve = A, f, m, dt, t0, curve
        self.minv = np.where(m > 0.0, 1.0 / np.where(m > 0.0, m, 1.0), 0.0)
        self.c0 = 1.0 / (dt * dt)
        self.c1 = alpha / (2.0 * dt)
        self.a = self.c0 + self.c1
        N = A.shape[0]
        self.u = np.zeros(N) if u0 is None else np.array(u0, dtype=np.float64)
        v0 = np.zeros(N) if v0 is None else np.asarray(v0, dtype=np.float64)
        a0 = (load_factor(curve, t0) * f - A @ self.u) * self.minv
        self.up = (self.u - dt * v0) + (0.5 * (dt * dt)) * a0
        self.n = 0

    @property
    def t(self):
        return self.t0 + float(self.n) * self.dt

    @property
    def v(self):
        return (self.u - self.up) / self.dt

    def step(self):
        u, up = self.u, self.up
        w = self.A @ u
        lam = load_factor(self.curve, self.t)
        x = (((2.0 * u - up) * self.c0 + self.c1 * up) + (lam * self.f - w) * self.minv) / self.a
        v = (x - u) / self.dt
        self.up, self.u = u, x
        self.n += 1
        self.magnitudes = (0.5 * np.sum(self.m * (v * v)), 0.5 * (np.abs(x) @ np.abs(w)), np.abs(self.f) @ np.abs(x))
        return self.t, 0.5 * np.sum(self.m * (v * v)), 0.5 * (x @ w), self.f @ x

    def run(self, n_steps, sample_every=0, magnitudes=False):
        """The rows of the sampled steps; ``magnitudes``: three more columns, the sums of the absolute values of the terms of
        T, S and W (what the rounding of a sum in another order is measured against)."""
        rows = []
        for k in range(1, n_steps + 1):
            r = self.step()
            if sample_every and k % sample_every == 0:
                rows.append(r + self.magnitudes if magnitudes else r)
        return np.array(rows).reshape(-1, 7 if magnitudes else 4)


def poisson_box(H, n=10):
    """(Problem, mass per free dof) of the n^3 x 6-tet Poisson box on [-1, 1]^3, unit conductivity, unit density: the mesh of
    the closed-form checks (n = 10: 729 free dofs).  ``H`` = pfemfort_amd.host."""
    import materials_reference as MR
    mesh = H.gen_box_tets(-1, 1, n, -1, 1, n, -1, 1, n)
    p = MR.setup_problem(O.POISSON_TET, mesh, H.POISSON_ELEMDATA[None, :], np.zeros(mesh.nElem, np.int32))
    m, _, _ = free_dof_mass(p, 1.0)
    return mesh, p, m


# ---- one launch of the step kernel, operation by operation (tests/test_gpu_stepper_kernels.py) --------------------------------
BLOCK_ROWS = 1024          # rows of a block of the steppers' vector kernels: 256 threads x 4 consecutive rows
LD = np.longdouble


def block_sums(terms, blocks, dtype=None):
    """The sum of ``terms`` over the rows r with (r // 1024) % blocks == b, for every b: what block b of a grid of ``blocks``
    blocks adds up, whatever the order.  ``dtype``: the type the sums are formed in (longdouble for rounding data; integer-valued
    float64 data below 2^53 is exact in any)."""
    terms = np.asarray(terms)
    dtype = terms.dtype if dtype is None else dtype
    per = blocks * BLOCK_ROWS
    trips = -(-terms.size // per)
    t = np.zeros(trips * per, dtype)
    t[:terms.size] = terms
    return t.reshape(trips, blocks, BLOCK_ROWS).sum(axis=(0, 2))


def step_par(dt, alpha):
    """(c0, c1, a) of a run's parameter block: 1 / dt^2, alpha / (2 dt), c0 + c1"""
    c0 = 1.0 / (dt * dt)
    c1 = alpha / (2.0 * dt)
    return c0, c1, c0 + c1


def step_kernel(dt, alpha, lam, f, m, minv, w, u, up):
    """k_dyn_step's rows in its written order of float64 operations: (u_{n+1}, the terms of T, of S and of W)."""
    c0, c1, a = step_par(dt, alpha)
    x = (((2.0 * u - up) * c0 + c1 * up) + (lam * f - w) * minv) / a
    v = (x - u) / dt
    return x, m * (v * v), x * w, f * x


def step_terms_ld(dt, x, f, m, w, u):
    """the terms of T, S, W in longdouble from the float64 u_{n+1} = x and v = (x - u) / dt the kernel formed"""
    v = ((x - u) / dt).astype(LD)
    return m.astype(LD) * (v * v), x.astype(LD) * w.astype(LD), f.astype(LD) * x.astype(LD)


def step_row(t0, dt, step, T, S, W, un, u, probes):
    """the history row of the sampled step `step` -> `step` + 1 from the totals"""
    probes = np.asarray(probes, dtype=np.int64)
    return np.concatenate([[t0 + float(step + 1) * dt, 0.5 * T, 0.5 * S, W], un[probes], (un[probes] - u[probes]) / dt])
