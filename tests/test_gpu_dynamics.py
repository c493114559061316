"""Explicit dynamics on the device (pfem_dynamics_*): the lumped mass, the Gershgorin step, 300 central-difference steps, a
single mode, the invariant T + S, the static limit, continuation across runs, the history rows and the state errors -- against
the numpy mirror (tests/dynamics_reference.py, itself checked against closed forms in tests/test_dynamics_reference.py).

The mirror runs on the K and the load the device holds (getCSR / getRHS, pinned against the oracle by older tests).  Every
bound is computed here, for the mesh at hand: 16 x the figure the mirror itself reaches -- against the closed form, or, for a
trajectory, against itself with every row's products added in reverse order.  The factor covers the one thing the device does
differently: the SpMV adds a row in slices, with fma."""
import os
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import dynamics_reference as DR
import modal_reference as MO
import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_parity import _hub_mesh, _shuffled

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ANISO = np.array([1.3, 0.7, 2.1])
COOK_DATA = np.array([H.ELAST_ELEMDATA[0], H.ELAST_ELEMDATA[1], 0.5, 0.05, -0.02])     # E, nu, thick, body force
BEAM_TABLE = np.array([[300.0, 0.3, 1.0, 0.0, -0.1, 0.0], [900.0, 0.2, 1.0, 0.05, 0.0, 0.0]])
NAMES = ["tet10", "cook", "beam2", "hub", "hub_elast"]
PLAIN = ["tet10", "cook", "beam2"]


@contextmanager
def reorder_env(value):
    """PFEM_REORDER = value (None: unset) inside the block, as it was afterwards"""
    old = os.environ.pop("PFEM_REORDER", None)
    if value is not None:
        os.environ["PFEM_REORDER"] = value
    try:
        yield
    finally:
        os.environ.pop("PFEM_REORDER", None)
        if old is not None:
            os.environ["PFEM_REORDER"] = old


class Case:
    """One mesh on the device, assembled, with its mass; the mirror's matrix, load, mass and modes -- made once.  A name that
    ends in _r: the mesh of that name under a random node numbering (test_gpu_parity._shuffled, seed 7), uploaded with
    PFEM_REORDER=1, so that the library holds it renumbered; in _s: the same numbering with PFEM_REORDER unset, the
    renumbering left to the library's own test."""

    def __init__(self, name, golden_dir):
        self.name = name
        self.table = self.ids = None
        self.density = 2.5
        self.reorder = {"_r": "1", "_s": None}.get(name[-2:], False)       # False: the environment as it stands
        if self.reorder is not False:
            name = name[:-2]
        self.base = name
        if name == "tet10":
            self.kind, self.ed, self.mesh = pf.POISSON_TET, ANISO, H.read_mesh(f"{golden_dir}/input/tet10")
        elif name == "cook":
            self.kind, self.ed, self.mesh = pf.ELAST_TRIA, COOK_DATA, H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
        elif name == "beam2":                # the small elastic box, two materials of different densities
            self.kind, self.mesh = pf.ELAST_TET, H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
            self.ed = self.table = BEAM_TABLE
            self.ids = (self.mesh.xyz[1][self.mesh.conn].mean(0) > 2.0).astype(np.int32)
            self.density = np.array([3.0, 11.0])
        elif name == "box19k":               # 19 656 dofs: beyond one pass of the modal kernels' capped grids (test_gpu_modal.py)
            self.kind, self.ed, self.mesh = pf.POISSON_TET, ANISO, H.gen_box_tets(-1, 1, 28, -0.9, 0.9, 27, -0.8, 0.8, 29)
        elif name == "hub":
            self.kind, self.ed, self.mesh = pf.POISSON_TET, ANISO, _hub_mesh(300, 1)
        else:
            self.kind, self.ed, self.mesh = pf.ELAST_TET, H.ELAST_ELEMDATA, _hub_mesh(100, 3)
        if self.reorder is not False:
            self.plain_mesh, self.mesh = self.mesh, _shuffled(self.mesh, seed=7)
        self.ndof = L.NDOF[self.kind]
        self.dm, self.conn, self.xyz, edof = D._setup(self.kind, self.mesh)
        self.N = self.dm.size_global
        s = self.s = pf.PetscSolver().initialise(self.N, self.N)
        if self.reorder is False:
            s.uploadMesh(self.kind, self.conn, self.xyz, edof, self.dm.solnApplied)
        else:
            with reorder_env(self.reorder):
                s.uploadMesh(self.kind, self.conn, self.xyz, edof, self.dm.solnApplied)
        if self.ids is not None:
            s.setMaterials(self.ids, n_mat=2, stride=6)
        s.buildPattern()
        s.assemble(self.ed, H.TIMEDATA)
        if self.base == "cook":              # a surface load and the nodal forces of the mesh's force file
            fe, fs = s.boundaryFaces()
            on = np.all(self.xyz[0][s.surfaceGeometry(fe, fs)[2]] == 48.0, axis=0)
            s.addSurfaceLoad(fe[on], fs[on], "traction", [0.5, 6.25], elemData=self.ed)
        self.total = s.dynamicsSetup(self.ed, self.density)
        rowptr, cols, vals = s.getCSR()
        self.p = SimpleNamespace(xyz_new=self.xyz, conn_new=self.conn, dm=self.dm, rowptr=rowptr, cols=cols, vals=vals, rhs=s.getRHS())
        self.A, self.Arev, self.f = DR.csr(self.p), DR.csr(self.p, reverse=True), self.p.rhs
        dens = self.density if self.ids is None else self.density[self.ids]
        thick = self.ed[2] if self.kind == pf.ELAST_TRIA else 1.0
        self.m_mirror, self.k, self.mnode = DR.free_dof_mass(self.p, dens, thick)
        # the mirror steps with the mass the device holds: the mirror's own bit for bit where every node has one writer, within
        # (k - 1) eps at a hub (test_mass_equals_the_mirror checks both)
        self.m = s.dynamicsMass()
        self.dt = DR.gershgorin_dt(self.A, self.m)
        self._modes = None

    def modes(self):
        """(omega ascending, M-orthonormal vectors): all of them by dense eigh; of box19k the lowest 13 by shift-invert Lanczos"""
        if self._modes is None:
            if self.base == "box19k":
                lam, phi = MO.lowest_modes(self.A, self.m, 13)
                self._modes = (np.sqrt(lam), phi)
            else:
                self._modes = DR.modes(self.A, self.m)
        return self._modes

    def mirror(self, A=None, **kw):
        return DR.Stepper(self.A if A is None else A, self.f, self.m, **kw)

    def device(self, t0=0.0, u0=None, v0=None, curve=None, probes=()):
        self.s.setLoadCurve(*(curve if curve is not None else (None, None)))
        self.s.setProbes(probes)
        self.s.setDynamicsState(t0, u0, v0)
        return self.s


_CASES = {}


def get_case(name, golden_dir):
    if name not in _CASES:
        _CASES[name] = Case(name, golden_dir)
    return _CASES[name]


@pytest.fixture
def case(request, golden_dir):
    return get_case(request.param, golden_dir)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


# ---- mass and the stable step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_mass_equals_the_mirror(case):
    """Bit for bit where every node has one writer; at a hub node of k elements (f64 atomics, any order) within (k-1) eps
    relative, the bound for a sum of k positive terms in any order.  The total is the sum over ALL nodes."""
    c = case
    got, want = c.s.dynamicsMass(), c.m_mirror
    assert got.shape == want.shape and (got > 0).all()
    hubs = c.s.assemblyInfo()["hub_nodes"]
    if c.name.startswith("hub"):
        assert hubs >= 1
        bound = (c.k - 1) * EPS * want
        print(f"{c.name}: largest mass deviation {np.abs(got / want - 1).max():.3e}, most elements at a node {c.k.max()}")
        assert (np.abs(got - want) <= bound).all()
        plain = c.k <= 64                      # (a hub has hundreds of elements)
        assert plain.any() and not plain.all() and np.array_equal(got[plain], want[plain])
    else:
        assert hubs == 0
        assert np.array_equal(got, want)
    n = len(c.mnode)
    assert abs(c.total - c.mnode.sum()) <= n * EPS * c.mnode.sum()
    if c.name == "tet10":
        assert c.N == 729
        assert c.total == pytest.approx(2.5 * DR.element_weights(c.xyz, c.conn).sum(), rel=1e-12)      # density x volume


@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_mass_in_the_scatter_form(case):
    """The assembly mode "scatter", set before the pattern is built: the element pass sums every node by f64 atomics (the default
    mode runs that pass for hub nodes only).  The element shares are the mirror's bit for bit (test_mass_equals_the_mirror's
    array_equal); only the order of a sum of k positive terms differs, and every order lies within (k - 1) eps / 2 relative of
    the exact sum: (k - 1) eps between two of them.  A solver of its own: the cached case keeps its mode."""
    c = case
    s = pf.PetscSolver().initialise(c.N, c.N)
    try:
        s.uploadMesh(c.kind, c.conn, c.xyz, D._setup(c.kind, c.mesh)[3], c.dm.solnApplied)
        if c.ids is not None:
            s.setMaterials(c.ids, n_mat=2, stride=6)
        s.setAssemblyMode("scatter")
        s.buildPattern()
        assert not s.assemblyInfo()["gather"]         # (the mode took: the element pass sums every node)
        s.assemble(c.ed, H.TIMEDATA)
        total = s.dynamicsSetup(c.ed, c.density)
        got, want = s.dynamicsMass(), c.m_mirror
    finally:
        s.free(collective=False)
    assert got.shape == want.shape and (got > 0).all()
    print(f"{c.name}: largest mass deviation {np.abs(got / want - 1).max():.3e}, most elements at a node {c.k.max()}")
    assert (np.abs(got - want) <= (c.k - 1) * EPS * want).all()
    n = len(c.mnode)
    assert abs(total - c.mnode.sum()) <= n * EPS * c.mnode.sum()


@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_stable_step_is_the_mirrors_gershgorin_step(case):
    """The same sums in the same order on non-hub rows; a square root and two divisions, each correctly rounded on both sides,
    leave an ulp or two.  Hub rows were assembled by atomics: their row sums are the device's own matrix, which the mirror reads."""
    c = case
    got = c.s.stableDt()
    print(f"{c.name}: stable dt {got:.6e}, mirror {c.dt:.6e}")
    assert abs(got - c.dt) <= 4 * EPS * c.dt
    if c.name in PLAIN:
        om = c.modes()[0]
        print(f"{c.name}: dt / (2 / omega_max) = {got * om[-1] / 2.0:.4f}")
        assert got <= 2.0 / om[-1]


# ---- trajectory -----------------------------------------------------------------------------------------------------------------
def _trajectory(c, n_steps=300, every=7):
    rng = np.random.default_rng(17)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt = 0.9 * c.dt
    curve = ([0.0, 150.5 * dt, 400.0 * dt], [0.0, 1.0, 0.25])
    out = []
    for A in (c.A, c.Arev):
        st = c.mirror(A, dt=dt, alpha=0.0, t0=0.0, u0=u0, v0=v0, curve=curve)
        out.append((st.run(n_steps, every, magnitudes=True), st.u.copy(), st.v.copy()))
    probes = np.array([0, c.N // 2, c.N - 1])
    s = c.device(0.0, u0, v0, curve, probes)
    hist = s.dynamicsRun(dt, n_steps, 0.0, every)
    t, u, v = s.dynamicsState()
    return dt, out, hist, t, u, v, probes


@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_300_steps_under_a_ramp_against_the_mirror(case):
    """u and v after 300 steps from a random state, and the rows of every 7th step.  Bound for u, v: 16 x (mirror - mirror with
    the rows' products added in reverse).  T, S and W are sums of N terms that the device adds in its own fixed order (four rows
    a thread, 64 lanes, four waves, the blocks) and numpy in another: on top of the trajectory's 16 x they get the bound of a sum
    in any order, N eps sum |terms|, with the magnitudes from the mirror."""
    c = case
    dt, (fwd, rev), hist, t, u, v, probes = _trajectory(c)
    assert hist.shape == (300 // 7, 4 + 6)
    assert t == 300 * dt and np.array_equal(hist[:, 0], fwd[0][:, 0])
    for name, got, a, b in (("u", u, fwd[1], rev[1]), ("v", v, fwd[2], rev[2])):
        bound, fig = 16 * rel(b, a), rel(got, a)
        print(f"{c.name}: {name} device vs mirror {fig:.3e}, bound 16 x {bound / 16:.3e}")
        assert fig <= bound, name
    for j, name in ((1, "T"), (2, "S"), (3, "W")):
        a, b, mag = fwd[0][:, j], rev[0][:, j], fwd[0][:, j + 3]
        scale = np.abs(a).max()
        bound = 16 * np.abs(b - a).max() / scale + c.N * EPS * mag.max() / scale
        fig = np.abs(hist[:, j] - a).max() / scale
        print(f"{c.name}: {name} device vs mirror {fig:.3e}, bound {bound:.3e} (16 x {np.abs(b - a).max() / scale:.3e} + the sum's)")
        assert fig <= bound, name


@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_a_single_mode_on_the_device(case):
    """(b) u0 = phi_k, v0 = 0, no load: u_n = phi_k cos(n theta), cos theta = 1 - (omega_k dt)^2 / 2."""
    c = case
    om, phi = c.modes()
    k, n_steps, dt = 3, 600, 0.5 * c.dt
    theta = np.arccos(1.0 - 0.5 * (om[k] * dt) ** 2)
    want = phi[:, k] * np.cos(n_steps * theta)
    st = DR.Stepper(c.A, np.zeros(c.N), c.m, dt, u0=phi[:, k])
    st.run(n_steps)
    mirror = np.abs(st.u - want).max() / np.abs(phi[:, k]).max()
    s = c.device(0.0, phi[:, k], None, ([0.0, 1.0], [0.0, 0.0]))
    s.dynamicsRun(dt, n_steps)
    got = np.abs(s.dynamicsState()[1] - want).max() / np.abs(phi[:, k]).max()
    print(f"{c.name}: modal error device {got:.3e}, mirror {mirror:.3e}")
    assert got <= 16 * mirror


@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_T_plus_S_is_constant_on_the_device(case):
    """(c) undamped, unloaded: the relative spread of T + S over 900 steps."""
    c = case
    rng = np.random.default_rng(5)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt, n_steps = 0.9 * c.dt, 900
    st = DR.Stepper(c.A, np.zeros(c.N), c.m, dt, u0=u0, v0=v0)
    h = st.run(n_steps, 1)
    e = h[:, 1] + h[:, 2]
    mirror = (e.max() - e.min()) / np.abs(e).max()
    s = c.device(0.0, u0, v0, ([0.0, 1.0], [0.0, 0.0]))
    hd = s.dynamicsRun(dt, n_steps, 0.0, 1)
    ed = hd[:, 1] + hd[:, 2]
    got = (ed.max() - ed.min()) / np.abs(ed).max()
    print(f"{c.name}: spread of T + S device {got:.3e}, mirror {mirror:.3e}; T + S = {ed[0]:.6e}")
    assert hd.shape == (n_steps, 4)
    assert got <= 16 * mirror


def _static_steps(c, x, dt, alpha, floor=1e-9, cap=60000):
    """steps (a multiple of 50) after which the mirror is within `floor` of the static solution, and its figure there"""
    st = c.mirror(dt=dt, alpha=alpha)
    while st.n < cap:
        st.run(50)
        err = rel(st.u, x)
        if err < floor:
            break
    return st.n, err


@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_critical_damping_reaches_the_static_solution_on_the_device(case):
    """(d) alpha = 2 omega_min, dt = 0.9 x the stable step, constant load: the step count is the mirror's first multiple of 50
    within 1e-9 of the sparse LU solution -- convergence still visible, so that the figure is the scheme's, not noise."""
    import scipy.sparse.linalg as spl
    c = case
    x = spl.splu(sp.csc_matrix(c.A)).solve(c.f)
    alpha, dt = 2.0 * c.modes()[0][0], 0.9 * c.dt
    n_steps, mirror = _static_steps(c, x, dt, alpha)
    s = c.device()
    s.dynamicsRun(dt, n_steps, alpha)
    got = rel(s.dynamicsState()[1], x)
    print(f"{c.name}: static limit after {n_steps} steps device {got:.3e}, mirror {mirror:.3e}")
    assert got <= 16 * mirror


# ---- continuation, history ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tet10", "cook", "hub_elast"], indirect=True)
def test_runs_continue_exactly(case):
    """run(100) = run(50); run(50) = run(1) x 100, bit for bit in u, v and every history row: the first goes through two replays
    of the captured graph and a remainder, the others through stream launches only -- buffer rotation, step counter and the
    parity of the partial sums line up."""
    c = case
    rng = np.random.default_rng(23)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt = 0.8 * c.dt
    curve = ([0.0, 40.0 * dt, 90.0 * dt], [0.2, 1.0, -0.5])
    probes = [1, c.N - 2]
    results = []
    for chunks in ([100], [50, 50], [1] * 100):
        s = c.device(0.5, u0, v0, curve, probes)
        hist = np.vstack([s.dynamicsRun(dt, n, 0.3, 1) for n in chunks])
        results.append((hist,) + s.dynamicsState())
    h0, t0, uu0, vv0 = results[0]
    assert h0.shape == (100, 8) and np.isfinite(h0).all()
    for h, t, u, v in results[1:]:
        assert t == t0 and np.array_equal(u, uu0) and np.array_equal(v, vv0)
        assert np.array_equal(h, h0)
    # a longer run -- five replays, sampled rows in the middle of a graph -- against fifty runs of five steps (stream launches,
    # every row written by the closing launch of its run)
    s = c.device(0.5, u0, v0, curve, probes)
    ha = s.dynamicsRun(dt, 250, 0.3, 5)
    ta, ua, va = s.dynamicsState()
    s = c.device(0.5, u0, v0, curve, probes)
    hb = np.vstack([s.dynamicsRun(dt, 5, 0.3, 5) for _ in range(50)])
    tb, ub, vb = s.dynamicsState()
    assert ha.shape == (50, 8) and np.array_equal(ha, hb)
    assert ta == tb and np.array_equal(ua, ub) and np.array_equal(va, vb)


@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_history_rows(case):
    """n_steps // sample_every rows; the probe columns of the last row are get_state's u and v where the run ends on a sampled
    step; W = f . u of that state within the rounding of a sum of N terms in any order; no rows with sample_every = 0."""
    c = case
    rng = np.random.default_rng(29)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt = 0.7 * c.dt
    probes = np.array([0, 7, c.N - 1])
    for n_steps, every in ((120, 8), (100, 7), (51, 51), (5, 9)):
        s = c.device(0.0, u0, v0, None, probes)
        h = s.dynamicsRun(dt, n_steps, 0.1, every)
        assert h.shape == (n_steps // every, 10)
        t, u, v = s.dynamicsState()
        if n_steps % every == 0:
            assert h[-1, 0] == t
            assert np.array_equal(h[-1, 4:7], u[probes]) and np.array_equal(h[-1, 7:10], v[probes])
            assert abs(h[-1, 3] - c.f @ u) <= c.N * EPS * (np.abs(c.f) @ np.abs(u))
            assert abs(h[-1, 1] - 0.5 * np.sum(c.m * v * v)) <= c.N * EPS * 0.5 * np.sum(c.m * v * v) * 2
    s = c.device(0.0, u0, v0)
    assert s.dynamicsRun(dt, 10).shape == (0, 4)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_static_limit_through_the_drivers(golden_dir):
    """triaelasticityexplicit on Cook's membrane, critically damped with the mirror's omega_min, reaches
    triaelasticityparallelimpl1(rtol=1e-10)'s solution; the step count is where the mirror has stopped improving against
    the sparse LU solution (rounding level)."""
    import scipy.sparse.linalg as spl
    mesh = H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
    ed = H.ELAST2D_ELEMDATA
    static = pf.triaelasticityparallelimpl1(mesh, rtol=1e-10)
    assert static.reason > 0
    rowptr, cols, vals = static.solver.getCSR()
    f = static.solver.getRHS()
    dm, conn, xyz, _ = D._setup(pf.ELAST_TRIA, mesh)
    p = SimpleNamespace(xyz_new=xyz, conn_new=conn, dm=dm, rowptr=rowptr, cols=cols, vals=vals, rhs=f)
    A = DR.csr(p)
    m, _, _ = DR.free_dof_mass(p, 10.0, ed[2])
    om, _ = DR.modes(A, m)
    dt, alpha = 0.9 * DR.gershgorin_dt(A, m), 2.0 * om[0]
    x = spl.splu(sp.csc_matrix(A)).solve(f)
    st = DR.Stepper(A, f, m, dt, alpha=alpha)
    best = np.inf
    while st.n < 200000:                     # until 2000 more steps no longer halve the error
        st.run(2000)
        err = rel(st.u, x)
        if err > 0.5 * best:
            break
        best = err
    n_steps, mirror = st.n, rel(st.u, x)
    r = pf.triaelasticityexplicit(mesh, dt=dt, n_steps=n_steps, elemData=ed, density=10.0, load_curve=None, alpha=alpha)
    assert r.history.shape == (0, 4) and r.t == n_steps * dt
    got = rel(r.soln_free, static.soln_free)
    print(f"cook driver: {n_steps} steps, explicit vs CG {got:.3e}, CG vs LU {rel(static.soln_free, x):.3e}, mirror vs LU {mirror:.3e}")
    assert got <= 16 * mirror
    with pytest.raises(ValueError):
        pf.triaelasticityexplicit(mesh, dt=1.5 * dt / 0.9, n_steps=1, elemData=ed)       # above the stable step: refused, not run


def test_tetra_driver_against_the_mirror():
    """tetraelasticityexplicit on the small beam, steel under its own weight switched on at t = 0: the PROGRAM's dt = 0.01 is
    refused (far above the stable step), 120 steps at 0.8 x the stable step follow the mirror within the trajectory's bound, and
    the probe of the last row is the returned state's entry."""
    mesh = H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
    ed = np.array([207.0e9, H._f32(0.3), 1.0, 0.0, -9.81 * 7800.0, 0.0])
    with pytest.raises(ValueError):
        pf.tetraelasticityexplicit(mesh, elemData=ed)
    r0 = pf.tetraelasticityexplicit(mesh, dt=1e-9, n_steps=0, elemData=ed)
    assert r0.t == 0.0 and not r0.soln_free.any() and r0.total_mass == pytest.approx(7800.0 * 6.0, rel=1e-6)
    dt = 0.8 * r0.stable_dt
    tip = int(np.nonzero((mesh.xyz[1] == 6.0) & (mesh.xyz[0] == 0.5) & (mesh.xyz[2] == 0.5))[0][0])
    r = pf.tetraelasticityexplicit(mesh, dt=dt, n_steps=120, elemData=ed, sample_every=40, probes=[(tip, 1)])
    rowptr, cols, vals = r.solver.getCSR()
    p = SimpleNamespace(rowptr=rowptr, cols=cols, vals=vals)
    f, m = r.solver.getRHS(), r.solver.dynamicsMass()
    fwd, rev = (DR.Stepper(DR.csr(p, reverse=q), f, m, dt) for q in (False, True))
    hf, hr = fwd.run(120, 40), rev.run(120, 40)
    fig, bound = rel(r.soln_free, fwd.u), 16 * rel(rev.u, fwd.u)
    print(f"tetra driver: u device vs mirror {fig:.3e}, bound 16 x {bound / 16:.3e}; tip u_y {r.history[-1, 4]:.4e}")
    assert fig <= bound and rel(r.velo_free, fwd.v) <= 16 * rel(rev.v, fwd.v)
    assert r.history.shape == (3, 6) and np.array_equal(r.history[:, 0], hf[:, 0]) and r.t == 120 * dt
    g = r.dm.NodeDofArrayNew[r.dm.node_map_get_new[tip], 1]
    assert r.history[-1, 4] == r.soln_free[g] and r.history[-1, 5] == r.velo_free[g] and r.history[-1, 4] < 0.0
    assert r.solnVTK[tip, 1] == r.soln_free[g]


# ---- states and errors -----------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(pf.PfemError) as ei:
        call()
    return ei.value.code


def test_state_errors(golden_dir):
    mesh = H.read_mesh(f"{golden_dir}/input/tet10")
    dm, conn, xyz, edof = D._setup(pf.POISSON_TET, mesh)
    N = dm.size_global
    s = pf.PetscSolver().initialise(N, N)
    assert _code(lambda: s.dynamicsSetup(ANISO, 1.0)) == L.ERR_STATE            # no mesh
    s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
    assert _code(lambda: s.dynamicsSetup(ANISO, 1.0)) == L.ERR_STATE            # no pattern
    s.buildPattern()
    assert _code(lambda: s.dynamicsSetup(ANISO, 1.0)) == L.ERR_STATE            # setup before assemble
    assert _code(lambda: s.dynamicsRun(1e-3, 1)) == L.ERR_STATE                 # run before setup
    for call in (s.stableDt, s.dynamicsMass, s.dynamicsState, s.setDynamicsState, s.setProbes, lambda: s.setLoadCurve([0.0], [1.0])):
        assert _code(call) == L.ERR_STATE
    s.assemble(ANISO, H.TIMEDATA)
    for bad in (0.0, -1.0, float("inf")):
        assert _code(lambda: s.dynamicsSetup(ANISO, bad)) == L.ERR_ARG
    with pytest.raises(ValueError):
        s.dynamicsSetup(ANISO, [1.0, 2.0])                                      # two densities without a material map
    s.dynamicsSetup(ANISO, 1.0)
    dt = 0.5 * s.stableDt()
    for args in ((0.0, 1), (-dt, 1), (dt, -1), (dt, 1, -0.1), (dt, 1, 0.0, -1)):
        assert _code(lambda: s.dynamicsRun(*args)) == L.ERR_ARG
    assert _code(lambda: s.setLoadCurve([0.0, 0.0], [1.0, 2.0])) == L.ERR_ARG   # times must ascend
    assert _code(lambda: s.setProbes([N])) == L.ERR_ARG and _code(lambda: s.setProbes([-1])) == L.ERR_ARG
    s.dynamicsRun(dt, 3)
    s.dynamicsRun(dt, 3)                                                        # the same dt continues
    assert s.dynamicsState()[0] == 6 * dt
    assert _code(lambda: s.dynamicsRun(0.5 * dt, 1)) == L.ERR_STATE             # a new dt without a new state
    s.setDynamicsState(1.0)
    s.dynamicsRun(0.5 * dt, 2)
    assert s.dynamicsState()[0] == 1.0 + 2 * (0.5 * dt)
    # the solve beside it is untouched: the same iteration count and solution before and after a run
    its0 = s.factoriseAndSolve()[0]
    x0 = s.getSolution()
    s.dynamicsRun(0.5 * dt, 60)
    assert s.factoriseAndSolve()[0] == its0 and np.array_equal(s.getSolution(), x0)
    s.buildPattern()                                                            # a new pattern drops the mass
    assert _code(lambda: s.dynamicsRun(dt, 1)) == L.ERR_STATE
    # more than one rank: refused before anything is launched
    s.assemble(ANISO, H.TIMEDATA)
    s.dynamicsSetup(ANISO, 1.0)
    cb = lambda *a: 0      # noqa: E731
    s.setCommHost(0, 2, cb, cb)
    for call in (lambda: s.dynamicsSetup(ANISO, 1.0), lambda: s.dynamicsRun(dt, 1), s.stableDt, s.dynamicsMass, s.dynamicsState):
        assert _code(call) == L.ERR_STATE
    s.free(collective=False)
