"""Thermal strains on the device: the load (pfem_rhs_add_thermal_load) against the numpy mirror (tests/thermal_reference.py),
the post-processing under a thermal state against the host's per-element routine and closed forms, solves against the mirror's
direct solve, the handover of a temperature field from a Poisson handle, and the isolation of every existing path.

Meshes (all at or below 2 112 dofs): the 3 x 12 x 3 beam (208 nodes: one block of the node kernels), an elastic box of
5 x 7 x 6 cells (336 nodes: two blocks and a partial last slice; 1 260 tets), Cook's membrane (1 089 nodes, plane stress),
the elastic hub mesh (the hub / atomic pass), the beam with three materials drawn per element."""
import numpy as np
import pytest

import materials_reference as MR
import post_reference as PR
import surface_reference as SR
import thermal_reference as TR
import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_parity import K_RTOL, U_ATOL, _hub_mesh, _shuffled      # noqa: F401  (K_RTOL: the parity file's pair)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NAMES = ["beam", "box", "cook", "hub_elast", "beam-rand3"]
GATHER = ["beam", "box", "cook", "beam-rand3"]                         # no hub: every row has one writer
ALPHA = 1.2e-3
ALPHA3 = np.array([1.2e-3, 0.4e-3, 2.0e-3])
ED3 = np.array([240.0, 0.3, 1.0, 0.1, -0.05, 0.02])
ED2 = np.array([240.0, 0.3, 0.5, 0.05, -0.02])


def _beam(ndof=3, bc_mode=1):
    return H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=bc_mode, ndof=ndof)


def _mesh(name, golden_dir):
    if name in ("beam", "beam-rand3"):
        return pf.ELAST_TET, ED3, _beam()
    if name == "box":
        return pf.ELAST_TET, ED3, H.gen_box_tets(0.0, 1.0, 5, 0.0, 1.0, 7, 0.0, 1.0, 6, bc_mode=1, ndof=3)
    if name == "cook":
        return pf.ELAST_TRIA, ED2, H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
    return pf.ELAST_TET, ED3, _hub_mesh(100, 3)


def _theta(xyz):
    """A temperature that is no linear function of the coordinates."""
    x, y = xyz[0], xyz[1]
    z = xyz[2] if xyz.shape[0] == 3 else 0.0 * x
    return 20.0 + 15.0 * x - 8.0 * y + 5.0 * x * y + 3.0 * z * z


class Case:
    """One mesh on the device with its pattern, the mirror's system for it, a seeded nodal field -- all made once."""

    def __init__(self, name, golden_dir):
        self.name = name
        self.kind, ed, self.mesh = _mesh(name, golden_dir)
        self.ndof, self.npe = L.NDOF[self.kind], L.NPELEM[self.kind]
        self.ids = None
        self.ed, self.alpha = ed, np.array([ALPHA])
        if name.endswith("rand3"):
            rng = np.random.default_rng(21)
            self.ed = np.tile(ed, (3, 1))
            self.ed[:, 0] = rng.uniform(100.0, 1000.0, 3)
            self.ed[:, 1] = rng.uniform(0.15, 0.4, 3)
            self.ids = np.random.default_rng(22).integers(0, 3, self.mesh.nElem).astype(np.int32)
            self.alpha = ALPHA3
        self.dm, self.conn, self.xyz, self.edof = D._setup(self.kind, self.mesh)
        self.nNode, self.nElem, self.N = self.xyz.shape[1], self.conn.shape[1], self.dm.size_global
        assert self.nNode % 64 != 0
        self.s = self.fresh()
        table = np.atleast_2d(self.ed)
        self.ref = MR.setup_problem(self.kind, self.mesh, table, np.zeros(self.nElem, np.int32) if self.ids is None else self.ids)
        assert np.array_equal(self.ref.conn_new, self.conn)
        self.rows = TR.rows_of(self.ed, self.nElem, self.ids)
        self.alpha_e = TR.alpha_of(self.alpha, self.nElem, self.ids)
        self.theta = _theta(self.xyz)
        self.u = 1e-2 * np.random.default_rng(11).standard_normal((self.nNode, self.ndof))
        self.w = TR.dvol(self.kind, self.xyz, self.conn, self.rows)

    def fresh(self):
        s = pf.PetscSolver().initialise(self.N, self.N)
        s.uploadMesh(self.kind, self.conn, self.xyz, self.edof, self.dm.solnApplied)
        if self.ids is not None:
            s.setMaterials(self.ids, n_mat=3, stride=self.ed.shape[1])
        s.buildPattern()
        return s

    def eth(self, theta, alpha_e=None):
        return TR.thermal_strain(self.kind, self.alpha_e if alpha_e is None else alpha_e, theta, self.conn)

    def loads(self, theta, alpha_e=None):
        """(F_th (nElem, nsize), b (N,), babs (N,)) of the mirror."""
        F, _ = TR.element_loads(self.kind, self.xyz, self.conn, self.rows, self.eth(theta, alpha_e))
        b, babs = TR.load_vector(self.conn, self.edof, self.N, F)
        return F, b, babs

    def forces_bound(self, u, Fth):
        """sum_e (|K_e||u_e| + |F_e| + |F_th,e|) per node dof, K_e and F_e the oracle's."""
        ue = np.abs(u[self.conn.T].reshape(self.nElem, -1))
        per = np.einsum("eij,ej->ei", np.abs(self.ref.K), ue) + np.abs(self.ref.F) + np.abs(Fth)
        return TR.node_sums(self.conn, self.ndof, self.nNode, per)

    def body(self):
        """-sum_e F_e per node dof: what the nodal forces are when K u = F_th."""
        return -TR.node_sums(self.conn, self.ndof, self.nNode, self.ref.F)

    def zs(self, nd):
        return self.xyz[2, nd] if self.xyz.shape[0] == 3 else None


_CASES = {}


@pytest.fixture
def case(request, golden_dir):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(name, golden_dir)
    c = _CASES[name]
    c.s.setAssemblyMode("gather")
    c.s.clearThermal()
    return c


def _code(call):
    with pytest.raises(pf.PfemError) as ei:
        call()
    return ei.value.code


# ---- 1. the load -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_load_equals_the_mirror(case, mode):
    """getRHS() after assemble + addThermalLoad minus getRHS() after assemble alone against the mirror's load vector, within
    64 eps sum_e |F_th,e| per row (the assembly's own rhs stays below 16 sum_e |F_th,e| in every row, so the addition to it and
    the subtraction here give the added load back to within 9 eps of that sum); the gather form without hub nodes gives the same
    bits twice, the mirror's."""
    c = case
    _, b, babs = c.loads(c.theta)
    if c.name.startswith("hub"):
        assert c.s.assemblyInfo()["hub_nodes"] >= 1
    c.s.setAssemblyMode(mode)
    try:
        c.s.setThermal(c.alpha, c.theta)
        out = []
        for _ in range(2):
            c.s.assemble(c.ed, H.TIMEDATA)
            r0 = c.s.getRHS()
            c.s.addThermalLoad(c.ed)
            out.append((r0, c.s.getRHS()))
    finally:
        c.s.setAssemblyMode("gather")
    (r0, r1), (_, r2) = out
    assert np.all(np.abs(r0) <= 16 * babs)
    worst = (np.abs((r1 - r0) - b) / (64 * EPS * babs)).max()
    print(f"{c.name}/{mode}: worst |added - mirror| / (64 eps sum |F_th|) = {worst:.3e}, max |b| = {np.abs(b).max():.3e}")
    assert np.all(np.abs((r1 - r0) - b) <= 64 * EPS * babs)
    if mode == "gather" and c.s.assemblyInfo()["hub_nodes"] == 0:
        assert np.array_equal(r1, r2)
        assert np.array_equal(r1, r0 + b)                      # one writer per row, ascending element order: the mirror's bits
    else:
        assert np.all(np.abs((r2 - r0) - b) <= 64 * EPS * babs)


# ---- 2. element fields -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_element_fields_equal_the_host_routine_bit_for_bit(case):
    """One source for both sides: the fields under a state are pfem_elem_post_thermal's per element, with the element's own
    elemData and alpha row."""
    c = case
    c.s.setThermal(c.alpha, c.theta)
    got = c.s.elementFields(c.ed, c.u)
    ng = L.NG[c.kind]
    grad = np.empty((ng, c.nElem)); flux = np.empty((ng, c.nElem)); sc = np.empty(c.nElem)
    for e in range(c.nElem):
        nd = c.conn[:, e]
        grad[:, e], flux[:, e], sc[e], _ = H.ElementPostThermal(c.kind, c.xyz[0, nd], c.xyz[1, nd], c.zs(nd), c.rows[e], c.u[nd].ravel(),
                                                                c.alpha_e[e], c.theta[nd])
    for name, a, b in zip(("grad", "flux", "scalar"), got, (grad, flux, sc)):
        assert a.shape == b.shape and np.array_equal(a, b), (name, np.abs(a - b).max())
    c.s.clearThermal()
    plain = c.s.elementFields(c.ed, c.u)
    assert np.array_equal(plain[0], got[0]) and not np.array_equal(plain[1], got[1])     # grad is the total strain; the stress moved


# ---- 3. free expansion -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", GATHER, indirect=True)
def test_free_expansion_without_a_solve(case, mode):
    """u = alpha theta0 (x - x0) and a uniform theta0 (one alpha for all materials): no stress, within the bound of
    tests/test_thermal_reference.py; the nodal forces are the body-force term alone at EVERY node dof, within
    64 eps sum_e (|K_e||u_e| + |F_e| + |F_th,e|)."""
    c = case
    theta0 = 37.5
    x0 = c.xyz.mean(1, keepdims=True) + 0.3
    u = (ALPHA * theta0 * (c.xyz - x0)).T.copy()
    alpha = np.full(len(c.alpha), ALPHA)
    theta = np.full(c.nNode, theta0)
    c.s.setThermal(alpha, theta)
    c.s.setAssemblyMode(mode)
    try:
        _, flux, sc = c.s.elementFields(c.ed, u)
        R = c.s.nodalForces(c.ed, H.TIMEDATA, u)
    finally:
        c.s.setAssemblyMode("gather")
    g, _ = TR.geometry(c.kind, c.xyz, c.conn)
    gmax = np.sqrt(sum(np.square(np.stack(gd)) for gd in g)).max(0)
    umax = np.abs(u[c.conn]).max((0, 2))
    d11, d12, _ = TR.material(c.kind, c.rows)
    dinf = d11 + (2 if c.kind == pf.ELAST_TET else 1) * d12
    tol = dinf * 64 * EPS * umax * gmax + 64 * EPS * dinf * 2 * ALPHA * theta0
    print(f"{c.name}/{mode}: worst |stress| / bound = {(np.abs(flux) / tol).max():.3e}")
    assert np.all(np.abs(flux) <= tol) and np.all(sc <= 4 * tol)
    Fth, _, _ = c.loads(theta, np.full(c.nElem, ALPHA))
    B = c.forces_bound(u, Fth)
    print(f"{c.name}/{mode}: worst |R - body| / (64 eps B) = {(np.abs(R - c.body()) / (64 * EPS * B)).max():.3e}")
    assert np.all(np.abs(R - c.body()) <= 64 * EPS * B)


# ---- 4. full restraint -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GATHER, indirect=True)
def test_full_restraint(case):
    """u = 0: the stress is -sigma_th of the host's load routine, bit for bit, element by element (a non-uniform theta, the
    element's own rows); with a uniform theta the nodal forces at the interior nodes of a uniform material are the body-force
    term alone -- the thermal forces of the elements round a node cancel -- within 64 eps sum_e (|F_e| + |F_th,e|)."""
    c = case
    u = np.zeros((c.nNode, c.ndof))
    c.s.setThermal(c.alpha, c.theta)
    _, flux, _ = c.s.elementFields(c.ed, u)
    want = np.empty_like(flux)
    for e in range(c.nElem):
        nd = c.conn[:, e]
        want[:, e] = -H.ThermalLoad(c.kind, c.xyz[0, nd], c.xyz[1, nd], c.zs(nd), c.rows[e], c.alpha_e[e], c.theta[nd])[1]
    assert np.array_equal(flux, want)
    if c.ids is not None:
        return
    theta = np.full(c.nNode, 37.5)
    c.s.setThermal(c.alpha, theta)
    R = c.s.nodalForces(c.ed, H.TIMEDATA, u)
    be, bs = SR.boundary_sides(c.conn)
    interior = np.ones(c.nNode, bool)
    interior[SR.geometry(c.xyz, c.conn, be, bs)[2].ravel()] = False
    assert interior.sum() >= 30
    Fth, _, _ = c.loads(theta)
    B = c.forces_bound(u, Fth)
    print(f"{c.name}: {interior.sum()} interior nodes, worst |R - body| / (64 eps B) = "
          f"{(np.abs(R - c.body())[interior] / (64 * EPS * B[interior])).max():.3e}; max |R| on the boundary = {np.abs(R[~interior]).max():.3e}")
    assert np.all(np.abs(R - c.body())[interior] <= 64 * EPS * B[interior])
    assert np.abs(R[~interior]).max() > 10 * np.abs(c.body()).max()         # ... while the boundary carries the thermal forces


# ---- 5. solves -------------------------------------------------------------------------------------------------------------
def _linear_theta(xyz):
    """Linear in the coordinates, zero at the centre of the bounding box, within +-40."""
    lo, hi = xyz.min(1, keepdims=True), xyz.max(1, keepdims=True)
    xi = (xyz - 0.5 * (lo + hi)) / (hi - lo)
    return 100.0 * (np.array([0.4, -0.25, 0.15])[:xyz.shape[0]] @ xi)


@pytest.mark.parametrize("case", ["box", "cook"], indirect=True)
def test_solve_against_the_direct_solve_of_the_mirror(case):
    """The clamped body under a linear theta.  u against the mirror's system with the mirror's load, solved by sparse LU, within
    U_ATOL as test_gpu_materials compares.  Reactions: with the field of the direct solve (refined once, so that its residual at
    the free dofs is rounding) R vanishes at the free dofs and its sum over the clamped set is minus the applied body force --
    the thermal load is self-equilibrated and adds nothing -- within the nodal-forces bound summed over those node dofs.  The sum
    over ALL node dofs is minus the body force whatever u is, so what that bound has to hold is the rounding of R at the free
    dofs, which grows with |K_e||u_e| there: theta has zero mean over the body, which keeps the displacements those of bending and
    not of a net expansion (the mirror alone, on the host: 0.05 of the bound on the box, 0.1 on Cook's membrane)."""
    import scipy.sparse as sp
    c = case
    theta = _linear_theta(c.xyz)
    Fth, b, _ = c.loads(theta)
    p = c.ref
    A = sp.csr_matrix((p.vals, p.cols, p.rowptr), shape=(c.N, c.N))
    rhs = p.rhs + b
    sys_ = MR.Problem(p.kind, p.dm, p.xyz_new, p.conn_new, p.edof, p.rowptr, p.cols, p.vals, rhs, p.K, p.F)
    ud = MR.direct_solve(sys_)
    sys_.rhs = rhs - A @ ud
    ud = ud + MR.direct_solve(sys_)
    s = c.s
    s.setThermal(c.alpha, theta)
    s.assemble(c.ed, H.TIMEDATA)
    s.addThermalLoad(c.ed)
    s.setTolerances(rtol=1e-10, maxits=20000)
    its, reason, _ = s.factoriseAndSolve()
    u = s.getSolution()
    bound = U_ATOL * np.maximum(1.0, np.abs(ud))
    print(f"{c.name}: its = {its}, reason = {reason}, max |u| = {np.abs(ud).max():.3e}, worst |u - direct| / bound = {(np.abs(u - ud) / bound).max():.3e}")
    assert reason > 0 and np.all(np.abs(u - ud) <= bound)
    assert np.abs(ud).max() > 1e3 * U_ATOL                                    # (the thermal load does move the body)
    # u = None is the field the solution assembles to
    nda = c.dm.NodeDofArrayNew
    full = MR.full_field(p, u)
    assert np.array_equal(s.nodalForces(c.ed, H.TIMEDATA), s.nodalForces(c.ed, H.TIMEDATA, full))
    for a_, b_ in zip(s.elementFields(c.ed), s.elementFields(c.ed, full)):
        assert np.array_equal(a_, b_)
    # reactions of the direct solve's field
    fd = MR.full_field(p, ud)
    R = s.nodalForces(c.ed, H.TIMEDATA, fd)
    B = c.forces_bound(fd, Fth)
    free = nda >= 0
    print(f"{c.name}: worst |R| / (64 eps B) at the free dofs = {(np.abs(R)[free] / (64 * EPS * B[free])).max():.3e}")
    assert np.all(np.abs(R)[free] <= 64 * EPS * B[free])
    react = np.where(free, 0.0, R).sum(0)
    applied = p.F.reshape(c.nElem, c.npe, c.ndof).sum((0, 1))
    rb = 64 * EPS * np.where(free, 0.0, B).sum(0)
    print(f"{c.name}: reactions {react}, applied body force {applied}, |sum| / bound = {np.abs(react + applied) / rb}")
    assert np.all(np.abs(react + applied) <= rb)


# ---- 6. recovery and indicator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_recovery_and_indicator_under_a_state(case, mode):
    """post_reference.recover / indicator fed with the thermal element stresses, within the bounds of test_gpu_post_recovery:
    (2 cnt + 8) eps B for the recovered values, 128 eps eta2 per element (evaluated from the device's own recovered values),
    1e-10 for the totals."""
    c = case
    c.s.setThermal(c.alpha, c.theta)
    _, flux, _ = c.s.elementFields(c.ed, c.u)
    c.s.setAssemblyMode(mode)
    try:
        nodal, sc, wt = c.s.nodalRecovery(c.ed, c.u, "flux")
        again = c.s.nodalRecovery(c.ed, c.u, "flux")
        eta2, tot, fn = c.s.errorIndicator(c.ed, c.u)
    finally:
        c.s.setAssemblyMode("gather")
    nodal_ref, w_ref, B, cnt = PR.recover(c.conn, c.w, flux, c.nNode)
    bound = (2 * cnt + 8)[:, None] * EPS * B
    print(f"{c.name}/{mode}: worst |nodal - ref| / bound = {np.nanmax(np.abs(nodal - nodal_ref) / np.where(bound > 0, bound, np.inf)):.3e}")
    assert np.all(np.abs(nodal - nodal_ref) <= bound)
    assert np.all(np.abs(wt - w_ref) <= (2 * cnt + 8) * EPS * w_ref)
    want = H.PostScalar(c.kind, nodal)
    assert np.all(np.abs(sc - want) <= 4 * EPS * want)
    if mode == "gather" and c.s.assemblyInfo()["hub_nodes"] == 0:
        for a, b in zip((nodal, sc, wt), again):
            assert np.array_equal(a, b)
    want2, fn2 = PR.indicator(c.conn, c.w, flux, nodal)
    print(f"{c.name}/{mode}: worst |eta2 - ref| / (128 eps eta2) = {(np.abs(eta2 - want2) / (128 * EPS * want2)).max():.3e}")
    assert np.all(np.abs(eta2 - want2) <= 128 * EPS * want2)
    assert abs(tot - want2.sum()) <= 1e-10 * want2.sum() and abs(fn - fn2.sum()) <= 1e-10 * fn2.sum()
    c.s.clearThermal()
    assert not np.array_equal(c.s.nodalRecovery(c.ed, c.u, "flux")[0], nodal)          # (the state did change the stresses)


# ---- 7. handover from a Poisson handle -------------------------------------------------------------------------------------
def _poisson(mesh):
    dm, conn, xyz, edof = D._setup(pf.POISSON_TET, mesh)
    s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    s.setTolerances(rtol=1e-10, maxits=20000)
    assert s.factoriseAndSolve()[1] > 0
    nda = dm.NodeDofArrayNew
    T = dm.solnApplied.copy()
    T[nda[:, 0] >= 0] = s.getSolution()[nda[nda[:, 0] >= 0, 0]]
    return s, dm, T


def _elastic(mesh):
    dm, conn, xyz, edof = D._setup(pf.ELAST_TET, mesh)
    s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    s.uploadMesh(pf.ELAST_TET, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    return s, dm


def _handover(ps, T, es, T_ref):
    """(theta, rhs) through the device and through the host, on the same two handles"""
    out = []
    for route in ("device", "host"):
        if route == "device":
            es.setThermalFrom(ps, ALPHA, T_ref=T_ref)
        else:
            es.setThermal(ALPHA, T - T_ref)
        a, th = es.getThermal()
        assert np.array_equal(a, [ALPHA])
        es.assemble(ED3, H.TIMEDATA)
        es.addThermalLoad(ED3)
        out.append((th, es.getRHS()))
    return out


def test_handover_from_a_poisson_solve(monkeypatch):
    """The Poisson kind on the beam's lattice, solved on the device; setThermalFrom carries its field to the elastic handle
    without a visit to the host.  getThermal() and the resulting rhs are bit for bit those of the route through the host
    (getSolution + solnApplied, minus T_ref, into setThermal).  Once more with both meshes under one random node numbering and
    the elastic handle renumbered inside the library (PFEM_REORDER=1): compared in the caller's numbering."""
    T_ref = 0.5
    ps, pdm, T = _poisson(_beam(ndof=1, bc_mode=0))
    es, edm = _elastic(_beam())
    ident = np.arange(len(T))
    assert np.array_equal(pdm.node_map_get_old, ident) and np.array_equal(edm.node_map_get_old, ident)   # one numbering for both
    assert np.ptp(T) > 1.0
    (th_d, rhs_d), (th_h, rhs_h) = _handover(ps, T, es, T_ref)
    assert np.array_equal(th_h, T - T_ref)
    assert np.array_equal(th_d, th_h) and np.array_equal(rhs_d, rhs_h)
    assert np.abs(rhs_d).max() > 1e-3
    # under a random numbering, the elastic handle renumbered inside
    ps2, pdm2, T2 = _poisson(_shuffled(_beam(ndof=1, bc_mode=0), seed=7))
    monkeypatch.setenv("PFEM_REORDER", "1")
    es2, edm2 = _elastic(_shuffled(_beam(), seed=7))
    assert es2.reordered()
    assert np.array_equal(pdm2.node_map_get_old, ident) and np.array_equal(edm2.node_map_get_old, ident)
    (th_d2, rhs_d2), (th_h2, rhs_h2) = _handover(ps2, T2, es2, T_ref)
    assert np.array_equal(th_h2, T2 - T_ref)
    assert np.array_equal(th_d2, th_h2) and np.array_equal(rhs_d2, rhs_h2)
    perm = np.random.default_rng(7).permutation(len(T)).astype(np.int32)                 # old id -> new id, as _shuffled draws it
    assert np.abs(th_d2[perm] - th_d).max() <= 1e-8 * np.abs(th_d).max()                 # the same field, to the two solves' tolerance


# ---- 8. isolation ----------------------------------------------------------------------------------------------------------
def _everything(s, c):
    out = list(s.elementFields(c.ed, c.u)) + [s.nodalForces(c.ed, H.TIMEDATA, c.u)]
    out += [a for a in s.nodalRecovery(c.ed, c.u, "flux")] + [a for a in s.nodalRecovery(c.ed, c.u, "grad") if a is not None]
    eta2, tot, fn = s.errorIndicator(c.ed, c.u)
    out += [eta2, np.array([tot, fn])]
    s.assemble(c.ed, H.TIMEDATA)
    s.setTolerances(rtol=1e-10, maxits=20000)
    its, reason, rn = s.factoriseAndSolve()
    assert reason > 0
    return out + [np.array([its, reason]), np.array([rn]), s.getSolution(), s.getRHS()]


@pytest.mark.parametrize("case", ["beam", "cook", "beam-rand3"], indirect=True)
def test_a_cleared_state_leaves_nothing_behind(case):
    """Set, then clear: element fields, nodal forces, recovery, indicator and a solve give the bits of a handle that never had a
    state.  And a load added to one assembly is gone with the next: the solve of a re-assembled system has the iteration count
    and the bits it had before."""
    c = case
    never = _everything(c.fresh(), c)
    s = c.fresh()
    s.setThermal(c.alpha, c.theta)
    s.clearThermal()
    for a, b in zip(_everything(s, c), never):
        assert np.array_equal(a, b)
    s.setThermal(c.alpha, c.theta)
    s.assemble(c.ed, H.TIMEDATA)
    s.addThermalLoad(c.ed)
    its, reason, _ = s.factoriseAndSolve()
    assert reason > 0 and not np.array_equal(s.getSolution(), never[-2])
    s.assemble(c.ed, H.TIMEDATA)                                   # re-assembled: the rhs is the assembly's again
    its2, reason2, rn2 = s.factoriseAndSolve()
    assert np.array_equal([its2, reason2], never[-4]) and rn2 == never[-3][0]
    assert np.array_equal(s.getSolution(), never[-2]) and np.array_equal(s.getRHS(), never[-1])


def test_states_and_error_codes(golden_dir):
    kind, ed, mesh = _mesh("beam", golden_dir)
    dm, conn, xyz, edof = D._setup(kind, mesh)
    nN = xyz.shape[1]
    th = np.ones(nN)
    s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    s.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    assert _code(lambda: s.setThermal(ALPHA, th)) == L.ERR_STATE                 # before the pattern
    s.buildPattern()
    assert _code(lambda: s.addThermalLoad(ed)) == L.ERR_STATE                    # no state
    assert _code(lambda: s.getThermal()) == L.ERR_STATE
    assert _code(lambda: s.setThermal([ALPHA, ALPHA], th)) == L.ERR_ARG          # n_alpha without a map is 1
    s.setThermal(ALPHA, th)
    a, t = s.getThermal()
    assert np.array_equal(a, [ALPHA]) and np.array_equal(t, th)
    s.assemble(ed, H.TIMEDATA)
    s.addThermalLoad(ed)
    s.buildPattern()                                                             # a new pattern drops the state
    s.assemble(ed, H.TIMEDATA)
    assert _code(lambda: s.addThermalLoad(ed)) == L.ERR_STATE
    s.setThermal(ALPHA, th)
    s.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)                          # ... and so does a new mesh
    s.buildPattern()
    assert _code(lambda: s.getThermal()) == L.ERR_STATE
    # with a map, one alpha per material row
    m = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    m.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    m.setMaterials(np.arange(conn.shape[1]) % 3, n_mat=3, stride=6)
    m.buildPattern()
    assert _code(lambda: m.setThermal(ALPHA, th)) == L.ERR_ARG
    m.setThermal(ALPHA3, th)
    assert np.array_equal(m.getThermal()[0], ALPHA3)
    # a Poisson kind has no thermal strains; as a source it needs the same nodes and a solve
    pm = _beam(ndof=1, bc_mode=0)
    pdm, pconn, pxyz, pedof = D._setup(pf.POISSON_TET, pm)
    p = pf.PetscSolver().initialise(pdm.size_global, pdm.size_global)
    p.uploadMesh(pf.POISSON_TET, pconn, pxyz, pedof, pdm.solnApplied)
    p.buildPattern()
    assert _code(lambda: p.setThermal(ALPHA, th)) == L.ERR_ARG
    assert _code(lambda: p.addThermalLoad(H.POISSON_ELEMDATA)) == L.ERR_ARG
    assert _code(lambda: s.setThermalFrom(p, ALPHA)) == L.ERR_STATE              # no solve of its pattern
    p.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    assert _code(lambda: s.setThermalFrom(p, ALPHA)) == L.ERR_STATE
    assert p.factoriseAndSolve()[1] > 0
    s.setThermalFrom(p, ALPHA, T_ref=1.0)
    assert _code(lambda: s.setThermalFrom(p, [ALPHA, ALPHA])) == L.ERR_ARG
    assert _code(lambda: s.setThermalFrom(s, ALPHA)) == L.ERR_ARG                # an elastic handle is no temperature field
    assert _code(lambda: s.setThermalFrom(m, ALPHA)) == L.ERR_ARG
    other = H.gen_box_tets(-1, 1, 4, -1, 1, 4, -1, 1, 4)
    odm, oconn, oxyz, oedof = D._setup(pf.POISSON_TET, other)
    o = pf.PetscSolver().initialise(odm.size_global, odm.size_global)
    o.uploadMesh(pf.POISSON_TET, oconn, oxyz, oedof, odm.solnApplied)
    o.buildPattern()
    o.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    assert o.factoriseAndSolve()[1] > 0
    assert _code(lambda: s.setThermalFrom(o, ALPHA)) == L.ERR_ARG                # another nNode


def test_driver_takes_a_thermal_state(golden_dir):
    """thermal=(alpha, theta) of the elastic drivers: the solution of test 5's system, and the state stays on the handle."""
    kind, ed, mesh = _mesh("cook", golden_dir)
    theta = _linear_theta(mesh.xyz)
    plain = H.Mesh(mesh.xyz, mesh.conn, mesh.bc_node, mesh.bc_dof, mesh.bc_val)          # (without the ForceBC file)
    r = D.triaelasticityparallelimpl1(plain, rtol=1e-10, elemData=ed, thermal=(ALPHA, theta))
    assert r.reason > 0
    a, th = r.solver.getThermal()
    assert np.array_equal(a, [ALPHA]) and np.array_equal(th[r.dm.node_map_get_new], theta)
    c = Case("cook", golden_dir) if "cook" not in _CASES else _CASES["cook"]
    _, b, _ = c.loads(theta[c.dm.node_map_get_old])
    sys_ = MR.Problem(c.ref.kind, c.ref.dm, c.ref.xyz_new, c.ref.conn_new, c.ref.edof, c.ref.rowptr, c.ref.cols, c.ref.vals, c.ref.rhs + b,
                      c.ref.K, c.ref.F)
    ud = MR.direct_solve(sys_)
    assert np.all(np.abs(r.soln_free - ud) <= U_ATOL * np.maximum(1.0, np.abs(ud)))
    with pytest.raises(ValueError):
        D.triaelasticityparallelimpl1(plain, mode="compat", elemData=ed, thermal=(ALPHA, theta))
