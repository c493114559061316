"""Post-processing on the device: element fields (gradient / strain, flux / stress, von Mises), nodal forces and reactions,
true residual -- against the host's per-element routine, closed forms, and numpy sums over the element matrices that
pfem_eval_elems (code older than this feature) computes."""
import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_parity import _hub_mesh, _shuffled
from test_post_host import check_linear_field

pytestmark = pytest.mark.gpu

ANISO = np.array([1.3, 0.7, 2.1])
COOK_DATA = np.array([H.ELAST_ELEMDATA[0], H.ELAST_ELEMDATA[1], 0.5, 0.05, -0.02])     # E, nu, thick, body force
NAMES = ["tet10", "box", "beam", "tria20", "tria20inline", "cook", "hub", "hub_elast"]


def _mesh(name, golden_dir):
    if name == "tet10":
        return pf.POISSON_TET, ANISO, H.read_mesh(f"{golden_dir}/input/tet10")
    if name == "box":
        return pf.POISSON_TET, H.POISSON_ELEMDATA, H.gen_box_tets(-1, 1, 14, -1, 1, 12, -1, 1, 10)
    if name == "beam":
        return pf.ELAST_TET, H.ELAST_ELEMDATA, H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
    if name == "tria20":
        return pf.POISSON_TRIA, np.array([1.5, 0.5]), H.read_mesh(f"{golden_dir}/input/tria20x20")
    if name == "tria20inline":
        return pf.POISSON_TRIA_INLINE, None, H.read_mesh(f"{golden_dir}/input/tria20x20")
    if name == "cook":
        return pf.ELAST_TRIA, COOK_DATA, H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
    if name == "hub":
        return pf.POISSON_TET, ANISO, _hub_mesh(300, 1)
    return pf.ELAST_TET, H.ELAST_ELEMDATA, _hub_mesh(100, 3)


class Case:
    """One mesh on the device with its pattern, a seeded random nodal field, and the reference sums -- computed once."""

    name = ""

    def __init__(self, kind, ed, mesh, seed=11):
        self.kind, self.ed, self.mesh = kind, ed, mesh
        self.ndof, self.npe = L.NDOF[kind], L.NPELEM[kind]
        self.dm, self.conn, self.xyz, edof = D._setup(kind, mesh)
        self.s = pf.PetscSolver().initialise(self.dm.size_global, self.dm.size_global)
        self.s.uploadMesh(kind, self.conn, self.xyz, edof, self.dm.solnApplied)
        self.s.buildPattern()
        self.nNode, self.nElem = self.xyz.shape[1], self.conn.shape[1]
        self.u = np.random.default_rng(seed).standard_normal((self.nNode, self.ndof))
        self._ref = None

    def reference(self):
        """numpy's scatter-add of K_e u_e - F_e and of |K_e||u_e| + |F_e| per node dof; K_e, F_e from pfem_eval_elems."""
        if self._ref is None:
            K, F = self.s.evalElems(self.ed, H.TIMEDATA)
            ue = self.u[self.conn.T].reshape(self.nElem, -1)
            idx = (self.conn.T[:, :, None] * self.ndof + np.arange(self.ndof)).reshape(self.nElem, -1)
            R = np.zeros(self.nNode * self.ndof)
            B = np.zeros(self.nNode * self.ndof)
            np.add.at(R, idx, np.einsum("eij,ej->ei", K, ue) - F)
            np.add.at(B, idx, np.einsum("eij,ej->ei", np.abs(K), np.abs(ue)) + np.abs(F))
            self._ref = (R.reshape(self.nNode, self.ndof), B.reshape(self.nNode, self.ndof), F)
        return self._ref


_CASES = {}


@pytest.fixture
def case(request, golden_dir):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(*_mesh(name, golden_dir))
        _CASES[name].name = name
    return _CASES[name]


def _host_fields(c, u):
    ng = L.NG[c.kind]
    grad = np.empty((ng, c.nElem)); flux = np.empty((ng, c.nElem)); sc = np.empty(c.nElem)
    for e in range(c.nElem):
        nd = c.conn[:, e]
        z = c.xyz[2, nd] if c.xyz.shape[0] == 3 else None
        grad[:, e], flux[:, e], sc[e], _ = H.ElementPost(c.kind, c.xyz[0, nd], c.xyz[1, nd], z, c.ed, u[nd].ravel())
    return grad, flux, sc


@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_device_fields_equal_the_host_routine_bit_for_bit(case):
    """One source for both sides (pfem_elem.hpp, built without contraction): the same bits, as pfem_eval_elems against the
    host's _ke routines."""
    c = case
    got = c.s.elementFields(c.ed, c.u)
    want = _host_fields(c, c.u)
    for name, a, b in zip(("grad", "flux", "scalar"), got, want):
        assert a.shape == b.shape
        assert np.array_equal(a, b), (name, np.abs(a - b).max())
    # any output may be NULL
    sc = np.empty(c.nElem)
    ed = None if c.ed is None else np.ascontiguousarray(c.ed, dtype=np.float64)
    vp = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    u = np.ascontiguousarray(c.u)
    L.check(L.lib().pfem_post_elements(c.s._h, vp(ed), vp(u), None, None, vp(sc)), "pfem_post_elements")
    assert np.array_equal(sc, got[2])


@pytest.mark.parametrize("case", ["tet10", "beam", "tria20", "tria20inline", "cook"], indirect=True)
def test_linear_field_on_the_device(case):
    """u = a + G x: gradient / engineering strains, flux / stress and scalar against their closed forms, for all five kinds
    (tolerances: test_post_host.check_linear_field)."""
    c = case
    rng = np.random.default_rng(3)
    ndim = c.xyz.shape[0]
    G = np.zeros((3, ndim))
    G[:c.ndof] = rng.standard_normal((c.ndof, ndim))
    a0 = rng.standard_normal(3)
    u = (a0[:c.ndof, None] + G[:c.ndof] @ c.xyz).T
    grad, flux, sc = c.s.elementFields(c.ed, u)
    for e in range(c.nElem):
        check_linear_field(c.kind, c.ed, G, a0, c.xyz, c.conn[:, e], grad[:, e], flux[:, e], sc[e], e)


@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_nodal_forces_equal_the_sum_of_the_element_matrices(case, mode):
    """R = sum_e K_e u_e - F_e within 1e-12 of sum_e |K_e||u_e| + |F_e| per node dof, in both forms; the sum over all nodes is
    -sum F_e whatever u is (partition of unity: a lost or doubled incidence shows); the gather form gives the same bits twice."""
    c = case
    Rref, B, F = c.reference()
    if c.name.startswith("hub"):
        assert c.s.assemblyInfo()["hub_nodes"] >= 1              # the restricted atomic pass is on the gather form's path
    c.s.setAssemblyMode(mode)
    try:
        R = c.s.nodalForces(c.ed, H.TIMEDATA, c.u)
        R2 = c.s.nodalForces(c.ed, H.TIMEDATA, c.u)
    finally:
        c.s.setAssemblyMode("gather")
    assert R.shape == (c.nNode, c.ndof)
    worst = (np.abs(R - Rref) / (1e-12 * B)).max()
    print(f"worst |R - ref| / bound = {worst:.3e}")
    assert np.all(np.abs(R - Rref) <= 1e-12 * B)
    total = -F.reshape(c.nElem, c.npe, c.ndof).sum((0, 1))
    assert np.all(np.abs(R.sum(0) - total) <= 1e-12 * np.abs(R).sum())
    if mode == "gather" and c.s.assemblyInfo()["hub_nodes"] == 0:
        assert np.array_equal(R, R2)
    else:
        assert np.all(np.abs(R2 - Rref) <= 1e-12 * B)


def test_af_scales_the_poisson_matrices_only(golden_dir):
    """timeData(2) = af as in pfem_assemble: K_e of the Poisson kinds carries it, the loads do not."""
    kind, ed, mesh = _mesh("tet10", golden_dir)
    c = Case(kind, ed, mesh)
    td = np.array([0.0, 0.75, 0.0])
    K, F = c.s.evalElems(ed, td)
    ue = c.u[c.conn.T].reshape(c.nElem, -1)
    R = np.zeros(c.nNode); B = np.zeros(c.nNode)
    np.add.at(R, c.conn.T, np.einsum("eij,ej->ei", K, ue) - F)
    np.add.at(B, c.conn.T, np.einsum("eij,ej->ei", np.abs(K), np.abs(ue)) + np.abs(F))
    got = c.s.nodalForces(ed, td, c.u)[:, 0]
    assert np.all(np.abs(got - R) <= 1e-12 * B)


def test_generated_box_agrees_with_the_uploaded_one(golden_dir):
    """pfem_mesh_generate_box numbers its nodes like the host generator: the same u gives the same R and fields."""
    if "box" not in _CASES:
        _CASES["box"] = Case(*_mesh("box", golden_dir))
    c = _CASES["box"]
    Rref, B, _ = c.reference()
    sz = H.box_slab_sizes(14, 12, 10, 0, 1)
    g = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    g.generateBoxMesh(pf.POISSON_TET, -1, 1, 14, -1, 1, 12, -1, 1, 10)
    g.buildPattern()
    R = g.nodalForces(c.ed, H.TIMEDATA, c.u)
    assert np.all(np.abs(R - Rref) <= 1e-12 * B)
    assert np.all(np.abs(R - c.s.nodalForces(c.ed, H.TIMEDATA, c.u)) <= 1e-12 * B)
    for a, b in zip(g.elementFields(c.ed, c.u), c.s.elementFields(c.ed, c.u)):
        assert np.array_equal(a, b)


def test_internal_renumbering_does_not_show(golden_dir, monkeypatch):
    """tet10 under a random node permutation with the library's internal renumbering forced: R and the element fields come back
    in the caller's numbering -- unscrambled, those of the unpermuted mesh."""
    if "tet10" not in _CASES:
        _CASES["tet10"] = Case(*_mesh("tet10", golden_dir))
    c = _CASES["tet10"]
    Rref, B, _ = c.reference()
    perm = np.random.default_rng(7).permutation(c.mesh.nNode).astype(np.int32)         # old id -> new id, as _shuffled draws it
    monkeypatch.setenv("PFEM_REORDER", "1")
    p = Case(c.kind, c.ed, _shuffled(c.mesh, seed=7))
    assert np.array_equal(p.conn, perm[c.conn])
    u = np.empty_like(c.u)
    u[perm] = c.u
    for mode in ("gather", "scatter"):
        p.s.setAssemblyMode(mode)
        R = p.s.nodalForces(c.ed, H.TIMEDATA, u)
        assert np.all(np.abs(R[perm] - Rref) <= 1e-12 * B), mode
    p.s.setAssemblyMode("gather")
    for a, b in zip(p.s.elementFields(c.ed, u), c.s.elementFields(c.ed, c.u)):
        assert np.array_equal(a, b)
    # ... and with the field of a solve (u = None): the same reactions as the unpermuted mesh's solve, to the solves' tolerance
    out = []
    for q, pm in ((c, np.arange(c.nNode)), (p, perm)):
        q.s.assemble(c.ed, H.TIMEDATA)
        q.s.setTolerances(rtol=1e-12, maxits=20000)
        assert q.s.factoriseAndSolve()[1] > 0
        out.append(q.s.nodalForces(c.ed, H.TIMEDATA)[pm])
    assert np.abs(out[0] - out[1]).max() <= 1e-8 * np.abs(out[0]).max()


@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("name", ["beam", "tet10"])
def test_after_a_solve(name, pc, golden_dir):
    """u = None: the field of the last solve.  Free dofs: R minus the applied nodal forces is K x - b of the assembled system;
    constrained dofs: the reactions balance the loads; the true residual is numpy's."""
    kind, ed, mesh = _mesh(name, golden_dir)
    if name == "tet10":
        ed = H.POISSON_ELEMDATA
    c = Case(kind, ed, mesh)
    s, nda = c.s, c.dm.NodeDofArrayNew
    s.assemble(ed, H.TIMEDATA)
    N = c.dm.size_global
    P = np.zeros(N)
    if name == "beam":                     # a few nodal forces at free dofs of the far end
        ids = nda[-4:].ravel()[[0, 4, 8, 9]]
        assert np.all(ids >= 0)
        vals = np.array([0.3, -0.2, 0.1, 0.25])
        s.addNodalForces(ids, vals)
        np.add.at(P, ids, vals)
    s.setPreconditioner(pc)
    s.setTolerances(rtol=1e-12, maxits=20000)
    its, reason, _ = s.factoriseAndSolve()
    assert reason > 0
    x, b = s.getSolution(), s.getRHS()
    rowptr, cols, vals_k = s.getCSR()
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    Kx = np.zeros(N); Kabs = np.zeros(N)
    np.add.at(Kx, rows, vals_k * x[cols])
    np.add.at(Kabs, rows, np.abs(vals_k) * np.abs(x[cols]))
    res = Kx - b
    scale = Kabs + np.abs(b)
    R = s.nodalForces(ed, H.TIMEDATA)
    free = nda >= 0
    Rfree = np.empty(N)
    Rfree[nda[free]] = R[free]
    worst = (np.abs((Rfree - P) - res) / (1e-12 * scale)).max()
    print(f"{name}/{pc}: its {its}, worst free-dof deviation / bound = {worst:.3e}, |Kx-b|_1 = {np.abs(res).sum():.3e}")
    assert np.all(np.abs((Rfree - P) - res) <= 1e-12 * scale)
    # reactions: -(load of the elements + applied forces) per component; the elements' load is bforce_d x volume as the element
    # routine integrates it (pfem_eval_elems' F: the reference's REAL(4) Gauss weight makes the volume 6 (1 + 3e-8)), -6 x volume
    # for the Poisson source
    _, F = s.evalElems(ed, H.TIMEDATA)
    load = F.reshape(c.nElem, c.npe, c.ndof).sum((0, 1))
    Pd = np.zeros(c.ndof)
    for d in range(c.ndof):
        m = nda[:, d] >= 0
        Pd[d] = P[nda[m, d]].sum()
    react = np.where(free, 0.0, R).sum(0)
    if name == "beam":
        bf, vol = ed[3:6], 6.0
        assert np.all(np.abs(load - bf * vol) <= 1e-7 * np.abs(bf * vol) + 1e-300)
    assert np.all(np.abs(react + (load + Pd)) <= np.abs(res).sum() + 1e-12 * np.abs(R).sum())
    rn, bn = s.trueResidual()
    tol = 1e-12 * np.linalg.norm(scale)
    assert abs(rn - np.linalg.norm(res)) <= tol and abs(bn - np.linalg.norm(b)) <= tol
    # the element fields of the same solve: those of the nodal field the solution assembles to
    full = c.dm.solnApplied.reshape(-1, c.ndof).copy()
    full[free] = x[nda[free]]
    for a, bb in zip(s.elementFields(ed), s.elementFields(ed, full)):
        assert np.array_equal(a, bb)


def test_states(golden_dir):
    kind, ed, mesh = _mesh("tet10", golden_dir)
    c = Case(kind, ed, mesh)
    for call in (lambda: c.s.elementFields(ed), lambda: c.s.nodalForces(ed, H.TIMEDATA), lambda: c.s.trueResidual()):
        with pytest.raises(pf.PfemError) as ei:
            call()                                                        # u = None before any solve
        assert ei.value.code == L.ERR_STATE
    c.s.assemble(ed, H.TIMEDATA)
    with pytest.raises(pf.PfemError) as ei:
        c.s.elementFields(ed)                                             # ... assembled, still not solved
    assert ei.value.code == L.ERR_STATE
    # the MatSetValues path has no mesh on the device
    compat = pf.tetrapoissonparallelimpl1(mesh, rtol=1e-10, mode="compat").solver
    for call in (lambda: compat.elementFields(ed), lambda: compat.nodalForces(ed, H.TIMEDATA)):
        with pytest.raises(pf.PfemError) as ei:
            call()
        assert ei.value.code == L.ERR_STATE and "no mesh" in str(ei.value)
    rn, bn = compat.trueResidual()                                        # (the residual needs the matrix only)
    assert 0 <= rn <= 1e-6 * bn
    # an inverted element
    bad = H.Mesh(mesh.xyz, mesh.conn.copy(), mesh.bc_node, mesh.bc_dof, mesh.bc_val)
    bad.conn[[0, 1], 5] = bad.conn[[1, 0], 5]
    b = Case(kind, ed, bad)
    for mode in ("gather", "scatter"):
        b.s.setAssemblyMode(mode)
        for call in (lambda: b.s.elementFields(ed, b.u), lambda: b.s.nodalForces(ed, H.TIMEDATA, b.u)):
            with pytest.raises(pf.PfemError) as ei:
                call()
            assert ei.value.code == L.ERR_NEG_JAC
