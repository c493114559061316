"""One material per element (pfem_mesh_set_materials) through assembly, solve and post-processing on the device, against the
numpy mirror of the oracle's serial assembly fed with the oracle's element matrices per material (tests/materials_reference.py),
the host's per-element routines, the numpy reference of the recovery (tests/post_reference.py) and a closed form.

Meshes: the smallest on which the paths differ, none with a multiple of 64 nodes (the last wave of the incidence slices is
ragged): tet10 (own records), the 14 x 12 x 10 box (lattice numbering: pattern records), the 3 x 12 x 3 beam (elastic tet
gather), tria20x20, Cook's membrane, and the two hub meshes of test_gpu_parity (restricted atomic pass over elem_mat)."""
import numpy as np
import pytest

import materials_reference as MR
import pfemfort_amd as pf
import post_reference as PR
from oracle import pfem_oracle as O
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_parity import K_RTOL, U_ATOL, _hub_mesh

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BOX = (14, 12, 10)
CASES = ["tet10-rand3", "tet10-n256", "box-rand3", "box-layers", "beam-rand3", "tria20-rand3", "cook-rand3", "hub-rand3",
         "hub_elast-rand3"]
PLAIN = ["tet10-rand3", "box-rand3", "beam-rand3", "tria20-rand3", "cook-rand3"]      # no hub: every row has one writer


def _mesh(name, golden_dir):
    if name == "tet10":
        return pf.POISSON_TET, H.read_mesh(f"{golden_dir}/input/tet10")
    if name == "box":
        return pf.POISSON_TET, H.gen_box_tets(-1, 1, BOX[0], -1, 1, BOX[1], -1, 1, BOX[2])
    if name == "beam":
        return pf.ELAST_TET, H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
    if name == "tria20":
        return pf.POISSON_TRIA, H.read_mesh(f"{golden_dir}/input/tria20x20")
    if name == "cook":
        return pf.ELAST_TRIA, H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
    if name == "hub":
        return pf.POISSON_TET, _hub_mesh(300, 1)
    return pf.ELAST_TET, _hub_mesh(100, 3)


def _table(kind, n_mat, seed):
    """n_mat rows of elemData: contrast at most 10 between rows; elasticity with its own nu, (thickness) and body force per row."""
    rng = np.random.default_rng(seed)
    if kind == pf.POISSON_TET:
        return rng.uniform(1.0, 10.0, (n_mat, 3))
    if kind == pf.POISSON_TRIA:
        return rng.uniform(1.0, 10.0, (n_mat, 2))
    E = rng.uniform(100.0, 1000.0, n_mat)
    nu = rng.uniform(0.15, 0.4, n_mat)
    if kind == pf.ELAST_TET:
        return np.column_stack([E, nu, np.ones(n_mat), rng.uniform(-0.2, 0.2, (n_mat, 3))])
    return np.column_stack([E, nu, rng.uniform(0.5, 1.0, n_mat), rng.uniform(-0.2, 0.2, (n_mat, 2))])


def _materials(kind, mesh, variant):
    if variant == "rand3":           # drawn per element: the visits of one lane and of neighbouring lanes differ
        return _table(kind, 3, 21), np.random.default_rng(22).integers(0, 3, mesh.nElem).astype(np.int32)
    if variant == "layers":          # two layers by centroid
        return _table(kind, 2, 23), (mesh.xyz[2][mesh.conn].mean(0) > 0.0).astype(np.int32)
    assert variant == "n256"
    ids = np.random.default_rng(24).integers(0, 256, mesh.nElem).astype(np.int32)
    ids[::97] = 255
    return _table(kind, 256, 25), ids


def _solver(kind, mesh, table=None, ids=None, n_mat=None, build=True):
    dm, conn, xyz, edof = D._setup(kind, mesh)
    s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    s.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    if ids is not None:
        s.setMaterials(ids, n_mat=len(table) if n_mat is None else n_mat, stride=table.shape[1])
    if build:
        s.buildPattern()
    return s, dm, conn, xyz


class Case:
    """One mesh with its material map on the device, and the mirror's system for it -- both made once."""

    def __init__(self, name, golden_dir):
        self.name = name
        mname, variant = name.split("-")
        self.kind, self.mesh = _mesh(mname, golden_dir)
        self.table, self.ids = _materials(self.kind, self.mesh, variant)
        self.ndof, self.npe = L.NDOF[self.kind], L.NPELEM[self.kind]
        self.s, self.dm, self.conn, self.xyz = _solver(self.kind, self.mesh, self.table, self.ids)
        self.nNode, self.nElem = self.xyz.shape[1], self.conn.shape[1]
        assert self.nNode % 64 != 0
        self.ref = MR.setup_problem(self.kind, self.mesh, self.table, self.ids)
        assert np.array_equal(self.ref.conn_new, self.conn)
        self.u = np.random.default_rng(11).standard_normal((self.nNode, self.ndof))
        self.rows = self.table[self.ids]                       # every element's own elemData


_CASES = {}


@pytest.fixture
def case(request, golden_dir, monkeypatch):
    for v in ("PFEM_DEBUG_INC_OWN_RECORDS", "PFEM_DEBUG_GATHER_SOA", "PFEM_INC_PATTERNS"):
        monkeypatch.delenv(v, raising=False)
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(name, golden_dir)
    return _CASES[name]


def _hub_rows(c, rowptr):
    return np.nonzero(np.diff(rowptr) > 255)[0]


# ---- 1. K and rhs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_gather_form_equals_the_mirror_bit_for_bit(case):
    """getCSR() and getRHS() against the mirror: every row the gather kernels write, bit for bit -- all rows of the five meshes
    without a hub, all but the hub's on the other two.  The rows of a hub node (more than 255 entries) are not the gather
    kernels': the per-element pass restricted to them (k_assemble_*<ElemPrmTab>, reading elem_mat[e]) sums them with f64 atomics
    in no fixed order, with or without a map, so they take the bound of the scatter form, as in test_gpu_parity's
    test_gather_assembly_long_rows.  Measured on an MI355X: hub-rand3 1 hub row, 93 of its entries off by at most 1.4e-14
    (8.5e-5 of that bound); hub_elast-rand3 3 hub rows, 363 entries off by at most 9.1e-13 (1.6e-4 of the bound)."""
    c = case
    info = c.s.assemblyInfo()
    assert info["gather"]
    if c.name.startswith("box"):
        # the lattice path or the case covers nothing: k_gather_poisson_tet4 (LDS rows of a Poisson tet mesh) on pattern records
        n_pat, longest = c.s.incidencePatterns()
        assert n_pat >= 1 and longest >= 1 and info["hub_nodes"] == 0 and info["block_threads"] > 0 and info["lds_bytes"] > 0
    if c.name.startswith("hub"):
        assert info["hub_nodes"] >= 1
    if c.name.endswith("n256"):
        assert c.s.materials()[1] == 256 and (c.ids == 255).any()
    c.s.assemble(c.table, H.TIMEDATA)
    rowptr, cols, vals = c.s.getCSR()
    rhs = c.s.getRHS()
    assert np.array_equal(rowptr, c.ref.rowptr) and np.array_equal(cols, c.ref.cols)
    hub = _hub_rows(c, rowptr)
    keep = np.ones(len(vals), bool)
    for r in hub:
        keep[rowptr[r]:rowptr[r + 1]] = False
    print(f"{c.name}: {len(hub)} hub rows; max |K - mirror| = {np.abs(vals - c.ref.vals).max():.3e} "
          f"(entries that differ: {(vals != c.ref.vals).sum()}), max |rhs - mirror| = {np.abs(rhs - c.ref.rhs).max():.3e} "
          f"(rows that differ: {(rhs != c.ref.rhs).sum()})")
    assert np.array_equal(vals[keep], c.ref.vals[keep])
    assert np.array_equal(np.delete(rhs, hub), np.delete(c.ref.rhs, hub))
    assert np.abs(vals - c.ref.vals).max() <= K_RTOL * np.abs(c.ref.vals).max()
    assert np.abs(rhs - c.ref.rhs).max() <= K_RTOL * np.abs(c.ref.rhs).max()
    assert (len(hub) > 0) == c.name.startswith("hub")
    c.s.assemble(c.table, H.TIMEDATA)                             # ... and reproducible
    assert np.array_equal(c.s.getCSR()[2][keep], vals[keep]) and np.array_equal(np.delete(c.s.getRHS(), hub), np.delete(rhs, hub))
    # the material really is in there: row 0 for every element is another matrix
    uni = MR.setup_problem(c.kind, c.mesh, c.table, np.zeros(c.nElem, np.int32))
    assert np.abs(uni.vals - c.ref.vals).max() > 1e-3 * np.abs(c.ref.vals).max()


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_scatter_form_within_the_parity_bound(case):
    """Atomic adds reorder the sums: the bound of test_gpu_parity's scatter-form test."""
    c = case
    c.s.setAssemblyMode("scatter")
    try:
        c.s.assemble(c.table, H.TIMEDATA)
        _, _, vals = c.s.getCSR()
        rhs = c.s.getRHS()
    finally:
        c.s.setAssemblyMode("gather")
    print(f"{c.name}: |K - mirror| / bound = {np.abs(vals - c.ref.vals).max() / (K_RTOL * np.abs(c.ref.vals).max()):.3e}")
    assert np.abs(vals - c.ref.vals).max() <= K_RTOL * np.abs(c.ref.vals).max()
    assert np.abs(rhs - c.ref.rhs).max() <= K_RTOL * max(np.abs(c.ref.rhs).max(), 1e-300)


# ---- 2. element matrices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_element_matrices_equal_the_oracle_per_material(case):
    c = case
    K, F = c.s.evalElems(c.table, H.TIMEDATA)
    assert np.array_equal(K, c.ref.K) and np.array_equal(F, c.ref.F)


# ---- 3. / 4. a map that changes nothing, and clearing -----------------------------------------------------------------------
def _system_and_history(s, ed):
    s.assemble(ed, H.TIMEDATA)
    vals, rhs = s.getCSR()[2], s.getRHS()
    s.setTolerances(rtol=1e-10, maxits=20000)
    its, reason, _ = s.factoriseAndSolve()
    assert reason > 0
    return vals, rhs, s.getHistory(), s.getSolution()


@pytest.mark.parametrize("name", [n.split("-")[0] for n in PLAIN])
def test_a_map_that_changes_nothing(name, golden_dir):
    """All ids 0, and random ids into three identical rows: K, rhs and the CG's residual history of the mesh without a map."""
    kind, mesh = _mesh(name, golden_dir)
    ed = _table(kind, 1, 31)[0]
    want = _system_and_history(_solver(kind, mesh)[0], ed)
    zeros = _solver(kind, mesh, ed[None, :], np.zeros(mesh.nElem, np.int32))[0]
    rnd = _solver(kind, mesh, np.tile(ed, (3, 1)), np.random.default_rng(5).integers(0, 3, mesh.nElem).astype(np.int32))[0]
    for what, s, table in (("ids 0", zeros, ed[None, :]), ("three identical rows", rnd, np.tile(ed, (3, 1)))):
        assert s.materials() is not None
        got = _system_and_history(s, table)
        for a, b, part in zip(got, want, ("K", "rhs", "history", "solution")):
            assert np.array_equal(a, b), (name, what, part)


@pytest.mark.parametrize("name", ["tet10", "box", "beam"])
def test_clearing_the_map_gives_the_uniform_bits(name, golden_dir):
    kind, mesh = _mesh(name, golden_dir)
    ed = _table(kind, 1, 31)[0]
    want = _system_and_history(_solver(kind, mesh)[0], ed)
    table, ids = _materials(kind, mesh, "rand3")
    for clear in (lambda s: s.setMaterials(None), lambda s: s.setMaterials(ids, n_mat=0, stride=table.shape[1])):
        s = _solver(kind, mesh, table, ids, build=False)[0]
        assert s.materials()[1] == 3 and np.array_equal(s.materials()[0], ids)
        clear(s)
        assert s.materials() is None
        s.buildPattern()
        got = _system_and_history(s, ed)
        for a, b, part in zip(got, want, ("K", "rhs", "history", "solution")):
            assert np.array_equal(a, b), (name, part)


# ---- 5. solves --------------------------------------------------------------------------------------------------------------
_DIRECT = {}


@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("case", ["tet10-rand3", "beam-rand3"], indirect=True)
def test_solves_agree_with_the_direct_solve_of_the_mirror(case, pc):
    c = case
    if c.name not in _DIRECT:
        _DIRECT[c.name] = MR.direct_solve(c.ref)
    ud = _DIRECT[c.name]
    c.s.assemble(c.table, H.TIMEDATA)
    c.s.setPreconditioner(pc)
    try:
        c.s.setTolerances(rtol=1e-10, maxits=20000)
        its, reason, _ = c.s.factoriseAndSolve()
        u = c.s.getSolution()
    finally:
        c.s.setPreconditioner("jacobi")
    bound = U_ATOL * np.maximum(1.0, np.abs(ud))
    print(f"{c.name}/{pc}: its = {its}, reason = {reason}, worst |u - direct| / bound = {(np.abs(u - ud) / bound).max():.3e}")
    assert reason > 0
    assert np.all(np.abs(u - ud) <= bound)


# ---- 6. the two-E bar ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
def test_two_material_bar_on_the_device(pc):
    """u against the closed form, sigma_xx = sigma in every element, the reactions on x = 0 sum to sigma x area.  The area the
    element routine integrates over is 1 + 3e-8: its Gauss weight is the reference's REAL(4) 1/6 (post_reference.GAUSS_WT_TET),
    which scales K_e, hence the reactions K_e u_e, and neither u nor the stresses (no body force) -- 2.4e-6 at sigma = 80, three
    times the bound, so the expected sum carries that factor."""
    mesh, table, ids, sigma, ux = MR.bar(H, delta=1.0)
    s, dm, conn, xyz = _solver(pf.ELAST_TET, mesh, table, ids)
    s.assemble(table, H.TIMEDATA)
    s.setPreconditioner(pc)
    s.setTolerances(rtol=1e-10, maxits=20000)
    its, reason, _ = s.factoriseAndSolve()
    assert reason > 0
    nda = dm.NodeDofArrayNew
    full = dm.solnApplied.reshape(nda.shape).copy()
    full[nda >= 0] = s.getSolution()[nda[nda >= 0]]
    exact = np.zeros_like(full)
    exact[:, 0] = ux(xyz[0])
    _, stress, _ = s.elementFields(table)
    R = s.nodalForces(table, H.TIMEDATA)
    left = xyz[0] == 0.0
    print(f"bar/{pc}: its = {its}, max |u - exact| = {np.abs(full - exact).max():.3e}, max |sigma_xx - sigma| = "
          f"{np.abs(stress[0] - sigma).max():.3e}, sum R_x(x=0) + sigma = {R[left, 0].sum() + sigma:.3e}")
    assert np.all(np.abs(full - exact) <= U_ATOL * np.maximum(1.0, np.abs(exact)))
    assert np.all(np.abs(stress[0] - sigma) <= U_ATOL * max(1.0, sigma))
    assert np.all(np.abs(stress[1:]) <= U_ATOL * max(1.0, sigma))
    area = 1.0 * (6.0 * PR.GAUSS_WT_TET)
    assert abs(abs(R[left, 0].sum()) - sigma * area) <= U_ATOL * max(1.0, sigma)
    assert R[left, 0].sum() < 0 < R[xyz[0] == 2.0, 0].sum()


# ---- 7. post-processing --------------------------------------------------------------------------------------------------------
def _host_fields(c, u):
    ng = L.NG[c.kind]
    grad = np.empty((ng, c.nElem)); flux = np.empty((ng, c.nElem)); sc = np.empty(c.nElem)
    for e in range(c.nElem):
        nd = c.conn[:, e]
        z = c.xyz[2, nd] if c.xyz.shape[0] == 3 else None
        grad[:, e], flux[:, e], sc[e], _ = H.ElementPost(c.kind, c.xyz[0, nd], c.xyz[1, nd], z, c.rows[e], u[nd].ravel())
    return grad, flux, sc


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_element_fields_equal_the_host_routine_with_the_elements_own_row(case):
    c = case
    got = c.s.elementFields(c.table, c.u)
    for name, a, b in zip(("grad", "flux", "scalar"), got, _host_fields(c, c.u)):
        assert a.shape == b.shape and np.array_equal(a, b), (name, np.abs(a - b).max())


@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_nodal_forces_equal_the_sums_over_the_element_matrices(case, mode):
    """R = sum_e K_e u_e - F_e per node dof within 64 eps sum_e (|K_e||u_e| + |F_e|); the gather form gives the same bits twice."""
    c = case
    K, F = c.ref.K, c.ref.F                                      # (test 2: what evalElems returns, bit for bit)
    ue = c.u[c.conn.T].reshape(c.nElem, -1)
    idx = (c.conn.T[:, :, None] * c.ndof + np.arange(c.ndof)).reshape(c.nElem, -1)
    Rref = np.zeros(c.nNode * c.ndof); B = np.zeros(c.nNode * c.ndof)
    np.add.at(Rref, idx, np.einsum("eij,ej->ei", K, ue) - F)
    np.add.at(B, idx, np.einsum("eij,ej->ei", np.abs(K), np.abs(ue)) + np.abs(F))
    Rref, B = Rref.reshape(c.nNode, c.ndof), B.reshape(c.nNode, c.ndof)
    c.s.setAssemblyMode(mode)
    try:
        R = c.s.nodalForces(c.table, H.TIMEDATA, c.u)
        R2 = c.s.nodalForces(c.table, H.TIMEDATA, c.u)
    finally:
        c.s.setAssemblyMode("gather")
    print(f"{c.name}/{mode}: worst |R - ref| / (64 eps B) = {(np.abs(R - Rref) / (64 * EPS * B)).max():.3e}")
    assert np.all(np.abs(R - Rref) <= 64 * EPS * B)
    if mode == "gather" and c.s.assemblyInfo()["hub_nodes"] == 0:
        assert np.array_equal(R, R2)
    else:
        assert np.all(np.abs(R2 - Rref) <= 64 * EPS * B)


def _thick(c):
    return c.rows[:, 2] if c.kind == pf.ELAST_TRIA else 1.0


@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_recovery_and_indicator_equal_the_reference(case, mode):
    """post_reference.recover / indicator fed with the per-element fields and weights.  Bounds: the recovery's (2 cnt + 8) eps B of
    test_gpu_post_recovery (two sums of cnt terms and a division on both sides).  The indicator is evaluated from the device's own
    recovered values, so d = nodal - f has the same bits on both sides and only the order of the sums differs: sum_a d^2 and
    (sum_a d)^2 <= npe sum_a d^2, all terms positive, at most 2 npe^2 + npe ng + ng + 4 <= 64 roundings -- 128 eps eta2 with a
    factor two to spare; the totals to 1e-10 as test_gpu_post_recovery has them."""
    c = case
    grad, flux, _ = c.s.elementFields(c.table, c.u)
    w = PR.element_weights(c.xyz, c.conn, _thick(c))
    c.s.setAssemblyMode(mode)
    try:
        out = {f: c.s.nodalRecovery(c.table, c.u, f) for f in ("flux", "grad")}
        again = c.s.nodalRecovery(c.table, c.u, "flux")
        eta2, tot, fn = c.s.errorIndicator(c.table, c.u)
    finally:
        c.s.setAssemblyMode("gather")
    for field, f in (("flux", flux), ("grad", grad)):
        nodal_ref, w_ref, B, cnt = PR.recover(c.conn, w, f, c.nNode)
        nodal, sc, wt = out[field]
        bound = (2 * cnt + 8)[:, None] * EPS * B
        print(f"{c.name}/{mode}/{field}: worst |nodal - ref| / bound = "
              f"{np.nanmax(np.where(bound > 0, np.abs(nodal - nodal_ref) / np.where(bound > 0, bound, 1.0), 0.0)):.3e}")
        assert np.all(np.abs(nodal - nodal_ref) <= bound)
        assert np.all(np.abs(wt - w_ref) <= (2 * cnt + 8) * EPS * w_ref)
        if field == "flux":
            want = H.PostScalar(c.kind, nodal)
            assert np.all(np.abs(sc - want) <= 4 * EPS * want)
    if mode == "gather" and c.s.assemblyInfo()["hub_nodes"] == 0:
        for a, b in zip(out["flux"], again):
            assert np.array_equal(a, b)
    want2, fn2 = PR.indicator(c.conn, w, flux, out["flux"][0])
    print(f"{c.name}/{mode}: worst |eta2 - ref| / (128 eps eta2) = {(np.abs(eta2 - want2) / (128 * EPS * want2)).max():.3e}")
    assert np.all(np.abs(eta2 - want2) <= 128 * EPS * want2)
    assert abs(tot - want2.sum()) <= 1e-10 * want2.sum() and abs(fn - fn2.sum()) <= 1e-10 * fn2.sum()


# ---- 8. steps on a standing pattern (lattice box) ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
def test_steps_on_a_standing_pattern(pc, golden_dir, monkeypatch):
    for v in ("PFEM_DEBUG_INC_OWN_RECORDS", "PFEM_DEBUG_GATHER_SOA", "PFEM_INC_PATTERNS"):
        monkeypatch.delenv(v, raising=False)
    kind, mesh = _mesh("box", golden_dir)
    table, ids = _materials(kind, mesh, "layers")
    other = _table(kind, 2, 41)

    def fresh(tab, mat=ids):
        s = _solver(kind, mesh, tab if mat is not None else None, mat)[0]
        s.setPreconditioner(pc)
        s.setTolerances(rtol=1e-10, maxits=20000)
        return s

    def step(s, tab):
        s.assemble(tab, H.TIMEDATA)
        its, reason, _ = s.factoriseAndSolve()
        assert reason > 0
        return s.getCSR()[2], s.getRHS(), s.getHistory(), s.getSolution()

    s = fresh(table)
    assert s.incidencePatterns()[0] >= 1
    steps = [step(s, table) for _ in range(3)]
    dict_two = s.spmvValueDictionary()
    for k in (1, 2):
        for a, b, part in zip(steps[k], steps[0], ("K", "rhs", "history", "solution")):
            assert np.array_equal(a, b), (k, part)
    ref = MR.setup_problem(kind, mesh, table, ids)
    assert np.array_equal(steps[2][0], ref.vals) and np.array_equal(steps[2][1], ref.rhs)
    # a coefficient update: the dictionary of the last step misses, the full path runs once -- the bits of a fresh solver.
    # With gamg that holds for K and rhs only: the hierarchy's symbolic phase belongs to the pattern and was decided with the
    # values of the pattern's first step (pfem_amg.inc: bricks are refused where the couplings inside them are weak), so the
    # standing solver preconditions the new matrix with the aggregates of the old one, with or without a material map -- on
    # this box WITHOUT a map, elemData (1, 5, 9) and then (7, 2, 3) leaves "bricks" where a fresh solver takes
    # "lattice-passes".  The same system, another history (25 against 20 iterations here), the same solution to the solves'
    # tolerance.
    changed = step(s, other)
    f = fresh(other)
    want = step(f, other)
    again = step(s, other)
    if pc == "gamg":
        print(f"box/gamg: aggregation standing {s.amgAggregation()}, fresh {f.amgAggregation()}; its {len(changed[2]) - 1} / {len(want[2]) - 1}")
    for got in (changed, again):
        for a, b, part in zip(got, want, ("K", "rhs", "history", "solution")):
            if pc == "jacobi" or part in ("K", "rhs"):
                assert np.array_equal(a, b), part
        assert np.all(np.abs(got[3] - want[3]) <= U_ATOL * np.maximum(1.0, np.abs(want[3])))
    for a, b, part in zip(again, changed, ("K", "rhs", "history", "solution")):
        assert np.array_equal(a, b), part
    # value codes: where the uniform mesh of this size streams them on its second step, the two-material one must too
    uni = fresh(table[0], None)
    step(uni, table[0]); step(uni, table[0])
    print(f"box/{pc}: value dictionary entries, uniform {uni.spmvValueDictionary()}, two layers {dict_two}")
    if uni.spmvValueDictionary() > 0:
        assert dict_two > 0


# ---- the Python drivers -----------------------------------------------------------------------------------------------------
def test_drivers_take_a_map_in_both_modes(tmp_path, golden_dir):
    """elem_mat= / elemData= of the driver functions: batched mode sets the map, compat mode picks the element's row on the host
    -- the bar's closed form from both, and the systems of the mirror; write_outputs(fields=True) evaluates with the table and
    writes the cell scalar `material`."""
    from test_post_recovery_host import parse_vtk_array
    mesh, table, ids, sigma, ux = MR.bar(H, delta=1.0)
    ref = MR.setup_problem(pf.ELAST_TET, mesh, table, ids)
    exact = np.zeros((mesh.nNode, 3))
    exact[:, 0] = ux(mesh.xyz[0])                                            # solnVTK is by OLD node id
    res = {}
    for mode in ("batched", "compat"):
        r = res[mode] = pf.tetraelasticityparallelimpl1(mesh, mode=mode, rtol=1e-10, elem_mat=ids, elemData=table)
        assert r.reason > 0 and np.array_equal(r.elem_mat, ids)
        assert np.all(np.abs(r.solnVTK - exact) <= U_ATOL * np.maximum(1.0, np.abs(exact))), mode
        vals, rhs = r.solver.getCSR()[2], r.solver.getRHS()
        if mode == "batched":
            assert np.array_equal(vals, ref.vals) and np.array_equal(rhs, ref.rhs)
        else:                                                                # MatSetValues adds in the host loop's order too
            assert np.abs(vals - ref.vals).max() <= K_RTOL * np.abs(ref.vals).max()
            assert np.abs(rhs - ref.rhs).max() <= K_RTOL * np.abs(ref.rhs).max()
    assert res["batched"].solver.materials()[1:] == (2, 6)
    res["batched"].write_outputs(tmp_path, fields=True)
    text = (tmp_path / "Elasticity-soln-fields.vtk").read_text()
    key, got = parse_vtk_array(text, "CELL_DATA", "material", mesh.nElem)
    assert key == "SCALARS" and np.array_equal(got[:, 0], ids)
    key, got = parse_vtk_array(text, "CELL_DATA", "stress", mesh.nElem)
    assert key == "TENSORS" and np.all(np.abs(got[:, 0] - sigma) <= 5e-9 * sigma + U_ATOL * sigma)
    # the other four drivers pass the keywords on: a Poisson tet and both triangles against the mirror's matrix
    for fn, name in ((pf.tetrapoissonparallelimpl1, "tet10"), (pf.triapoissonparallelimpl1, "tria20"), (pf.triaelasticityparallelimpl1, "cook")):
        kind, m = _mesh(name, golden_dir)
        tab, em = _materials(kind, m, "rand3")
        r = fn(m, rtol=1e-10, elem_mat=em, elemData=tab)
        want = MR.setup_problem(kind, m, tab, em)
        assert r.reason > 0 and np.array_equal(r.solver.getCSR()[2], want.vals), name
    kind, m = _mesh("tria20", golden_dir)
    with pytest.raises(pf.PfemError) as ei:                                  # the inline triangle has no material
        pf.triapoissonserialimpl1(m, elem_mat=np.zeros(m.nElem, np.int32), elemData=np.ones((1, 2)))
    assert ei.value.code == L.ERR_ARG
    with pytest.raises(ValueError):
        pf.tetrapoissonparallelimpl1(_mesh("tet10", golden_dir)[1], elem_mat=np.zeros(5, np.int32), elemData=np.ones((1, 3)))


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(pf.PfemError) as ei:
        call()
    return ei.value.code


def test_errors_and_states(golden_dir):
    kind, mesh = _mesh("tet10", golden_dir)
    table, ids = _materials(kind, mesh, "rand3")
    ne = mesh.nElem
    lib = L.lib()
    p = lambda a: a.ctypes.data      # noqa: E731
    # a handle without a mesh
    empty = pf.PetscSolver().initialise(10, 10)
    assert lib.pfem_mesh_set_materials(empty._h, ne, p(ids), 3, 3) == L.ERR_STATE
    assert lib.pfem_mesh_get_materials(empty._h, None, None, None) == L.ERR_STATE
    s = _solver(kind, mesh, build=False)[0]
    assert s.materials() is None
    bad = ids.copy(); bad[7] = 3
    neg = ids.copy(); neg[7] = -1
    wide = np.zeros(ne, np.int32); wide[3] = 256
    for args in ((ne - 1, p(ids), 3, 3), (ne + 1, p(ids), 3, 3), (ne, p(bad), 3, 3), (ne, p(neg), 3, 3), (ne, p(wide), 257, 3),
                 (ne, p(ids), 257, 3), (ne, p(ids), -1, 3), (ne, p(ids), 3, 2), (ne, p(ids), 3, 0)):
        assert lib.pfem_mesh_set_materials(s._h, *args) == L.ERR_ARG, args[0:1] + args[2:]
        assert s.materials() is None                                       # a refused map leaves none behind
    # the strides of the other kinds
    for k, name, need in ((pf.POISSON_TRIA, "tria20", 2), (pf.ELAST_TET, "beam", 6), (pf.ELAST_TRIA, "cook", 5)):
        km, mm = _mesh(name, golden_dir)
        t = _solver(km, mm, build=False)[0]
        z = np.zeros(mm.nElem, np.int32)
        assert lib.pfem_mesh_set_materials(t._h, mm.nElem, p(z), 1, need - 1) == L.ERR_ARG
        assert lib.pfem_mesh_set_materials(t._h, mm.nElem, p(z), 1, need) == L.OK
        assert lib.pfem_mesh_set_materials(t._h, mm.nElem, p(z), 1, need + 2) == L.OK
        assert t.materials()[2] == need + 2
    # the inline triangle has no material
    km, mm = pf.POISSON_TRIA_INLINE, _mesh("tria20", golden_dir)[1]
    t = _solver(km, mm, build=False)[0]
    assert lib.pfem_mesh_set_materials(t._h, mm.nElem, p(np.zeros(mm.nElem, np.int32)), 1, 2) == L.ERR_ARG
    # a legal map with a wider stride; a NULL table in the later calls; the map after the pattern
    wide_table = np.concatenate([table, np.full((3, 2), np.nan)], axis=1)
    s.setMaterials(ids, n_mat=3, stride=5)
    em, n_mat, stride = s.materials()
    assert (n_mat, stride) == (3, 5) and np.array_equal(em, ids)
    s.buildPattern()
    assert _code(lambda: s.setMaterials(ids, n_mat=3, stride=5)) == L.ERR_STATE
    assert _code(lambda: s.setMaterials(None)) == L.ERR_STATE
    u = np.zeros(s.nNode)
    for call in (lambda: s.assemble(None, H.TIMEDATA), lambda: s.evalElems(None, H.TIMEDATA), lambda: s.elementFields(None, u),
                 lambda: s.nodalForces(None, H.TIMEDATA, u), lambda: s.nodalRecovery(None, u), lambda: s.errorIndicator(None, u)):
        assert _code(call) == L.ERR_ARG
    with pytest.raises(ValueError):
        s.assemble(table, H.TIMEDATA)                                      # (3, 3) where the map wants (3, 5)
    s.assemble(wide_table, H.TIMEDATA)                                     # the columns past the kind's are never read
    ref = MR.setup_problem(kind, mesh, table, ids)
    assert np.array_equal(s.getCSR()[2], ref.vals) and np.array_equal(s.getRHS(), ref.rhs)
    # more than one rank: refused before anything is launched
    cb = lambda *a: 0      # noqa: E731
    s.setCommHost(0, 2, cb, cb)
    assert _code(lambda: s.assemble(wide_table, H.TIMEDATA)) == L.ERR_STATE
    s.free(collective=False)
    # a new mesh clears the map
    s2 = _solver(kind, mesh, table, ids, build=False)[0]
    assert s2.materials()[1] == 3
    dm, conn, xyz, edof = D._setup(kind, mesh)
    s2.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    assert s2.materials() is None
    s2.buildPattern()
    ed = _table(kind, 1, 31)[0]
    s2.assemble(ed, H.TIMEDATA)
    want = O.setup_problem(kind, O.Mesh(mesh.xyz, mesh.conn, mesh.bc_node, mesh.bc_dof, mesh.bc_val), elemData=ed)
    assert np.array_equal(s2.getCSR()[2], want.vals) and np.array_equal(s2.getRHS(), want.rhs)
    # ... and so does a generated one; on it the map is in the generator's element order
    nx, ny, nz = 5, 4, 3
    sz = H.box_slab_sizes(nx, ny, nz, 0, 1)
    g = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    g.generateBoxMesh(pf.POISSON_TET, -1, 1, nx, -1, 1, ny, -1, 1, nz)
    gm = H.gen_box_tets(-1, 1, nx, -1, 1, ny, -1, 1, nz)
    gids = np.random.default_rng(8).integers(0, 3, gm.nElem).astype(np.int32)
    g.setMaterials(gids, n_mat=3)
    assert g.materials()[2] == 3
    g.generateBoxMesh(pf.POISSON_TET, -1, 1, nx, -1, 1, ny, -1, 1, nz)
    assert g.materials() is None
    g.setMaterials(gids, n_mat=3)
    g.buildPattern()
    g.assemble(table, H.TIMEDATA)
    gref = MR.setup_problem(kind, gm, table, gids)
    assert np.array_equal(g.getCSR()[2], gref.vals) and np.array_equal(g.getRHS(), gref.rhs)
