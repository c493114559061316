"""Surface loads on the device: boundary sides (pfem_mesh_boundary_faces), their geometry (pfem_surface_geometry) and their
consistent nodal loads in the right-hand side (pfem_rhs_add_surface_load), against the numpy mirror
(tests/surface_reference.py), the host's per-side routine (host.FaceLoad), the reference's Cook's-membrane force file and
closed forms that the P1 space holds exactly.

Meshes as in test_gpu_materials: small, none with a multiple of 64 nodes: tet10, the 14 x 12 x 10 box, the 3 x 12 x 3 beam,
tria20x20, Cook's membrane, and the two hub meshes of test_gpu_parity."""
import math
import zlib

import numpy as np
import pytest

import materials_reference as MR
import post_reference as PR
import pfemfort_amd as pf
import surface_reference as SR
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_materials import _mesh
from test_gpu_parity import K_RTOL, U_ATOL

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MESHES = ["tet10", "box", "beam", "tria20", "cook", "hub", "hub_elast"]
N_BOUNDARY = {"tet10": 1200, "box": 1712, "beam": 324, "tria20": 80, "cook": 128}
ELEMDATA = {pf.POISSON_TET: H.POISSON_ELEMDATA, pf.POISSON_TRIA: np.array([1.0, 1.0]), pf.ELAST_TET: H.ELAST_ELEMDATA,
            pf.ELAST_TRIA: H.ELAST2D_ELEMDATA, pf.POISSON_TRIA_INLINE: None}


def _code(fn):
    with pytest.raises(pf.PfemError) as ei:
        fn()
    return ei.value.code


class Case:
    """One mesh on the device with its pattern, and what the mirror says about its boundary -- made once."""

    def __init__(self, kind, mesh, build=True, table=None, ids=None):
        self.kind, self.mesh = kind, mesh
        self.dm, self.conn, self.xyz, self.edof = D._setup(kind, mesh)
        self.N = self.dm.size_global
        self.s = pf.PetscSolver().initialise(self.N, self.N)
        self.s.uploadMesh(kind, self.conn, self.xyz, self.edof, self.dm.solnApplied)
        if ids is not None:
            self.s.setMaterials(ids, n_mat=len(table), stride=table.shape[1])
        if build:
            self.s.buildPattern()
        self.npe, self.ndof = L.NPELEM[kind], L.NDOF[kind]
        self.nElem, self.nNode = self.conn.shape[1], self.xyz.shape[1]
        self.be, self.bs = SR.boundary_sides(self.conn)


_CASES = {}


@pytest.fixture
def case(request, golden_dir):
    c = _rhs_case(request.param, golden_dir)
    assert c.nNode % 64 != 0
    c.name = request.param
    return c


# ---- 1. boundary sides ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MESHES, indirect=True)
def test_boundary_faces_equal_the_mirror(case, golden_dir):
    c = case
    fe, fs = c.s.boundaryFaces()                                          # after buildPattern
    assert fe.dtype == np.int32 and fs.dtype == np.int32
    assert np.array_equal(fe, c.be) and np.array_equal(fs, c.bs)
    if c.name in N_BOUNDARY:
        assert len(fe) == N_BOUNDARY[c.name]
    else:                                                                 # the sphere's triangles: the side opposite the hub
        assert np.array_equal(fe, np.arange(c.nElem)) and np.all(fs == 3)
    assert np.all(np.diff(fe.astype(np.int64) * 4 + fs) > 0)              # sorted by (element, side), no repeats
    again = c.s.boundaryFaces()                                           # the handle's copy
    assert np.array_equal(again[0], fe) and np.array_equal(again[1], fs)
    fresh = Case(c.kind, c.mesh, build=False)                             # before buildPattern, on a handle of its own ...
    f0 = fresh.s.boundaryFaces()
    assert np.array_equal(f0[0], fe) and np.array_equal(f0[1], fs)
    fresh.s.buildPattern()                                                # ... and the pattern build leaves it alone
    f1 = fresh.s.boundaryFaces()
    assert np.array_equal(f1[0], fe) and np.array_equal(f1[1], fs)
    # a new mesh drops the result: the same handle, the mesh without its first boundary element, the others in reverse order
    keep = np.delete(np.arange(c.nElem), fe[0])[::-1]
    rev = np.ascontiguousarray(fresh.conn[:, keep]); erev = np.ascontiguousarray(fresh.edof[:, keep])
    fresh.s.uploadMesh(c.kind, rev, fresh.xyz, erev, fresh.dm.solnApplied)
    want = SR.boundary_sides(rev)
    assert not (len(want[0]) == len(fe) and np.array_equal(want[0], fe) and np.array_equal(want[1], fs))
    f2 = fresh.s.boundaryFaces()
    assert np.array_equal(f2[0], want[0]) and np.array_equal(f2[1], want[1])


# ---- 2. geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MESHES, indirect=True)
def test_geometry_equals_the_host_bit_for_bit(case):
    """Measure and normal of every boundary side (and of as many interior ones) against host.FaceLoad: the same source compiled
    for both sides, IEEE sqrt and division -- bit for bit.  Against the mirror: the bounds derived in
    tests/test_surface_host.py, 8 eps mabs for the measure and 16 eps mabs / measure for a normal component.  Nodes: the
    mirror's, in the numbering the mesh was uploaded in.  A closed boundary: sum measure normal = 0 within eps sum measure
    (exact sums: math.fsum), and the box's area is 2 (2 * 2) * 3 = 24 within the measures' own 8 eps sum mabs."""
    c = case
    rng = np.random.default_rng(3)
    ie = rng.integers(0, c.nElem, len(c.be)).astype(np.int32); isd = rng.integers(0, c.npe, len(c.be)).astype(np.int32)
    for fe, fs in ((c.be, c.bs), (ie, isd)):
        meas, nrm, nodes = c.s.surfaceGeometry(fe, fs)
        mm, nm, ndm, mabs = SR.geometry(c.xyz, c.conn, fe, fs)
        assert np.array_equal(nodes, ndm)
        assert np.all(np.abs(meas - mm) <= 8 * EPS * mabs) and np.all(np.abs(nrm - nm) <= 16 * EPS * (mabs / mm)[None, :])
        hm = np.empty_like(meas); hn = np.empty_like(nrm)
        for i, (e, f) in enumerate(zip(fe, fs)):
            nd = c.conn[:, e]
            z = c.xyz[2, nd] if c.xyz.shape[0] == 3 else None
            _, hm[i], hn[:, i] = H.FaceLoad(c.kind, c.xyz[0, nd], c.xyz[1, nd], z, f)
        print(f"{c.name}: {len(fe)} sides, measures that differ from the host's: {(hm != meas).sum()}, normals: {(hn != nrm).sum()}; "
              f"from the mirror's: {(mm != meas).sum()}, {(nm != nrm).sum()}")
        assert np.array_equal(meas, hm) and np.array_equal(nrm, hn)
    meas, nrm, _ = c.s.surfaceGeometry(c.be, c.bs)
    total = math.fsum(meas)
    for d in range(nrm.shape[0]):
        closed = math.fsum(meas * nrm[d])
        print(f"{c.name}: sum measure n[{d}] = {closed:.3e}, eps sum measure = {EPS * total:.3e}")
        assert abs(closed) <= EPS * total
    if c.name == "box":
        mabs = SR.geometry(c.xyz, c.conn, c.be, c.bs)[3]
        assert abs(total - 24.0) <= 8 * EPS * math.fsum(mabs)
    # any output may be left out
    fe, fs = _i32(c.be[:5]), _i32(c.bs[:5])
    m5 = np.empty(5)
    L.check(L.lib().pfem_surface_geometry(c.s._h, 5, fe.ctypes.data, fs.ctypes.data, m5.ctypes.data, None, None), "pfem_surface_geometry")
    assert np.array_equal(m5, meas[:5])
    L.check(L.lib().pfem_surface_geometry(c.s._h, 5, fe.ctypes.data, fs.ctypes.data, None, None, None), "pfem_surface_geometry")


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- 3. the right-hand side ---------------------------------------------------------------------------------------------------
RHS_CASES = [("tet10", "flux", "uniform"), ("tet10", "flux", "face"), ("tet10", "flux", "face_node"),
             ("box", "flux", "face_node"), ("tria20", "flux", "uniform"), ("tria20", "flux", "face"), ("tria20", "flux", "face_node"),
             ("tria20_inline", "flux", "face_node"),
             ("beam", "traction", "uniform"), ("beam", "traction", "face"), ("beam", "traction", "face_node"),
             ("beam", "pressure", "uniform"), ("beam", "pressure", "face"), ("beam", "pressure", "face_node"),
             ("cook", "traction", "uniform"), ("cook", "traction", "face_node"), ("cook", "pressure", "face"), ("cook", "pressure", "face_node"),
             ("cook_2mat", "traction", "face"), ("cook_2mat", "pressure", "face_node"),
             ("hub", "flux", "face_node"), ("hub_elast", "pressure", "uniform"), ("hub_elast", "pressure", "face_node"),
             ("hub_elast", "traction", "face")]
LOAD_CODE = {"flux": L.LOAD_FLUX, "traction": L.LOAD_TRACTION, "pressure": L.LOAD_PRESSURE}
LAYOUT_CODE = {"uniform": SR.UNIFORM, "face": SR.PER_FACE, "face_node": SR.PER_FACE_NODE}


def _rhs_case(name, golden_dir):
    if name not in _CASES:
        if name == "tria20_inline":
            _CASES[name] = Case(pf.POISSON_TRIA_INLINE, H.read_mesh(f"{golden_dir}/input/tria20x20"))
        elif name == "cook_2mat":
            kind, mesh = _mesh("cook", golden_dir)
            table = np.array([[240.0, 0.3, 0.75, 0.0, 0.0], [120.0, 0.25, 1.5, 0.0, 0.0]])
            ids = (mesh.xyz[1][mesh.conn].mean(0) > 30.0).astype(np.int32)
            assert 0 < ids.sum() < mesh.nElem
            _CASES[name] = Case(kind, mesh, table=table, ids=ids)
            _CASES[name].table, _CASES[name].ids = table, ids
        else:
            kind, mesh = _mesh(name, golden_dir)
            if name == "hub_elast":                                        # no lifting: with zero body force the element loop leaves rhs = 0
                mesh.bc_val[:] = 0.0
            _CASES[name] = Case(kind, mesh)
    return _CASES[name]


@pytest.mark.parametrize("name,load,layout", RHS_CASES)
def test_rhs_gains_the_mirrors_load_vector(name, load, layout, golden_dir):
    """getRHS() after assemble and again after addSurfaceLoad: the difference is the mirror's load vector, per dof within
    8 eps sum |contributions to that dof|; dofs that no loaded side touches keep their bits; constrained dofs receive nothing
    (the mirror skips them, and the rhs has no entry for them).

    The sides: every boundary side, as many sides drawn from all (element, side) pairs -- interior ones, where the normal is
    the named element's; not on the hub meshes, which take their load on the sphere -- and the first three once more (a side
    given twice adds twice); on the meshes that are free on part
    of their boundary (beam, Cook, hubs) half of the boundary only, so that free surface dofs stay untouched.  The atomics add
    the contributions to what assemble left, one after the other: a running sum s picks up u |s| per addition, u = eps / 2.
    What the element loop left must not enter that rounding.  The elasticity cases run without body force and with zero
    Dirichlet values: assemble leaves rhs = 0 exactly.  The Poisson cases (the tet's source term, the lifting of u = x^2 + ...)
    scale the flux, which has one sign on a side, until the smallest side's load is 4096 times the largest entry assemble
    left.  Then k additions and the subtraction stay below (k + 1)(1 + 2^-11) u sum |contributions|, under
    8 eps sum |contributions| for up to 14 sides at a node."""
    c = _rhs_case(name, golden_dir)
    s, kind = c.s, c.kind
    rng = np.random.default_rng(zlib.crc32(f"{name}-{load}-{layout}".encode()))
    table = getattr(c, "table", None)
    ed = table if table is not None else ELEMDATA[kind]
    if kind in (pf.ELAST_TET, pf.ELAST_TRIA) and table is None:
        ed = ed.copy()
        ed[3:] = 0.0
    half = name.split("_")[0] in ("beam", "cook", "hub")
    nb = len(c.be) // 2 if half else len(c.be)
    pick = rng.permutation(len(c.be))[:nb]
    ni = 0 if name.startswith("hub") else nb          # (every interior side of a hub mesh holds the hub: hundreds of sides at one node)
    fe = np.concatenate([c.be[pick], rng.integers(0, c.nElem, ni), c.be[pick[:3]]]).astype(np.int32)
    fs = np.concatenate([c.bs[pick], rng.integers(0, c.npe, ni), c.bs[pick[:3]]]).astype(np.int32)
    n, ns = len(fe), c.npe - 1
    ncomp = SR.load_components(kind, LOAD_CODE[load])
    s.assemble(ed, H.TIMEDATA)
    r0 = s.getRHS()
    assert load == "flux" or np.all(r0 == 0.0)
    meas = SR.geometry(c.xyz, c.conn, fe, fs)[0]
    thick = 1.0 if kind != pf.ELAST_TRIA else (table[c.ids, 2] if table is not None else ed[2])
    tmin = np.min(thick)
    scale = 2.0 ** math.ceil(math.log2(4096.0 * max(np.abs(r0).max(), 1.0) * (12.0 if c.npe == 4 else 6.0) / (meas.min() * tmin)))
    shape = {"uniform": (ncomp,), "face": (n, ncomp), "face_node": (n, ns, ncomp)}[layout]
    sign = rng.choice([-1.0, 1.0], (n,) + (1,) * (len(shape) - 1)) if layout != "uniform" else rng.choice([-1.0, 1.0])
    values = scale * rng.uniform(1.0, 2.0, shape) * sign                   # one sign on a side: no cancellation inside a load
    s.addSurfaceLoad(fe, fs, load, values, layout=None if layout != "uniform" else "uniform", elemData=ed)
    r1 = s.getRHS()
    b, babs = SR.load_vector(kind, c.xyz, c.conn, c.edof, c.N, fe, fs, LOAD_CODE[load], values, LAYOUT_CODE[layout], thick)
    touched = babs > 0
    diff = r1 - r0
    worst = (np.abs(diff - b)[touched] / (8 * EPS * babs[touched])).max()
    print(f"{name} {load} {layout}: {n} sides, {touched.sum()} of {c.N} dofs loaded, scale 2^{int(math.log2(scale))}, "
          f"worst |diff - mirror| / bound = {worst:.3f}, dofs that differ from the mirror at all: {(diff != b).sum()}")
    assert touched.any() and not touched.all()
    assert np.array_equal(r1[~touched], r0[~touched])
    assert np.all(np.abs(diff - b) <= 8 * EPS * babs)
    # the case covers what it says: constrained dofs on loaded sides, and the smallest contribution dwarfs what assemble left
    loc = SR.side_local_nodes(c.npe)[fs]
    assert (c.edof[loc[:, 0] * c.ndof, fe] == -1).any()
    assert babs[touched].min() >= 1024 * np.abs(r0).max()
    # after a second assemble the loads are gone until they are added again (the rows of a hub node are summed with atomics by
    # the element loop itself, in no fixed order: those take the parity bound, as in test_gpu_materials)
    s.assemble(ed, H.TIMEDATA)
    r2 = s.getRHS()
    hub = np.nonzero(np.diff(s.getCSR()[0]) > 255)[0]
    assert (len(hub) > 0) == name.startswith("hub")
    assert np.array_equal(np.delete(r2, hub), np.delete(r0, hub))
    assert np.abs(r2 - r0).max() <= K_RTOL * max(np.abs(r0).max(), 1e-300)


# ---- 4. Cook's membrane -------------------------------------------------------------------------------------------------------
def test_cook_traction_is_the_force_file_and_the_drivers_solution(golden_dir):
    """The traction (0, 6.25) on the 32 edges with x = 48 leaves the rhs that addNodalForces leaves with the reference's ForceBC
    file, bit for bit (each node sums at most two equal terms: no order to matter), and
    triaelasticityparallelimpl1(surface_loads=...) on the mesh without its force file gives the driver's own solution."""
    c = _rhs_case("cook", golden_dir)
    mesh, s = c.mesh, c.s
    ed = H.ELAST2D_ELEMDATA
    fe, fs = s.boundaryFaces()
    nodes = s.surfaceGeometry(fe, fs)[2]
    on = np.all(c.xyz[0][nodes] == 48.0, axis=0)
    assert on.sum() == 32
    s.assemble(ed, H.TIMEDATA)
    s.addSurfaceLoad(fe[on], fs[on], "traction", [0.0, 6.25], elemData=ed)
    r_surface = s.getRHS()
    s.assemble(ed, H.TIMEDATA)
    gdof = c.dm.NodeDofArrayNew[c.dm.node_map_get_new[mesh.force_node], mesh.force_dof]
    s.addNodalForces(gdof, mesh.force_val)
    r_nodal = s.getRHS()
    assert np.abs(r_nodal).sum() > 0
    assert np.array_equal(r_surface, r_nodal)
    bare = H.Mesh(mesh.xyz, mesh.conn, mesh.bc_node, mesh.bc_dof, mesh.bc_val)
    own = pf.triaelasticityparallelimpl1(mesh, rtol=1e-10)
    got = pf.triaelasticityparallelimpl1(bare, rtol=1e-10, surface_loads=[
        {"elem": fe[on], "side": fs[on], "load": "traction", "values": [0.0, 6.25]}])
    assert own.reason > 0 and got.reason > 0
    print(f"cook: |u(surface load) - u(force file)| = {np.abs(got.soln_free - own.soln_free).max():.3e}, its {got.its} / {own.its}")
    assert np.abs(got.soln_free - own.soln_free).max() <= U_ATOL
    assert np.abs(own.soln_free).max() > 1.0                               # (a solution, not zeros)
    with pytest.raises(ValueError):
        pf.triaelasticityparallelimpl1(bare, mode="compat", surface_loads=[
            {"elem": fe[on], "side": fs[on], "load": "traction", "values": [0.0, 6.25]}])


# ---- 5. / 6. closed forms -----------------------------------------------------------------------------------------------------
E3, NU3, T3 = 10.0, 0.3, 1.0
# The volume the tet routine integrates over is 6 w V with w the reference's REAL(4) Gauss weight 1/6 (post_reference.GAUSS_WT_TET):
# 1 + 2.98e-8 times the volume.  K carries that factor, a surface load does not, so under a prescribed TRACTION the discrete
# problem's exact solution is the closed form divided by it, displacements and stresses alike (under a prescribed displacement,
# as in test_gpu_materials' bar, neither sees it) -- three times U_ATOL, so the expected values carry it.  Triangles: 0.5 jac, exact.
VOL3 = 6.0 * PR.GAUSS_WT_TET


def _roller_box():
    m = H.gen_box_tets(0.0, 1.0, 3, 0.0, 2.0, 4, 0.0, 1.0, 3, bc_mode=1, ndof=3)
    xyz = SR.jiggle_interior(m.xyz, 0.06, 5)
    assert (xyz != m.xyz).any()
    return H.Mesh(xyz, m.conn, *SR.rollers(xyz))


def _solve(c, ed, rtol=1e-12):
    c.s.setTolerances(rtol=rtol, maxits=20000)
    its, reason, _ = c.s.factoriseAndSolve()
    assert reason > 0
    nda = c.dm.NodeDofArrayNew
    full = c.dm.solnApplied.reshape(nda.shape).copy()
    u = c.s.getSolution()
    full[nda >= 0] = u[nda[nda >= 0]]
    return full, its


def test_uniaxial_tension_3d_and_its_reactions():
    """The elastic tet box 3 x 4 x 3 on [0,1] x [0,2] x [0,1], interior nodes off their sites, no body force, rollers on x = 0,
    y = 0, z = 0, traction (0, t, 0) on y = 2: u = (-nu t x / E, t y / E, -nu t z / E) and sigma_yy = t, the rest zero (both over VOL3,
    see above) -- exact in P1, so what is left is the solve (rtol 1e-12): U_ATOL for u, U_ATOL t for the stresses.

    Reactions: at the converged solution nodalForces() at the free dofs is the applied load, i.e. the mirror's load vector,
    within rtol |b|_2 (the residual the CG stopped at) + 8 eps sum |contributions| (item 3's bound).  The y-forces of ALL node
    dofs sum to minus the body force, zero here, whatever u is; the free ones carry b +- the residual, so the reactions on
    y = 0 sum to -t area within n_free rtol |b|_2 plus the rounding of the sums, 1e3 eps t."""
    c = Case(pf.ELAST_TET, _roller_box())
    ed = np.array([E3, NU3, 1.0, 0.0, 0.0, 0.0])
    fe, fs = c.s.boundaryFaces()
    meas, nrm, nodes = c.s.surfaceGeometry(fe, fs)
    top = nrm[1] == 1.0
    assert top.sum() == 18 and abs(meas[top].sum() - 1.0) < 1e-14 and np.all(c.xyz[1][nodes[:, top]] == 2.0)
    c.s.assemble(ed, H.TIMEDATA)
    assert np.all(c.s.getRHS() == 0.0)
    c.s.addSurfaceLoad(fe[top], fs[top], "traction", [0.0, T3, 0.0])
    u, its = _solve(c, ed)
    x, y, z = c.xyz
    want = np.stack([-NU3 * T3 * x / E3, T3 * y / E3, -NU3 * T3 * z / E3], axis=1) / VOL3
    _, stress, _ = c.s.elementFields(ed)
    sw = np.zeros(6); sw[1] = T3 / VOL3
    print(f"uniaxial 3-D: its {its}, |u - exact| = {np.abs(u - want).max():.3e}, |sigma - exact| = {np.abs(stress - sw[:, None]).max():.3e}")
    assert np.abs(u - want).max() <= U_ATOL
    assert np.abs(stress - sw[:, None]).max() <= U_ATOL * T3
    # 6. reactions
    R = c.s.nodalForces(ed, H.TIMEDATA)
    b, babs = SR.load_vector(c.kind, c.xyz, c.conn, c.edof, c.N, fe[top], fs[top], L.LOAD_TRACTION, [0.0, T3, 0.0], SR.UNIFORM)
    nda = c.dm.NodeDofArrayNew
    free = nda >= 0
    bn = np.linalg.norm(b)
    bound = 1e-12 * bn + 8 * EPS * babs[nda[free]]
    print(f"reactions: |R_free - b| = {np.abs(R[free] - b[nda[free]]).max():.3e}, rtol |b| = {1e-12 * bn:.3e}")
    assert np.all(np.abs(R[free] - b[nda[free]]) <= bound)
    on_y0 = (y == 0.0)
    assert not free[on_y0, 1].any()
    react = R[on_y0, 1].sum()
    assert abs(react - (-T3 * 1.0)) <= free[:, 1].sum() * 1e-12 * bn + 1e3 * EPS * T3, react


def test_hydrostatic_pressure_3d():
    """The same box with the pressure p on all six faces (what falls on roller dofs is dropped): sigma = -p I and
    u = -p (1 - 2 nu) x / E.  Every face orientation is in it."""
    p = 0.7
    c = Case(pf.ELAST_TET, _roller_box())
    ed = np.array([E3, NU3, 1.0, 0.0, 0.0, 0.0])
    fe, fs = c.s.boundaryFaces()
    nrm = c.s.surfaceGeometry(fe, fs)[1]
    assert {tuple(v) for v in np.round(nrm.T).astype(int)} == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}
    c.s.assemble(ed, H.TIMEDATA)
    c.s.addSurfaceLoad(fe, fs, "pressure", np.full((len(fe), 3), p))       # (nFace, npe-1): one value per side node
    u, its = _solve(c, ed)
    want = -p * (1.0 - 2.0 * NU3) / E3 * c.xyz.T / VOL3
    _, stress, _ = c.s.elementFields(ed)
    sw = np.array([-p, -p, -p, 0.0, 0.0, 0.0]) / VOL3
    print(f"hydrostatic: its {its}, |u - exact| = {np.abs(u - want).max():.3e}, |sigma - exact| = {np.abs(stress - sw[:, None]).max():.3e}")
    assert np.abs(u - want).max() <= U_ATOL
    assert np.abs(stress - sw[:, None]).max() <= U_ATOL * p


def test_uniaxial_tension_2d_plane_stress():
    """Triangles on [0,2] x [0,1] (tests/surface_reference.tria_strip), plane stress, thickness 0.5, rollers on x = 0 and y = 0,
    edge traction (t, 0) on x = 2: eps_xx = t / E, eps_yy = -nu t / E, no shear -- the reference's D(3,3) does not enter
    (checked on the CPU in tests/test_surface_host.py)."""
    E, nu, thick, t = 50.0, 0.3, 0.5, 2.0
    xyz, conn = SR.tria_strip(4, 3, 2.0, 1.0)
    c = Case(pf.ELAST_TRIA, H.Mesh(xyz, conn, *SR.rollers(xyz)))
    ed = np.array([E, nu, thick, 0.0, 0.0])
    fe, fs = c.s.boundaryFaces()
    meas, nrm, _ = c.s.surfaceGeometry(fe, fs)
    right = nrm[0] == 1.0
    assert right.sum() == 3 and abs(meas[right].sum() - 1.0) < 1e-14
    c.s.assemble(ed, H.TIMEDATA)
    c.s.addSurfaceLoad(fe[right], fs[right], "traction", [t, 0.0], elemData=ed)
    assert abs(c.s.getRHS().sum() - t * thick) < 1e-13
    u, its = _solve(c, ed)
    want = np.stack([t * c.xyz[0] / E, -nu * t * c.xyz[1] / E], axis=1)
    strain, stress, _ = c.s.elementFields(ed)
    print(f"uniaxial 2-D: its {its}, |u - exact| = {np.abs(u - want).max():.3e}, |sigma_xx - t| = {np.abs(stress[0] - t).max():.3e}")
    assert np.abs(u - want).max() <= U_ATOL
    assert np.abs(strain - np.array([t / E, -nu * t / E, 0.0])[:, None]).max() <= U_ATOL
    assert np.abs(stress - np.array([t, 0.0, 0.0])[:, None]).max() <= U_ATOL * t


# ---- 7. Poisson with a prescribed flux ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tet10", "tria20"])
def test_poisson_flux_against_a_direct_solve(name, golden_dir):
    """The Dirichlet data is taken off the nodes strictly inside the boundary face x = max x, and a flux that varies linearly
    along the face is prescribed there (PFEM_LOAD_FLUX, per side node).  Against scipy's sparse LU of the mirror's K and
    rhs + load vector (the oracle's serial assembly; the Poisson tet's built-in source of -6 stays): U_ATOL."""
    kind, mesh = _mesh(name, golden_dir)
    x = mesh.xyz
    hi, lo = x.max(1), x.min(1)
    face = x[0] == hi[0]
    inner = face & np.all((x[1:] > lo[1:, None]) & (x[1:] < hi[1:, None]), axis=0)
    assert inner.sum() >= 5
    keep = ~inner[mesh.bc_node]
    assert keep.sum() < len(keep)
    open_mesh = H.Mesh(mesh.xyz, mesh.conn, mesh.bc_node[keep], mesh.bc_dof[keep], mesh.bc_val[keep])
    c = Case(kind, open_mesh)
    assert c.nNode % 64 != 0
    ed = ELEMDATA[kind]
    fe, fs = c.s.boundaryFaces()
    _, nrm, nodes = c.s.surfaceGeometry(fe, fs)
    on = nrm[0] == 1.0
    assert on.sum() >= 10 and np.all(c.xyz[0][nodes[:, on]] == hi[0])
    g = (3.0 + 2.0 * c.xyz[1][nodes[:, on]]).T                             # (nFace, npe-1): linear in y
    c.s.assemble(ed, H.TIMEDATA)
    c.s.addSurfaceLoad(fe[on], fs[on], "flux", g)
    u, its = _solve(c, ed)
    ref = MR.setup_problem(kind, open_mesh, np.atleast_2d(ed), np.zeros(c.nElem, np.int32))
    assert np.array_equal(ref.conn_new, c.conn)
    b, _ = SR.load_vector(kind, c.xyz, c.conn, c.edof, c.N, fe[on], fs[on], L.LOAD_FLUX, g, SR.PER_FACE_NODE)
    assert np.count_nonzero(b) >= inner.sum()
    plain = MR.direct_solve(ref)
    ref.rhs = ref.rhs + b
    want = MR.direct_solve(ref)
    got = c.s.getSolution()
    print(f"{name}: its {its}, |u - direct| = {np.abs(got - want).max():.3e}, the flux moved u by {np.abs(want - plain).max():.3e}")
    assert np.abs(got - want).max() <= U_ATOL
    assert np.abs(want - plain).max() > 1e-2


# ---- 8. errors and state --------------------------------------------------------------------------------------------------------
def test_errors_and_state(golden_dir):
    kind, mesh = _mesh("tet10", golden_dir)
    c = Case(kind, mesh, build=False)
    s = c.s
    fe, fs = s.boundaryFaces()
    one = np.array([1.0])
    # no pattern: the load is refused, the sides and their geometry are not
    assert _code(lambda: s.addSurfaceLoad(fe, fs, "flux", one)) == L.ERR_STATE
    assert len(s.surfaceGeometry(fe, fs)[0]) == len(fe)
    s.buildPattern()
    s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    r0 = s.getRHS()
    e0, s0 = fe[:4].copy(), fs[:4].copy()
    for bad_e, bad_s in (([c.nElem], [0]), ([-1], [0]), ([0], [4]), ([0], [-1])):
        be = np.concatenate([e0, bad_e]).astype(np.int32); bs = np.concatenate([s0, bad_s]).astype(np.int32)
        assert _code(lambda: s.addSurfaceLoad(be, bs, "flux", one)) == L.ERR_ARG
        assert _code(lambda: s.surfaceGeometry(be, bs)) == L.ERR_ARG
    for load in ("traction", "pressure", 0, 4):
        assert _code(lambda: s.addSurfaceLoad(e0, s0, load, one, layout="uniform")) == L.ERR_ARG
    for layout in (-1, 3):
        assert _code(lambda: s.addSurfaceLoad(e0, s0, "flux", one, layout=layout)) == L.ERR_ARG
    assert L.lib().pfem_rhs_add_surface_load(s._h, 4, e0.ctypes.data, s0.ctypes.data, L.LOAD_FLUX, 0, None, None) == L.ERR_ARG
    assert L.lib().pfem_rhs_add_surface_load(s._h, 4, None, s0.ctypes.data, L.LOAD_FLUX, 0, one.ctypes.data, None) == L.ERR_ARG
    assert L.lib().pfem_mesh_boundary_faces(s._h, None, None, None) == L.ERR_ARG
    with pytest.raises(ValueError):
        s.addSurfaceLoad(e0, s0, "flux", np.ones((3, 2)))                  # a shape that fits no layout
    assert np.array_equal(s.getRHS(), r0)                                  # none of the refused calls added anything
    # elasticity: a flux is refused, and the plane-stress triangle wants its thickness
    ck = _rhs_case("cook", golden_dir)
    assert _code(lambda: ck.s.addSurfaceLoad(ck.be[:2], ck.bs[:2], "flux", one, layout="uniform")) == L.ERR_ARG
    assert _code(lambda: ck.s.addSurfaceLoad(ck.be[:2], ck.bs[:2], "pressure", one, layout="uniform", elemData=None)) == L.ERR_ARG
    # the MatSetValues path has no mesh on the device
    compat = pf.tetrapoissonparallelimpl1(H.gen_box_tets(-1, 1, 3, -1, 1, 3, -1, 1, 3), rtol=1e-6, mode="compat").solver
    assert _code(compat.boundaryFaces) == L.ERR_STATE
    assert _code(lambda: compat.surfaceGeometry(e0, s0)) == L.ERR_STATE
    assert _code(lambda: compat.addSurfaceLoad(e0, s0, "flux", one)) == L.ERR_STATE
    # a side of zero measure reports like a negative Jacobian (and so does every side of an element without volume)
    xyz = mesh.xyz.copy()
    n0, n1 = mesh.conn[0, 7], mesh.conn[1, 7]
    xyz[:, n1] = xyz[:, n0]
    d = Case(kind, H.Mesh(xyz, mesh.conn, mesh.bc_node, mesh.bc_dof, mesh.bc_val))
    de, ds = np.array([7, 7], np.int32), np.array([3, 0], np.int32)         # side 3 holds both nodes: no area
    assert _code(lambda: d.s.surfaceGeometry(de, ds)) == L.ERR_NEG_JAC
    assert _code(lambda: d.s.addSurfaceLoad(de, ds, "flux", one, layout="uniform")) == L.ERR_NEG_JAC
    # more than one rank: refused before anything is launched
    cb = lambda *a: 0      # noqa: E731
    s.setCommHost(0, 2, cb, cb)
    assert _code(s.boundaryFaces) == L.ERR_STATE
    assert _code(lambda: s.surfaceGeometry(e0, s0)) == L.ERR_STATE
    assert _code(lambda: s.addSurfaceLoad(e0, s0, "flux", one)) == L.ERR_STATE
    s.free(collective=False)
