"""The steppers, the modal analysis and the surface geometry on a mesh the library holds renumbered (maybe_reorder: Morton order
of the nodes and their dofs inside the library, the caller's numbering at every entry point).  The solve, SpMV, aggregates and
post-processing test that elsewhere (test_gpu_parity.py, test_gpu_post.py, test_gpu_post_recovery.py); here it is the
translations of the newer entry points: the state vectors and the mass of the explicit and implicit steppers, the probes and
through them the history rows, the start block, the hashed start through the device's permutation, the modes on their way
out, the block product, and the nodes of a side.

tet10_r, beam2_r and box19k_r are test_gpu_dynamics.py's meshes under a random node numbering, uploaded with PFEM_REORDER=1;
box19k_s is the 19 656-dof box under such a numbering with PFEM_REORDER unset, the renumbering left to the library.  Every test
asserts that the renumbering is in effect (pfem_solver_reordered).  The mirrors run on the shuffled case's own getCSR(), getRHS()
and dynamicsMass() -- the caller's numbering -- while K lies in the internal order on the device: a vector mapped wrongly on
its way in or out is wrong by its own size, not by a rounding.  The bounds are those of the files that test the same calls on
plain meshes."""
import numpy as np
import pytest

import implicit_reference as IR
import modal_reference as MO
from test_gpu_dynamics import get_case, rel
from test_gpu_implicit import RTOL, tolerances
from test_gpu_modal import check_block_product, check_lowest_modes, device_of, mirror_of

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FORCED = ["tet10_r", "beam2_r"]


def pair(name, golden_dir):
    """(the plain case, the shuffled one, the plain case's free dof -> the shuffled case's, new node -> new node)"""
    c0, c1 = get_case(name[:-2], golden_dir), get_case(name, golden_dir)
    assert c1.s.reordered() and not c0.s.reordered()
    perm = np.random.default_rng(7).permutation(c0.mesh.nNode)       # old id -> new id, as _shuffled draws it
    assert np.array_equal(c1.mesh.conn, perm[c0.mesh.conn])
    nodes = np.empty(c0.mesh.nNode, np.int64)
    nodes[c0.dm.node_map_get_new] = c1.dm.node_map_get_new[perm]
    g0, g1 = c0.dm.NodeDofArrayNew, c1.dm.NodeDofArrayNew[nodes]
    assert np.array_equal(g0 >= 0, g1 >= 0)
    dofs = np.empty(c0.N, np.int64)
    dofs[g0[g0 >= 0]] = g1[g0 >= 0]
    assert np.array_equal(np.sort(dofs), np.arange(c0.N)) and not np.array_equal(dofs, np.arange(c0.N))
    return c0, c1, dofs, nodes


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- mass and the stable step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORCED)
def test_mass_and_stable_step(name, golden_dir):
    """Elements are not renumbered, so every node sums the same terms in the same order: the plain case's mass bit for bit
    through the dof map.  A row of K holds the same values in another order: the row sums of the Gershgorin step move by
    (longest row) eps."""
    c0, c1, dofs, _ = pair(name, golden_dir)
    assert same_bits(c1.s.dynamicsMass()[dofs], c0.s.dynamicsMass())
    assert np.array_equal(c1.m_mirror, c1.m)                          # (the mirror's own mass, in the caller's numbering)
    longest = np.diff(c0.p.rowptr).max()
    a, b = c0.s.stableDt(), c1.s.stableDt()
    print(f"{name}: stable dt {b:.17e}, plain {a:.17e}, longest row {longest}")
    assert abs(b - a) <= longest * EPS * a


# ---- the explicit stepper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORCED)
def test_explicit_run_against_the_mirror(name, golden_dir):
    """100 steps at 0.9 x the stable step from a random state under a ramp, rows of every 10th step with probes on three dofs of
    the caller's numbering: u, v and T, S, W within test_gpu_dynamics.py's trajectory bounds (16 x mirror against the mirror with
    every row added in reverse; for the sums N eps sum |terms| more), the probe columns the mirror's u and v at those dofs
    within 16 x the two mirrors' largest difference at that step."""
    _, c, _, _ = pair(name, golden_dir)
    rng = np.random.default_rng(17)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt, n_steps, every = 0.9 * c.dt, 100, 10
    curve = ([0.0, 50.5 * dt, 140.0 * dt], [0.0, 1.0, 0.25])
    probes = np.array([1, c.N // 3, c.N - 2])
    runs = []
    for A in (c.A, c.Arev):
        st = c.mirror(A, dt=dt, alpha=0.0, t0=0.0, u0=u0, v0=v0, curve=curve)
        rows, us, vs = [], [], []
        for _ in range(n_steps // every):
            rows.append(st.run(every, every, magnitudes=True)[0])
            us.append(st.u.copy())
            vs.append(st.v.copy())
        runs.append((np.array(rows), np.array(us), np.array(vs)))
    (ra, ua, va), (rb, ub, vb) = runs
    s = c.device(0.0, u0, v0, curve, probes)
    hist = s.dynamicsRun(dt, n_steps, 0.0, every)
    t, u, v = s.dynamicsState()
    assert s.reordered() and hist.shape == (n_steps // every, 4 + 6)
    assert t == n_steps * dt and np.array_equal(hist[:, 0], ra[:, 0])
    for what, got, a, b in (("u", u, ua[-1], ub[-1]), ("v", v, va[-1], vb[-1])):
        fig, bound = rel(got, a), 16 * rel(b, a)
        print(f"{name}: {what} device vs mirror {fig:.3e}, bound 16 x {bound / 16:.3e}")
        assert fig <= bound, what
    for j, what in ((1, "T"), (2, "S"), (3, "W")):
        a, b, mag = ra[:, j], rb[:, j], ra[:, j + 3]
        scale = np.abs(a).max()
        bound = 16 * np.abs(b - a).max() / scale + c.N * EPS * mag.max() / scale
        fig = np.abs(hist[:, j] - a).max() / scale
        print(f"{name}: {what} device vs mirror {fig:.3e}, bound {bound:.3e}")
        assert fig <= bound, what
    for what, cols, a, b in (("u", hist[:, 4:7], ua, ub), ("v", hist[:, 7:10], va, vb)):
        bound = 16 * np.abs(b - a).max(1)                             # per sampled step, over the whole vector
        fig = np.abs(cols - a[:, probes]).max(1)
        print(f"{name}: probes of {what} vs mirror {fig.max():.3e}, bound at that step {bound[fig.argmax()]:.3e}, magnitude {np.abs(a[:, probes]).max():.3e}")
        assert (fig <= bound).all(), what
    assert np.array_equal(hist[-1, 4:7], u[probes]) and np.array_equal(hist[-1, 7:10], v[probes])


# ---- the implicit stepper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORCED)
def test_implicit_run_against_the_mirror(name, golden_dir):
    """20 damped Newmark steps at 20 x the stable step from the same state, rtol = 1e-13, rows of every 5th step: u, v, T, S, W
    and the probe columns, device against mirror-LU, within test_gpu_implicit.py's 16 x (mirror-PCG - mirror-LU)."""
    _, c, _, _ = pair(name, golden_dir)
    rng = np.random.default_rng(17)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt, n_steps, every = 20.0 * c.dt, 20, 5
    alpha = 0.1 / dt
    curve = ([0.0, 10.5 * dt, 30.0 * dt], [0.0, 1.0, 0.25])
    probes = np.array([1, c.N // 3, c.N - 2])
    runs = []
    for solve in ("lu", "pcg"):
        st = IR.ImplicitStepper(c.A, c.f, c.m, dt, solve=solve, rtol=RTOL, alpha=alpha, u0=u0, v0=v0, curve=curve)
        rows, us, vs = [], [], []
        for _ in range(n_steps // every):
            rows.append(st.run(every, every)[0])
            us.append(st.u.copy())
            vs.append(st.v.copy())
        runs.append((np.array(rows), np.array(us), np.array(vs), np.array(st.iterations)))
    (rl, ul, vl, _), (rp, up, vp, ip) = runs
    s = c.device(0.0, u0, v0, curve, probes)
    with tolerances(s, rtol=RTOL):
        hist, its = s.implicitRun(dt, n_steps, alpha=alpha, sample_every=every)
    t, u, v = s.dynamicsState()
    assert s.reordered() and hist.shape == (n_steps // every, 10) and its.shape == (n_steps,)
    assert t == n_steps * dt and np.array_equal(hist[:, 0], rl[:, 0])
    print(f"{name}: iterations device {its.min()}..{its.max()}, mirror {ip.min()}..{ip.max()}")
    for what, got, lu, pcg in (("u", u, ul[-1], up[-1]), ("v", v, vl[-1], vp[-1]), ("T", hist[:, 1], rl[:, 1], rp[:, 1]),
                               ("S", hist[:, 2], rl[:, 2], rp[:, 2]), ("W", hist[:, 3], rl[:, 3], rp[:, 3])):
        fig, bound = np.abs(got - lu).max(), 16 * np.abs(pcg - lu).max()
        print(f"{name}: {what} device vs mirror-LU {fig:.3e}, bound 16 x {bound / 16:.3e} (magnitude {np.abs(lu).max():.3e})")
        assert fig <= bound, what
    for what, cols, lu, pcg in (("u", hist[:, 4:7], ul, up), ("v", hist[:, 7:10], vl, vp)):
        bound = 16 * np.abs(pcg - lu).max(1)
        fig = np.abs(cols - lu[:, probes]).max(1)
        print(f"{name}: probes of {what} vs mirror-LU {fig.max():.3e}, bound at that step {bound[fig.argmax()]:.3e}, magnitude {np.abs(lu[:, probes]).max():.3e}")
        assert (fig <= bound).all(), what
    assert np.array_equal(hist[-1, 4:7], u[probes]) and np.array_equal(hist[-1, 7:10], v[probes])


# ---- the modal path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [4, 8, 16])
@pytest.mark.parametrize("name", FORCED)
def test_block_product_against_the_csr(name, mb, golden_dir):
    _, c, _, _ = pair(name, golden_dir)
    check_block_product(c, mb)


def hashed_start_is_the_uploaded_one(c, tol):
    """x0 = None (k_modal_init through the device's permutation) and x0 = the mirror's block (modal_upload_block through the
    host's) start from the same bits in the same rows: every bit of the two runs agrees"""
    a, cap = device_of(c, 2, tol), 4 * mirror_of(c, 2, tol).iterations
    b = c.s.modalSolve(2, tol=tol, max_iterations=cap, x0=MO.start_block(c.N, 4))
    assert c.s.reordered()
    assert b.iterations == a.iterations and b.restarts == a.restarts and b.reason == a.reason == 1
    assert np.array_equal(b.omega2, a.omega2) and np.array_equal(b.modes, a.modes) and np.array_equal(b.residuals, a.residuals)


@pytest.mark.parametrize("name", FORCED)
def test_hashed_start_equals_the_uploaded_block(name, golden_dir):
    _, c, _, _ = pair(name, golden_dir)
    hashed_start_is_the_uploaded_one(c, 1e-9 if name == "tet10_r" else 1e-6)


@pytest.mark.parametrize("name,n_modes,tol", [("tet10_r", 2, 1e-9), ("tet10_r", 6, 1e-9), ("beam2_r", 6, 1e-6)])
def test_lowest_modes_against_dense_eigh(name, n_modes, tol, golden_dir):
    _, c, _, _ = pair(name, golden_dir)
    check_lowest_modes(c, n_modes, tol)


# ---- boundary faces and their geometry ----------------------------------------------------------------------------------------------
def test_surface_geometry_in_the_callers_numbering(golden_dir):
    """the sides are named by element and local node, which no renumbering touches; their nodes come back in the caller's
    numbering -- the plain mesh's through the node map, face by face --, areas and normals with the same bits"""
    c0, c1, _, nodes = pair("tet10_r", golden_dir)
    (fe0, fs0), (fe1, fs1) = c0.s.boundaryFaces(), c1.s.boundaryFaces()
    assert fe0.size > 0 and np.array_equal(fe0, fe1) and np.array_equal(fs0, fs1)
    (a0, n0, nd0), (a1, n1, nd1) = c0.s.surfaceGeometry(fe0, fs0), c1.s.surfaceGeometry(fe1, fs1)
    assert np.array_equal(np.sort(nd1, axis=0), np.sort(nodes[nd0], axis=0))
    assert not np.array_equal(np.sort(nd1, axis=0), np.sort(nd0, axis=0))
    assert same_bits(a1, a0) and same_bits(n1, n0)


# ---- beyond one pass of the modal kernels' grids ---------------------------------------------------------------------------------------
def box19k_checks(name, golden_dir):
    """The two lowest modes meet the bounds of test_gpu_modal.py's run on the plain box -- the reference pairs are the plain
    case's, carried over by the dof map --, and the hashed start through a permutation over many blocks is the uploaded one."""
    c0, c, dofs, _ = pair(name, golden_dir)
    assert c.N == 19656 and same_bits(c.m[dofs], c0.m)
    om, phi = c0.modes()
    moved = np.empty_like(phi)
    moved[dofs] = phi
    c._modes = (om, moved)
    check_lowest_modes(c, 2, 1e-6)
    hashed_start_is_the_uploaded_one(c, 1e-6)


def test_forced_renumbering_beyond_one_grid_pass(golden_dir):
    """box19k under a random node numbering with PFEM_REORDER=1"""
    box19k_checks("box19k_r", golden_dir)


def test_automatic_renumbering_beyond_one_grid_pass(golden_dir):
    """box19k under a random node numbering, PFEM_REORDER unset: 4 096 owned dofs or more and a numbering without locality, so
    the library renumbers it of its own accord (pair() asserts pfem_solver_reordered).  2 048 places -- what maybe_reorder calls
    near -- are a tenth of these 19 656 dofs: only 25.1 % of the shuffled box's elements have no near pair of nodes, which is
    what a random numbering gives ((1 - 0.21)^6 = 0.25) and what the library's test holds the count against."""
    box19k_checks("box19k_s", golden_dir)
