"""Modal analysis on the device (pfem_modal_solve): the block product against getCSR() @ X, the lowest
eigenpairs against the dense eigh of the device's own K and m, reproducibility, gamg's cycle as the preconditioner, isolation
from the solve and the steppers, the state errors, and the lowest mode as the start of an implicit run.

Bounds.  The block product: row length x eps x sum_j |K_ij x_j| per entry -- a sum of that many terms in any order, with
fma.  The eigenpairs: 16 x the figure the numpy mirror (tests/modal_reference.py, checked against eigh in
tests/test_modal_reference.py) reaches at the same settings on the same K and m, with a floor of 1e-12 where the mirror's own
figure is the rounding of the dense reference.  The factor covers what the device does differently: the order of its sums
(fma, slices, blocks) and Jacobi sweeps where the mirror calls eigh, which also move the stopping iteration by one or two.
max_iterations is 4 x the mirror's count: it only catches a stall.

box19k (19 656 dofs; its reference is the lowest 13 pairs by eigsh, Case.modes) is the one mesh beyond one pass of the capped
grids of k_modal_gram (8 192 rows), and at MB 16 of k_modal_update and k_modal_residual (16 384 rows): the solve there takes
the later trips of their loops, which tests/test_gpu_modal_kernels.py checks a launch at a time."""
import numpy as np
import pytest

import implicit_reference as IR
import modal_reference as MO
import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_dynamics import ANISO, NAMES, PLAIN, case      # noqa: F401  (case: the fixture that builds a Case once)
from test_gpu_implicit import RTOL, tolerances

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FLOOR = 1e-12
# fixture -> (n_modes, tol) of the eigenpair checks
SETTINGS = [("tet10", 2, 1e-9), ("tet10", 6, 1e-9), ("tet10", 12, 1e-9), ("cook", 6, 1e-6), ("beam2", 6, 1e-6), ("hub", 2, 1e-6),
            ("hub_elast", 2, 1e-6), ("box19k", 12, 1e-6), ("box19k", 2, 1e-6)]

_MIRROR, _DEVICE = {}, {}


def mirror_of(c, n_modes, tol):
    """the mirror's run on the device's K and m with its figures against dense eigh, made once"""
    key = (c.name, n_modes, tol)
    if key not in _MIRROR:
        om, phi = c.modes()
        r = MO.lobpcg(c.A, c.m, n_modes, tol, 20000)
        assert r.reason == 1
        r.eig = MO.eig_error(r.omega2, om ** 2)
        r.dist = MO.subspace_distance(r.modes, phi[:, :n_modes], c.m)
        r.orth = MO.orthonormality(r.modes, c.m)
        _MIRROR[key] = r
    return _MIRROR[key]


def device_of(c, n_modes, tol):
    key = (c.name, n_modes, tol)
    if key not in _DEVICE:
        c.s.setPreconditioner("jacobi")
        _DEVICE[key] = c.s.modalSolve(n_modes, tol=tol, max_iterations=4 * mirror_of(c, n_modes, tol).iterations)
    return _DEVICE[key]


# ---- the block product -------------------------------------------------------------------------------------------------------------
def check_block_product(c, mb):
    rng = np.random.default_rng(40 + mb)
    X = rng.standard_normal((c.N, mb))
    got = c.s.modalSpmm(X)
    want = c.A @ X
    rowlen = np.diff(c.p.rowptr)
    bound = (rowlen * EPS)[:, None] * (abs(c.A) @ np.abs(X))
    worst = (np.abs(got - want) / bound).max()
    print(f"{c.name}: MB {mb}, longest row {rowlen.max()}, largest error / bound {worst:.3f}")
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all()
    # the hashed start block is the mirror's, bit for bit, and its product obeys the same bound
    X0 = MO.start_block(c.N, mb)
    Y0 = c.s.modalSpmm(X0)
    assert (np.abs(Y0 - c.A @ X0) <= (rowlen * EPS)[:, None] * (abs(c.A) @ np.abs(X0))).all()


@pytest.mark.parametrize("mb", [4, 8, 16])
@pytest.mark.parametrize("case", NAMES + ["box19k"], indirect=True)
def test_block_product_against_the_csr(case, mb):
    c = case
    if c.name in ("tet10", "hub"):          # a partial last slice (cook, beam2 and hub_elast have 33, 9 and 4 full ones)
        assert c.N % 64 != 0
    check_block_product(c, mb)


# ---- eigenpairs ----------------------------------------------------------------------------------------------------------------------
def check_lowest_modes(c, n_modes, tol):
    """the device's run at these settings against the reference pairs of its own K and m, within the bounds of the docstring"""
    om, phi = c.modes()
    mir = mirror_of(c, n_modes, tol)
    r = device_of(c, n_modes, tol)
    eig = MO.eig_error(r.omega2, om ** 2)
    dist = MO.subspace_distance(r.modes, phi[:, :n_modes], c.m)
    orth = MO.orthonormality(r.modes, c.m)
    print(f"{c.name}: n_modes {n_modes}, MB {r.block}, tol {tol:g}: device {r.iterations} iterations ({r.restarts} restarts), mirror {mir.iterations}; "
          f"largest residual {r.residuals.max():.3e} (mirror {mir.residuals.max():.3e}); eigenvalue error {eig:.3e} (mirror {mir.eig:.3e}); "
          f"subspace distance {dist:.3e} (mirror {mir.dist:.3e}); orthonormality {orth:.3e} (mirror {mir.orth:.3e}); omega_1 {r.omega[0]:.6e}")
    assert r.reason == 1 and r.block == mir.block
    assert r.modes.shape == (c.N, n_modes) and (r.residuals <= tol).all()
    assert (np.diff(r.omega2) >= 0.0).all() and np.array_equal(r.omega, np.sqrt(r.omega2))
    assert eig <= 16 * max(mir.eig, FLOOR)
    assert dist <= 16 * max(mir.dist, FLOOR)
    assert orth <= 16 * max(mir.orth, FLOOR)
    # the convention: the entry of largest magnitude is positive, the first of equal ones decides
    big = np.abs(r.modes).argmax(0)
    assert (r.modes[big, np.arange(n_modes)] > 0.0).all()
    # the residuals are those of the returned pairs (an explicit product on the host)
    _, res = MO.residuals(c.A @ r.modes, r.modes, c.m, r.omega2)
    assert np.abs(res - r.residuals).max() <= 1e-3 * tol + 64 * c.N * EPS
    return r


@pytest.mark.parametrize("case,n_modes,tol", SETTINGS, indirect=["case"])
def test_lowest_modes_against_dense_eigh(case, n_modes, tol):
    check_lowest_modes(case, n_modes, tol)


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tet10", "hub_elast"], indirect=True)
def test_two_runs_give_the_same_bits(case):
    """no atomics and no generator state: a second run, and a run from x0 = the hashed block, repeat every bit"""
    c = case
    tol = 1e-9 if c.name == "tet10" else 1e-6
    a, cap = device_of(c, 2, tol), 4 * mirror_of(c, 2, tol).iterations
    b = c.s.modalSolve(2, tol=tol, max_iterations=cap)
    d = c.s.modalSolve(2, tol=tol, max_iterations=cap, x0=MO.start_block(c.N, 4))
    for r in (b, d):
        assert r.iterations == a.iterations and r.restarts == a.restarts and r.reason == a.reason
        assert np.array_equal(r.omega2, a.omega2) and np.array_equal(r.modes, a.modes) and np.array_equal(r.residuals, a.residuals)
    # a forced larger block is another run (and converges too); without the vectors only the numbers come back
    e = c.s.modalSolve(2, tol=tol, max_iterations=4 * cap, block=8, modes=False)
    assert e.block == 8 and e.reason == 1 and e.modes is None
    assert np.abs(e.omega2 / a.omega2 - 1.0).max() <= 16 * max(tol, FLOOR)


# ---- gamg's cycle as T --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tet10", "beam2"], indirect=True)
def test_gamg_as_the_preconditioner(case):
    """With gamg in effect and a solve behind it, W is the multigrid cycle of R, a column at a time: the same eigenvalues and
    subspace within the bounds of the Jacobi run, in far fewer iterations (printed, not asserted).  pc="jacobi" still gives the
    Jacobi run's bits."""
    c = case
    n_modes, tol = (6, 1e-9) if c.name == "tet10" else (6, 1e-6)
    om, phi = c.modes()
    mir, jac = mirror_of(c, n_modes, tol), device_of(c, n_modes, tol)
    s = c.s
    s.setPreconditioner("gamg")
    try:
        assert s.factoriseAndSolve()[1] > 0
        r = s.modalSolve(n_modes, tol=tol, max_iterations=4 * mir.iterations)
        again = s.modalSolve(n_modes, tol=tol, max_iterations=4 * mir.iterations)
        forced = s.modalSolve(n_modes, tol=tol, max_iterations=4 * mir.iterations, pc="jacobi")
    finally:
        s.setPreconditioner("jacobi")
    eig = MO.eig_error(r.omega2, om ** 2)
    dist = MO.subspace_distance(r.modes, phi[:, :n_modes], c.m)
    orth = MO.orthonormality(r.modes, c.m)
    print(f"{c.name}: n_modes {n_modes}, tol {tol:g}: gamg {r.iterations} iterations ({r.restarts} restarts), Jacobi {jac.iterations}, mirror (Jacobi) "
          f"{mir.iterations}; eigenvalue error {eig:.3e} (mirror {mir.eig:.3e}); subspace distance {dist:.3e} (mirror {mir.dist:.3e}); "
          f"orthonormality {orth:.3e}")
    assert r.pc == "gamg" and jac.pc == "jacobi" and forced.pc == "jacobi"
    assert r.reason == 1 and (r.residuals <= tol).all()
    assert eig <= 16 * max(mir.eig, FLOOR)
    assert dist <= 16 * max(mir.dist, FLOOR)
    assert orth <= 16 * max(mir.orth, FLOOR)
    assert again.iterations == r.iterations and np.array_equal(again.omega2, r.omega2) and np.array_equal(again.modes, r.modes)
    assert forced.iterations == jac.iterations and np.array_equal(forced.omega2, jac.omega2) and np.array_equal(forced.modes, jac.modes)


# ---- the lowest mode in the implicit stepper ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_the_lowest_mode_oscillates_with_the_returned_omega(case):
    """u0 = phi_1 from the device, v0 = 0, no load, Newmark (1/4, 1/2), 100 steps at 20 x the Gershgorin step:
    u_n = cos(n vartheta) phi_1 with vartheta = 2 atan(omega_1 dt / 2) and the device's omega_1.  The mirror of the stepper starts
    from the same vector, so that its figure carries the same residual of the mode."""
    c = case
    n_modes, tol = (2, 1e-9) if c.name == "tet10" else (6, 1e-6)
    r = device_of(c, n_modes, tol)
    phi, om = r.modes[:, 0].copy(), r.omega[0]
    n_steps, dt = 100, 20.0 * c.dt
    want = np.cos(n_steps * 2.0 * np.arctan(0.5 * om * dt)) * phi
    scale = np.abs(phi).max()
    st = IR.ImplicitStepper(c.A, np.zeros(c.N), c.m, dt, u0=phi, solve="pcg", rtol=RTOL)
    st.run(n_steps)
    mirror = np.abs(st.u - want).max() / scale
    s = c.device(0.0, phi, None, ([0.0, 1.0], [0.0, 0.0]))
    with tolerances(s, rtol=RTOL):
        s.implicitRun(dt, n_steps)
    got = np.abs(s.dynamicsState()[1] - want).max() / scale
    print(f"{c.name}: omega_1 {om:.6e}, omega_1 dt {om * dt:.3f}: modal error device {got:.3e}, mirror-PCG {mirror:.3e}")
    assert got <= 16 * mirror


# ---- states, errors, isolation ------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(pf.PfemError) as ei:
        call()
    return ei.value.code


def test_state_errors_and_isolation(golden_dir):
    mesh = H.read_mesh(f"{golden_dir}/input/tet10")
    dm, conn, xyz, edof = D._setup(pf.POISSON_TET, mesh)
    N = dm.size_global
    s = pf.PetscSolver().initialise(N, N)
    assert _code(lambda: s.modalSolve(2)) == L.ERR_STATE                        # no mesh, no mass
    s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    assert _code(lambda: s.modalSolve(2)) == L.ERR_STATE                        # no dynamicsSetup
    s.assemble(ANISO, H.TIMEDATA)
    assert _code(lambda: s.modalSolve(2)) == L.ERR_STATE
    s.dynamicsSetup(ANISO, 2.5)
    for kw in (dict(n_modes=0), dict(n_modes=13), dict(block=5), dict(n_modes=6, block=4), dict(tol=0.0), dict(tol=float("nan")),
               dict(max_iterations=0), dict(pc=9)):
        assert _code(lambda: s.modalSolve(**{"n_modes": 2, **kw})) == L.ERR_ARG, kw
    with pytest.raises(ValueError):
        s.modalSolve(2, x0=np.zeros((N, 8)))
    # a cap that is reached: reason -1, the pairs and residuals of that moment, PFEM_OK
    r = s.modalSolve(2, tol=1e-9, max_iterations=5)
    assert r.reason == -1 and r.iterations == 5 and (r.residuals > 1e-9).any() and np.isfinite(r.modes).all() and (r.omega2 > 0).all()
    # a start block with a repeated column: breakdown at once
    x0 = MO.start_block(N, 4)
    x0[:, 3] = x0[:, 0]
    r = s.modalSolve(2, x0=x0)
    assert r.reason == -2 and r.iterations == 0
    # gamg in effect but no gamg solve since the assemble: the point Jacobi runs, and asking for gamg by name is refused
    s.setPreconditioner("gamg")
    assert s.modalSolve(2, tol=1e-6, max_iterations=400).pc == "jacobi"
    assert _code(lambda: s.modalSolve(2, pc="gamg")) == L.ERR_STATE
    # the solve beside it is untouched: the same iteration count and solution bits before and after, with Jacobi and with gamg
    # (under gamg the run's T is the cycle of that solve)
    for pc in ("jacobi", "gamg"):
        s.setPreconditioner(pc)
        its0 = s.factoriseAndSolve()[0]
        x_before = s.getSolution()
        rhs = s.getRHS()
        r = s.modalSolve(6, tol=1e-6, max_iterations=400)
        assert r.reason == 1 and r.pc == pc
        assert np.array_equal(s.getRHS(), rhs) and np.array_equal(s.getSolution(), x_before), pc
        assert s.factoriseAndSolve()[0] == its0 and np.array_equal(s.getSolution(), x_before), pc
    s.assemble(ANISO, H.TIMEDATA)                                               # new values: the cycle's set-up is not theirs
    assert s.modalSolve(2, tol=1e-6, max_iterations=400).pc == "jacobi"
    s.setPreconditioner("jacobi")
    # an implicit run continues exactly across a modal run
    rng = np.random.default_rng(3)
    u0, v0 = rng.standard_normal(N), rng.standard_normal(N)
    dt = 20.0 * s.stableDt()
    s.setDynamicsState(0.0, u0, v0)
    s.implicitRun(dt, 10)
    s.implicitRun(dt, 10)
    t_a, u_a, v_a = s.dynamicsState()
    s.setDynamicsState(0.0, u0, v0)
    s.implicitRun(dt, 10)
    s.modalSolve(2, tol=1e-6, max_iterations=400)
    s.implicitRun(dt, 10)
    t_b, u_b, v_b = s.dynamicsState()
    assert t_a == t_b and np.array_equal(u_a, u_b) and np.array_equal(v_a, v_b)
    # ... and an explicit one
    de = 0.9 * s.stableDt()
    s.setDynamicsState(0.0, u0, v0)
    s.dynamicsRun(de, 60)
    _, u_a, v_a = s.dynamicsState()
    s.setDynamicsState(0.0, u0, v0)
    s.dynamicsRun(de, 30)
    s.modalSolve(2, tol=1e-6, max_iterations=400)
    s.dynamicsRun(de, 30)
    _, u_b, v_b = s.dynamicsState()
    assert np.array_equal(u_a, u_b) and np.array_equal(v_a, v_b)
    s.buildPattern()                                                            # a new pattern drops the mass
    assert _code(lambda: s.modalSolve(2)) == L.ERR_STATE
    # more than one rank: refused before anything is launched
    s.assemble(ANISO, H.TIMEDATA)
    s.dynamicsSetup(ANISO, 2.5)
    cb = lambda *a: 0      # noqa: E731
    s.setCommHost(0, 2, cb, cb)
    assert _code(lambda: s.modalSolve(2)) == L.ERR_STATE
    s.free(collective=False)
    # the compat path has no mesh on the device, hence no mass
    compat = pf.tetrapoissonparallelimpl1(H.gen_box_tets(-1, 1, 3, -1, 1, 3, -1, 1, 3), rtol=1e-6, mode="compat").solver
    assert _code(lambda: compat.modalSolve(2)) == L.ERR_STATE
