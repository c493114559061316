"""Implicit time stepping on the device (pfem_dynamics_run_implicit): Newmark and the theta-method on the lumped mass, every step
one Jacobi-PCG solve of (K + sigma diag(m)) d = b -- against the numpy mirror (tests/implicit_reference.py, itself checked
against closed forms in tests/test_implicit_reference.py).

The meshes are test_gpu_dynamics.py's (tet10: 729 dofs, the tail of a four-rows-a-thread kernel and one block of partials; Cook:
2 112 dofs, several blocks, a surface load; beam2: 576 dofs, two densities; hub and hub_elast: hub rows), and the mirror runs on
the K, the load and the mass the device holds.  Every bound is computed here: 16 x the figure the mirror's own PCG reaches at the
same rtol -- against its LU form, or against the closed form.  The factor is the project's standing margin for the one thing the
device does differently: it adds a row, and a dot product, in slices with fma.  The device's own figure never enters a bound."""
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import dynamics_reference as DR
import implicit_reference as IR
import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_dynamics import ANISO, NAMES, PLAIN, case, rel      # noqa: F401  (case: the fixture that builds a Case once)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
RTOL = 1e-13


@contextmanager
def tolerances(s, **kw):
    s.setTolerances(**kw)
    try:
        yield s
    finally:
        s.setTolerances()


def _scheme_kw(scheme):
    """(keywords of the mirror, keywords of implicitRun)"""
    if scheme == "newmark":
        return dict(scheme="newmark"), dict(scheme="newmark")
    theta = float(scheme.split("=")[1])
    return dict(scheme="theta", theta=theta), dict(scheme="theta", theta=theta)


def _state(c, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(c.N), rng.standard_normal(c.N)


def _mirrors(c, dt, n_steps, every, kw, rtol, pcg_orders=(False,), lu=True):
    """mirror-LU and mirror-PCG(s) run over the same steps: [(rows, u, v, iterations)]"""
    out = []
    runs = ([("lu", c.A)] if lu else []) + [("pcg", c.Arev if rev else c.A) for rev in pcg_orders]
    for solve, A in runs:
        st = IR.ImplicitStepper(A, c.f, c.m, dt, solve=solve, rtol=rtol, **kw)
        rows = st.run(n_steps, every)
        out.append((rows, st.u.copy(), st.v.copy(), np.array(st.iterations)))
    return out


# ---- 1. trajectory ---------------------------------------------------------------------------------------------------------------
TRAJ = [(n, "newmark") for n in NAMES] + [(n, s) for n in ("tet10", "hub") for s in ("theta=1.0", "theta=0.5")]


@pytest.mark.parametrize("case,scheme", TRAJ, indirect=["case"])
def test_100_steps_under_a_ramp_against_the_mirror(case, scheme):
    """100 steps from a random state under a ramp at 20 x the Gershgorin step, rtol = 1e-13, Newmark damped with alpha = 0.1 / dt:
    u, v and every column of the rows of every 7th step, device against mirror-LU, within 16 x (mirror-PCG - mirror-LU)."""
    c = case
    mkw, dkw = _scheme_kw(scheme)
    u0, v0 = _state(c, 17)
    dt, n_steps, every = 20.0 * c.dt, 100, 7
    alpha = 0.1 / dt if scheme == "newmark" else 0.0
    curve = ([0.0, 50.5 * dt, 140.0 * dt], [0.0, 1.0, 0.25])
    probes = np.array([0, c.N // 2, c.N - 1])
    (rl, ul, vl, _), (rp, up, vp, ip) = _mirrors(c, dt, n_steps, every, dict(alpha=alpha, u0=u0, v0=v0, curve=curve, **mkw), RTOL)
    s = c.device(0.0, u0, v0, curve, probes)
    with tolerances(s, rtol=RTOL):
        hist, its = s.implicitRun(dt, n_steps, alpha=alpha, sample_every=every, **dkw)
    t, u, v = s.dynamicsState()
    assert hist.shape == (n_steps // every, 10) and its.shape == (n_steps,)
    assert t == n_steps * dt and np.array_equal(hist[:, 0], rl[:, 0])
    print(f"{c.name} {scheme}: iterations device {its.min()}..{its.max()}, mirror {ip.min()}..{ip.max()}")
    for name, got, lu, pcg in (("u", u, ul, up), ("v", v, vl, vp), ("T", hist[:, 1], rl[:, 1], rp[:, 1]), ("S", hist[:, 2], rl[:, 2], rp[:, 2]),
                               ("W", hist[:, 3], rl[:, 3], rp[:, 3])):
        fig, bound = np.abs(got - lu).max(), 16 * np.abs(pcg - lu).max()
        print(f"{c.name} {scheme}: {name} device vs mirror-LU {fig:.3e}, bound 16 x {bound / 16:.3e} (magnitude {np.abs(lu).max():.3e})")
        assert fig <= bound, name


# ---- 2. iterations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1.0, 20.0])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_iterations_per_step_are_the_mirrors(case, factor):
    """Per step of 40 damped Newmark steps under a ramp: |device - mirror-PCG(A)| <= max(2, 4 x |mirror-PCG(A) - mirror-PCG(Arev)|)
    -- a threshold crossing moves a count by one on each side.  rtol = 1e-8: far enough above the rounding level of the
    recurrence for the count to be a property of the operator.  At 1 x the operator is mass dominated: a dinv without sigma m,
    or a (p, Ap) without sum sigma m p^2, shows as many more iterations or as a breakdown."""
    c = case
    u0, v0 = _state(c, 31)
    dt, n_steps = factor * c.dt, 40
    alpha = 0.1 / dt
    curve = ([0.0, 20.5 * dt], [0.0, 1.0])
    kw = dict(alpha=alpha, u0=u0, v0=v0, curve=curve)
    (_, _, _, ia), (_, _, _, ir) = _mirrors(c, dt, n_steps, 0, kw, 1e-8, pcg_orders=(False, True), lu=False)
    s = c.device(0.0, u0, v0, curve)
    with tolerances(s, rtol=1e-8):
        _, its = s.implicitRun(dt, n_steps, alpha=alpha)
    print(f"{c.name} dt = {factor:g} x: device {its.tolist()}")
    print(f"{c.name} dt = {factor:g} x: mirror {ia.tolist()}; orders differ by at most {np.abs(ia - ir).max()}")
    assert (np.abs(its - ia) <= np.maximum(2, 4 * np.abs(ia - ir))).all()


# ---- 3. single mode and energy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["newmark", "theta=1.0", "theta=0.5"])
@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_a_single_mode_on_the_device(case, scheme):
    """u0 = phi_k, v0 = 0, no load, 100 steps.  Newmark (1/4, 1/2): u_n = cos(n vartheta) phi_k, vartheta = 2 atan(omega dt / 2), at
    20 x the Gershgorin step; theta-method: u_n = g^n phi_k, g = (1 - (1 - theta) lambda dt) / (1 + theta lambda dt), lambda dt = 0.05."""
    c = case
    mkw, dkw = _scheme_kw(scheme)
    om, phi = c.modes()
    k, n_steps = 3, 100
    if scheme == "newmark":
        dt = 20.0 * c.dt
        factor = np.cos(n_steps * 2.0 * np.arctan(0.5 * om[k] * dt))
    else:
        lam = om[k] ** 2
        dt = 0.05 / lam
        factor = ((1.0 - (1.0 - mkw["theta"]) * lam * dt) / (1.0 + mkw["theta"] * lam * dt)) ** n_steps
    want = factor * phi[:, k]
    scale = np.abs(phi[:, k]).max()
    st = IR.ImplicitStepper(c.A, np.zeros(c.N), c.m, dt, u0=phi[:, k], solve="pcg", rtol=RTOL, **mkw)
    st.run(n_steps)
    mirror = np.abs(st.u - want).max() / scale
    s = c.device(0.0, phi[:, k], None, ([0.0, 1.0], [0.0, 0.0]))
    with tolerances(s, rtol=RTOL):
        s.implicitRun(dt, n_steps, **dkw)
    got = np.abs(s.dynamicsState()[1] - want).max() / scale
    print(f"{c.name} {scheme}: modal error device {got:.3e}, mirror-PCG {mirror:.3e}")
    assert got <= 16 * mirror


@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_T_plus_S_is_constant_on_the_device(case):
    """undamped, unloaded, beta = 1/4, gamma = 1/2, 300 steps at 50 x the Gershgorin step: the relative spread of T + S."""
    c = case
    u0, v0 = _state(c, 5)
    dt, n_steps = 50.0 * c.dt, 300
    st = IR.ImplicitStepper(c.A, np.zeros(c.N), c.m, dt, u0=u0, v0=v0, solve="pcg", rtol=RTOL)
    h = st.run(n_steps, 1)
    e = h[:, 1] + h[:, 2]
    mirror = (e.max() - e.min()) / np.abs(e).max()
    s = c.device(0.0, u0, v0, ([0.0, 1.0], [0.0, 0.0]))
    with tolerances(s, rtol=RTOL):
        hd, its = s.implicitRun(dt, n_steps, sample_every=1)
    ed = hd[:, 1] + hd[:, 2]
    got = (ed.max() - ed.min()) / np.abs(ed).max()
    print(f"{c.name}: spread of T + S device {got:.3e}, mirror-PCG {mirror:.3e}; T + S = {ed[0]:.6e}; iterations {its.min()}..{its.max()}")
    assert hd.shape == (n_steps, 4)
    assert got <= 16 * mirror


# ---- 4. static limit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PLAIN, indirect=True)
def test_backward_euler_reaches_the_static_solution(case):
    """three backward-Euler steps at 1e6 x the Gershgorin step under the constant load against sparse LU of K u = f"""
    c = case
    x = spl.splu(sp.csc_matrix(c.A)).solve(c.f)
    dt = 1e6 * c.dt
    st = IR.ImplicitStepper(c.A, c.f, c.m, dt, scheme="theta", theta=1.0, solve="pcg", rtol=1e-10)
    st.run(3)
    mirror = rel(st.u, x)
    s = c.device()
    with tolerances(s, rtol=1e-10):
        _, its = s.implicitRun(dt, 3, scheme="theta", theta=1.0)
    got = rel(s.dynamicsState()[1], x)
    print(f"{c.name}: static limit device {got:.3e}, mirror-PCG {mirror:.3e}; iterations device {its.tolist()}, mirror {st.iterations}")
    assert got <= 16 * mirror


# ---- 5. continuation and determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,scheme", [("tet10", "newmark"), ("cook", "newmark"), ("hub_elast", "newmark"), ("tet10", "theta=0.5")],
                         indirect=["case"])
def test_runs_continue_exactly(case, scheme):
    """run(100) = run(50); run(50) = run(1) x 100 = run(100) again, bit for bit in u, v, every row and every iteration count."""
    c = case
    _, dkw = _scheme_kw(scheme)
    u0, v0 = _state(c, 23)
    dt = 20.0 * c.dt
    alpha = 0.3 / dt if scheme == "newmark" else 0.0
    curve = ([0.0, 40.0 * dt, 90.0 * dt], [0.2, 1.0, -0.5])
    probes = [1, c.N - 2]
    results = []
    with tolerances(c.s, rtol=1e-8):
        for chunks in ([100], [50, 50], [1] * 100, [100]):
            s = c.device(0.5, u0, v0, curve, probes)
            parts = [s.implicitRun(dt, n, alpha=alpha, sample_every=1, **dkw) for n in chunks]
            results.append((np.vstack([p[0] for p in parts]), np.concatenate([p[1] for p in parts])) + s.dynamicsState())
    h0, i0, t0, uu0, vv0 = results[0]
    assert h0.shape == (100, 8) and np.isfinite(h0).all() and i0.min() > 0
    assert np.array_equal(h0[-1, 4:6], uu0[probes]) and np.array_equal(h0[-1, 6:8], vv0[probes]) and h0[-1, 0] == t0
    for h, i, t, u, v in results[1:]:
        assert t == t0 and np.array_equal(u, uu0) and np.array_equal(v, vv0)
        assert np.array_equal(h, h0) and np.array_equal(i, i0)
    # another dt continues from the state reached: the mirror does the same
    s = c.device(0.5, u0, v0, curve, probes)
    with tolerances(s, rtol=1e-8):
        s.implicitRun(dt, 10, alpha=alpha, **dkw)
        s.implicitRun(0.5 * dt, 4, alpha=alpha, **dkw)
    assert s.dynamicsState()[0] == (0.5 + 10.0 * dt) + 4.0 * (0.5 * dt)


# ---- 6. at rest ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["newmark", "theta=1.0"])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_at_rest_nothing_moves(case, scheme):
    """zero state and zero load factor: zero iterations on every step (no division by (p, w) = 0), the state exactly 0, finite rows"""
    c = case
    _, dkw = _scheme_kw(scheme)
    s = c.device(0.0, None, None, ([0.0, 1.0], [0.0, 0.0]), [0])
    hist, its = s.implicitRun(5.0 * c.dt, 6, sample_every=2, **dkw)
    t, u, v = s.dynamicsState()
    assert not its.any() and not u.any() and not v.any()
    assert hist.shape == (3, 6) and np.isfinite(hist).all() and not hist[:, 1:].any()


# ---- 7. errors and isolation ---------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(pf.PfemError) as ei:
        call()
    return ei.value.code


def test_state_errors_and_isolation(golden_dir):
    mesh = H.read_mesh(f"{golden_dir}/input/tet10")
    dm, conn, xyz, edof = D._setup(pf.POISSON_TET, mesh)
    N = dm.size_global
    s = pf.PetscSolver().initialise(N, N)
    assert _code(lambda: s.implicitRun(1e-3, 1)) == L.ERR_STATE                 # no dynamics set-up
    s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    assert _code(lambda: s.implicitRun(1e-3, 1)) == L.ERR_STATE
    s.assemble(ANISO, H.TIMEDATA)
    s.dynamicsSetup(ANISO, 1.0)
    dt = 20.0 * s.stableDt()
    for kw in (dict(dt=0.0), dict(dt=-dt), dict(dt=float("nan")), dict(n_steps=-1), dict(beta=0.0), dict(gamma=0.4), dict(alpha=-1.0),
               dict(scheme="theta", theta=0.0), dict(scheme="theta", theta=1.1), dict(scheme="theta", alpha=0.1), dict(sample_every=-1)):
        assert _code(lambda: s.implicitRun(**{"dt": dt, "n_steps": 1, **kw})) == L.ERR_ARG, kw
    rc = L.lib().pfem_dynamics_run_implicit(s._h, 7, dt, 1, 0.25, 0.5, 0.0, 0, None, None, None, None)
    assert rc == L.ERR_ARG                                                      # an unknown scheme
    # the scheme switches need a new state
    rng = np.random.default_rng(3)
    u0, v0 = rng.standard_normal(N), rng.standard_normal(N)
    s.setDynamicsState(0.0, u0, v0)
    s.implicitRun(dt, 2)
    s.implicitRun(0.5 * dt, 2, beta=0.3, gamma=0.6)                             # another dt, other parameters: continues
    assert s.dynamicsState()[0] == 2.0 * dt + 2.0 * (0.5 * dt)
    assert _code(lambda: s.implicitRun(dt, 1, scheme="theta")) == L.ERR_STATE
    assert _code(lambda: s.dynamicsRun(0.01 * dt, 1)) == L.ERR_STATE
    s.setDynamicsState(0.0, u0, v0)
    s.implicitRun(dt, 2, scheme="theta")
    assert _code(lambda: s.implicitRun(dt, 1)) == L.ERR_STATE
    s.setDynamicsState(0.0, u0, v0)
    s.dynamicsRun(0.01 * dt, 2)
    assert _code(lambda: s.implicitRun(dt, 1)) == L.ERR_STATE
    # a solve that runs out of iterations stops the run: nothing done, the state as it was
    s.setDynamicsState(0.25, u0, v0)
    s.setTolerances(rtol=1e-12, maxits=2)
    with pytest.raises(pf.PfemError) as ei:
        s.implicitRun(dt, 3, sample_every=1)
    assert ei.value.code == L.ERR_DIVERGED and ei.value.steps_done == 0 and len(ei.value.iterations) == 0 and len(ei.value.history) == 0
    t, u, v = s.dynamicsState()
    assert t == 0.25 and np.array_equal(u, u0) and np.array_equal(v, v0)
    s.setTolerances()
    # the solve beside it is untouched: the same iteration count and solution bits before and after, with Jacobi and with gamg
    for pc in ("jacobi", "gamg"):
        s.setPreconditioner(pc)
        its0 = s.factoriseAndSolve()[0]
        x0 = s.getSolution()
        s.setDynamicsState(0.0, u0, v0)
        _, its = s.implicitRun(dt, 20)
        assert its.min() > 0
        assert s.factoriseAndSolve()[0] == its0 and np.array_equal(s.getSolution(), x0), pc
    s.setPreconditioner("jacobi")
    # an explicit run after a new state still equals its mirror
    rowptr, cols, vals = s.getCSR()
    p = SimpleNamespace(rowptr=rowptr, cols=cols, vals=vals)
    f, m = s.getRHS(), s.dynamicsMass()
    de = 0.9 * s.stableDt()
    fwd, rev = (DR.Stepper(DR.csr(p, reverse=q), f, m, de, u0=u0, v0=v0) for q in (False, True))
    fwd.run(60), rev.run(60)
    s.setDynamicsState(0.0, u0, v0)
    s.dynamicsRun(de, 60)
    _, u, v = s.dynamicsState()
    assert rel(u, fwd.u) <= 16 * rel(rev.u, fwd.u) and rel(v, fwd.v) <= 16 * rel(rev.v, fwd.v)
    s.buildPattern()                                                            # a new pattern drops the mass and the run's buffers
    assert _code(lambda: s.implicitRun(dt, 1)) == L.ERR_STATE
    s.assemble(ANISO, H.TIMEDATA)
    s.dynamicsSetup(ANISO, 1.0)
    cb = lambda *a: 0      # noqa: E731
    s.setCommHost(0, 2, cb, cb)                                                 # more than one rank: refused before anything is launched
    assert _code(lambda: s.implicitRun(dt, 1)) == L.ERR_STATE
    s.free(collective=False)


# ---- 8. drivers ------------------------------------------------------------------------------------------------------------------------
def test_tetra_driver_with_newmark_at_the_programs_dt():
    """tetraelasticityexplicit on the small beam, steel under its own weight switched on at t = 0: the PROGRAM's dt = 0.01, refused
    for central differences, runs with integrator="newmark"; 20 steps against mirror-LU within 16 x (mirror-PCG - mirror-LU)."""
    mesh = H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
    ed = np.array([207.0e9, H._f32(0.3), 1.0, 0.0, -9.81 * 7800.0, 0.0])
    with pytest.raises(ValueError):
        pf.tetraelasticityexplicit(mesh, elemData=ed)
    tip = int(np.nonzero((mesh.xyz[1] == 6.0) & (mesh.xyz[0] == 0.5) & (mesh.xyz[2] == 0.5))[0][0])
    r = pf.tetraelasticityexplicit(mesh, n_steps=20, elemData=ed, integrator="newmark", rtol=1e-12, sample_every=5, probes=[(tip, 1)])
    assert r.dt == 0.01 and r.t == 20 * 0.01 and r.iterations.shape == (20,) and r.iterations.min() > 0
    rowptr, cols, vals = r.solver.getCSR()
    p = SimpleNamespace(rowptr=rowptr, cols=cols, vals=vals)
    f, m = r.solver.getRHS(), r.solver.dynamicsMass()
    lu, pcg = (IR.ImplicitStepper(DR.csr(p), f, m, 0.01, solve=q, rtol=1e-12) for q in ("lu", "pcg"))
    hl, hp = lu.run(20, 5), pcg.run(20, 5)
    print(f"tetra driver: dt / stable dt {0.01 / r.stable_dt:.1f}, iterations device {r.iterations.min()}..{r.iterations.max()}, "
          f"mirror {min(pcg.iterations)}..{max(pcg.iterations)}; tip u_y {r.history[-1, 4]:.4e}")
    for name, got, a, b in (("u", r.soln_free, lu.u, pcg.u), ("v", r.velo_free, lu.v, pcg.v), ("rows", r.history[:, 1:4], hl[:, 1:], hp[:, 1:])):
        fig, bound = np.abs(got - a).max(), 16 * np.abs(b - a).max()
        print(f"tetra driver: {name} device vs mirror-LU {fig:.3e}, bound 16 x {bound / 16:.3e}")
        assert fig <= bound, name
    g = r.dm.NodeDofArrayNew[r.dm.node_map_get_new[tip], 1]
    assert r.history.shape == (4, 6) and r.history[-1, 4] == r.soln_free[g] and r.history[-1, 5] == r.velo_free[g]
    assert pf.tetraelasticityexplicit(mesh, dt=1e-9, n_steps=0, elemData=ed).iterations is None


def test_poissontransient_decays_to_the_steady_state(golden_dir):
    """backward Euler on tet10 from u = 0 under the constant load (the Dirichlet lift): 30 steps at 1000 x the Gershgorin step
    against sparse LU of K u = f, within 16 x what the mirror's PCG reaches"""
    mesh = H.read_mesh(f"{golden_dir}/input/tet10")
    r0 = pf.poissontransient(mesh, dt=1.0, n_steps=0, capacity=2.0)
    dt = 1000.0 * r0.stable_dt
    r = pf.poissontransient(mesh, dt=dt, n_steps=30, capacity=2.0, rtol=1e-10, sample_every=10)
    rowptr, cols, vals = r.solver.getCSR()
    A = DR.csr(SimpleNamespace(rowptr=rowptr, cols=cols, vals=vals))
    f, m = r.solver.getRHS(), r.solver.dynamicsMass()
    x = spl.splu(sp.csc_matrix(A)).solve(f)
    st = IR.ImplicitStepper(A, f, m, dt, scheme="theta", theta=1.0, solve="pcg", rtol=1e-10)
    st.run(30)
    got, mirror = rel(r.soln_free, x), rel(st.u, x)
    print(f"poissontransient: steady state device {got:.3e}, mirror-PCG {mirror:.3e}; iterations {r.iterations.min()}..{r.iterations.max()}")
    assert r.history.shape == (3, 4) and r.t == 30 * dt and r.iterations.shape == (30,)
    assert got <= 16 * mirror
    assert np.abs(r.solnVTK[:, 0]).max() > 0.0
