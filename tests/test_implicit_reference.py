"""The numpy mirror of the implicit time stepping (tests/implicit_reference.py) against closed forms, so that the yardstick of
the GPU tests is itself checked: a single mode under Newmark (1/4, 1/2) and under the theta-method, the invariant T + S of the
undamped, unloaded trapezoidal rule, the PCG mirror against the LU mirror -- and what the C entry points answer without a
device.  Mesh: the 10^3 x 6-tet Poisson box (729 free dofs).

Bounds: 16 x eps x steps x the magnitude printed beside the figure -- every step adds a few roundings of relative size eps to a
quantity of that magnitude, and neither scheme amplifies them (|g| <= 1 for every mode)."""
import ctypes as C

import numpy as np
import pytest

import dynamics_reference as DR
import implicit_reference as IR
from pfemfort_amd import _lib
from pfemfort_amd import host as H

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def box():
    mesh, p, m = DR.poisson_box(H, 10)
    A = IR.csr(p)
    om, phi = IR.modes(A, m)
    return {"p": p, "m": m, "A": A, "Arev": IR.csr(p, reverse=True), "om": om, "phi": phi, "dt": DR.gershgorin_dt(A, m)}


def test_a_single_mode_under_newmark(box):
    """u0 = phi, v0 = 0, no load, beta = 1/4, gamma = 1/2: u_n = cos(n vartheta) phi with vartheta = 2 atan(omega dt / 2)."""
    A, m, om, phi = box["A"], box["m"], box["om"], box["phi"]
    k, steps, dt = 3, 200, 20.0 * box["dt"]
    st = IR.ImplicitStepper(A, np.zeros(A.shape[0]), m, dt, u0=phi[:, k])
    st.run(steps)
    vth = 2.0 * np.arctan(0.5 * om[k] * dt)
    mag = np.abs(phi[:, k]).max()
    err = np.abs(st.u - np.cos(steps * vth) * phi[:, k]).max()
    print(f"newmark mode: error {err:.3e}, magnitude {mag:.3e}, omega dt {om[k] * dt:.3f}, bound {16 * EPS * steps * mag:.3e}")
    assert err <= 16 * EPS * steps * mag


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_a_single_mode_under_the_theta_method(box, theta):
    """u0 = phi, no load: u_n = g^n phi with g = (1 - (1 - theta) lambda dt) / (1 + theta lambda dt), lambda = omega^2."""
    A, m, om, phi = box["A"], box["m"], box["om"], box["phi"]
    k, steps = 3, 100
    lam = om[k] ** 2
    dt = 0.05 / lam
    st = IR.ImplicitStepper(A, np.zeros(A.shape[0]), m, dt, scheme="theta", theta=theta, u0=phi[:, k])
    st.run(steps)
    g = (1.0 - (1.0 - theta) * lam * dt) / (1.0 + theta * lam * dt)
    mag = np.abs(phi[:, k]).max()
    err = np.abs(st.u - g ** steps * phi[:, k]).max()
    print(f"theta = {theta} mode: error {err:.3e}, magnitude {mag:.3e}, g^n {g ** steps:.3e}, bound {16 * EPS * steps * mag:.3e}")
    assert err <= 16 * EPS * steps * mag
    assert np.allclose(st.v, (g ** steps - g ** (steps - 1)) / dt * phi[:, k], rtol=1e-9, atol=1e-12 * mag / dt)


def test_T_plus_S_is_conserved_by_the_trapezoidal_rule(box):
    """undamped, unloaded, beta = 1/4, gamma = 1/2, dt = 50 x the Gershgorin step, 300 steps: the spread of T + S against T + S."""
    A, m = box["A"], box["m"]
    N, steps = A.shape[0], 300
    rng = np.random.default_rng(5)
    st = IR.ImplicitStepper(A, np.zeros(N), m, 50.0 * box["dt"], u0=rng.standard_normal(N), v0=rng.standard_normal(N))
    h = st.run(steps, 1)
    e = h[:, 1] + h[:, 2]
    spread, mag = e.max() - e.min(), np.abs(e).max()
    print(f"T + S: spread {spread:.3e}, magnitude {mag:.3e}, bound {16 * EPS * steps * mag:.3e}")
    assert spread <= 16 * EPS * steps * mag


@pytest.mark.parametrize("scheme", ["newmark", "theta"])
def test_the_pcg_mirror_follows_the_lu_mirror(box, scheme):
    """50 loaded, damped steps under a ramp at 20 x the Gershgorin step: PCG at rtol = 1e-13 against LU, in both orders of the
    row sums (their iteration counts are printed: near rounding level a count moves by a few with the order of a sum); under
    Newmark at dt = 1 x the operator is mass dominated and far fewer iterations do."""
    A, Arev, m, f = box["A"], box["Arev"], box["m"], box["p"].rhs
    N = A.shape[0]
    rng = np.random.default_rng(11)
    u0, v0 = rng.standard_normal(N), rng.standard_normal(N)
    dt = 20.0 * box["dt"]
    kw = dict(scheme=scheme, alpha=0.1 if scheme == "newmark" else 0.0, u0=u0, v0=v0, curve=([0.0, 30.5 * dt], [0.0, 1.0]))
    lu = IR.ImplicitStepper(A, f, m, dt, **kw)
    lu.run(50)
    out = []
    for M in (A, Arev):
        st = IR.ImplicitStepper(M, f, m, dt, solve="pcg", rtol=1e-13, **kw)
        st.run(50)
        out.append(st)
    mag = np.abs(lu.u).max()
    err = max(np.abs(s.u - lu.u).max() for s in out)
    its = np.array([s.iterations for s in out])
    # a solve stopped at rtol leaves an error of at most rtol x kappa x |d|, and kappa of the Jacobi-scaled shifted operator is
    # about 1 + (the largest eigenvalue of M^-1 K) / sigma; 50 steps add up
    om_max = box["om"][-1]
    kappa = 1.0 + (0.25 * (om_max * dt) ** 2 if scheme == "newmark" else om_max ** 2 * dt)
    bound = 50 * 1e-13 * kappa * mag
    print(f"{scheme}: pcg vs lu {err:.3e} of {mag:.3e}, kappa {kappa:.1f}, bound {bound:.3e}; iterations {its[0].min()}..{its[0].max()}, "
          f"orders differ by {np.abs(its[0] - its[1]).max()}")
    assert err <= bound
    if scheme == "newmark":          # sigma ~ 1 / dt^2: at the Gershgorin step omega_max dt <= 2 and kappa <= 1 + 1/4 x 4 = 2
        one = IR.ImplicitStepper(A, f, m, box["dt"], solve="pcg", rtol=1e-13, **{**kw, "curve": None})
        one.run(5)
        print(f"{scheme}: iterations at dt = 1 x: {one.iterations}")
        assert max(one.iterations) < min(its[0])


def test_at_rest_takes_no_iterations(box):
    A, m = box["A"], box["m"]
    st = IR.ImplicitStepper(A, box["p"].rhs, m, box["dt"], solve="pcg", curve=([0.0, 1.0], [0.0, 0.0]))
    h = st.run(4, 1)
    assert st.iterations == [0, 0, 0, 0] and not st.u.any() and not st.v.any() and np.isfinite(h).all()


def test_a_row_without_mass_stays_put(box):
    """a row no element touches: no matrix entries, no mass"""
    import scipy.sparse as sp
    f = box["p"].rhs
    m = box["m"].copy()
    m[[3, 77]] = 0.0
    keep = sp.diags((m > 0.0).astype(np.float64))
    A = sp.csr_matrix(keep @ box["A"] @ keep)
    rng = np.random.default_rng(2)
    u0 = rng.standard_normal(A.shape[0])
    for solve in ("lu", "pcg"):
        st = IR.ImplicitStepper(A, f, m, 5.0 * box["dt"], scheme="theta", u0=u0, solve=solve)
        st.run(3)
        assert np.array_equal(st.u[[3, 77]], u0[[3, 77]]) and np.isfinite(st.u).all()


# ---- the C entry points without a device ---------------------------------------------------------------------------------------
# (A handle exists only with a device -- pfem_solver_create returns PFEM_ERR_NOGPU without one --, so what can be asked here is
# what the entry points answer to no handle and to bad parameters; the state errors are asked on the device, in
# tests/test_gpu_implicit.py.)
def _run(L, handle, scheme, dt, n_steps, p0, p1, alpha, every=0):
    rows, done = C.c_int64(-1), C.c_int64(-1)
    rc = L.pfem_dynamics_run_implicit(handle, scheme, dt, n_steps, p0, p1, alpha, every, None, C.byref(rows), None, C.byref(done))
    return rc, rows.value, done.value


def test_run_implicit_without_a_handle_is_an_argument_error():
    L = _lib.lib()
    assert _run(L, None, _lib.SCHEME_NEWMARK, 1e-3, 10, 0.25, 0.5, 0.0) == (_lib.ERR_ARG, 0, 0)
    assert _run(L, None, _lib.SCHEME_THETA, 1e-3, 10, 1.0, 0.0, 0.0) == (_lib.ERR_ARG, 0, 0)
    us = C.c_double(0)
    assert L.pfem_dynamics_bench_implicit(None, _lib.SCHEME_NEWMARK, 1e-3, 0.25, 0.5, 10, C.byref(us)) == _lib.ERR_ARG


def test_run_implicit_refuses_bad_parameters_before_anything_else():
    """dt <= 0 or not finite, n_steps < 0, an unknown scheme, beta <= 0, gamma < 1/2, theta outside (0, 1], damping with the
    theta-method, a negative sample_every: PFEM_ERR_ARG, nothing written but zeros into rows and steps_done."""
    L = _lib.lib()
    N, T = _lib.SCHEME_NEWMARK, _lib.SCHEME_THETA
    bad = [(N, 0.0, 1, 0.25, 0.5, 0.0), (N, -1.0, 1, 0.25, 0.5, 0.0), (N, float("inf"), 1, 0.25, 0.5, 0.0), (N, float("nan"), 1, 0.25, 0.5, 0.0),
           (N, 1e-3, -1, 0.25, 0.5, 0.0), (0, 1e-3, 1, 0.25, 0.5, 0.0), (3, 1e-3, 1, 0.25, 0.5, 0.0), (N, 1e-3, 1, 0.0, 0.5, 0.0),
           (N, 1e-3, 1, 0.25, 0.49, 0.0), (N, 1e-3, 1, 0.25, 0.5, -0.1), (T, 1e-3, 1, 0.0, 0.0, 0.0), (T, 1e-3, 1, 1.5, 0.0, 0.0),
           (T, 1e-3, 1, 1.0, 0.0, 0.2)]
    for args in bad:
        assert _run(L, None, *args) == (_lib.ERR_ARG, 0, 0), args
    assert _run(L, None, N, 1e-3, 1, 0.25, 0.5, 0.0, every=-1)[0] == _lib.ERR_ARG


# ---- the per-operation functions of tests/test_gpu_stepper_kernels.py, chained over steps, against the mirrors above -----------
def _chain_pcg(P, A, m, dinv, b, z, rtol=1e-5, abstol=1e-50, dtol=1e5, maxits=10000):
    """pcg_shifted's loop written with IR.update / IR.direction / IR.dot_terms in float64, the sums by np.sum"""
    F = np.float64
    r, p, d = b, z, np.zeros_like(b)
    rzt, zzt, mpt = IR.dot_terms(P, r, dinv, m, p, F)
    beta, rn0, mp = rzt.sum(), np.sqrt(zzt.sum()), mpt.sum()
    if rn0 <= abstol:
        return d, 0, 3
    if beta < 0.0:
        return d, 0, -8
    ttol = max(rtol * rn0, abstol)
    for it in range(maxits):
        w = A @ p
        pw = p @ w + mp
        if not pw > 0.0:
            return d, it + 1, -10
        alpha = beta / pw
        r, _ = IR.update(P, alpha, p, w, m, r, F)
        rzt, zzt, _ = IR.dot_terms(P, r, dinv, m, p, F)
        rz, rn = rzt.sum(), np.sqrt(zzt.sum())
        flag = 2 if rn <= ttol else -4 if rn >= dtol * rn0 else -8 if rz < 0.0 else -3 if it + 1 >= maxits else 0
        d, p2, _ = IR.direction(alpha, rz / beta, r, dinv, p, d, F)
        if flag:
            return d, it + 1, flag
        p, beta = p2, rz
        mp = IR.dot_terms(P, r, dinv, m, p, F)[2].sum()
    return d, 0, -3


def _chain(box, scheme, solve, steps, rtol=1e-13):
    """`steps` steps by the per-operation functions beside the same steps of ImplicitStepper; solve: "lu" (the mirror's own
    factorisation solves both) or "pcg" (each its own loop)"""
    A, m, f = box["A"], box["m"], box["p"].rhs
    N = A.shape[0]
    rng = np.random.default_rng(21)
    u0, v0 = rng.standard_normal(N), rng.standard_normal(N)
    dt = 20.0 * box["dt"]
    curve = ([0.0, 30.5 * dt], [0.0, 1.0])
    alpha = 0.1 if scheme == "newmark" else 0.0
    st = IR.ImplicitStepper(A, f, m, dt, scheme=scheme, theta=0.5, alpha=alpha, u0=u0, v0=v0, curve=curve, solve=solve, rtol=rtol)
    P = IR.Par(scheme, dt, theta=0.5, alpha=alpha)
    assert P.sigma == st.sigma
    u, v, a = u0.copy(), v0.copy(), getattr(st, "a", None)
    its = []
    for n in range(steps):
        lam = IR.rhs_load_factor(P, curve, 0.0, n)
        if scheme == "newmark":
            ut, vt = IR.predict(P, u, v, a)
            b, z = IR.rhs(P, lam, f, m, vt, A @ ut, st.dinv)
        else:
            ut = vt = None
            b, z = IR.rhs(P, lam, f, m, None, A @ u, st.dinv)
        st.step()
        if solve == "lu":
            d = st._lu.solve(b)
        else:
            d, k, reason = _chain_pcg(P, A, m, st.dinv, b, z, rtol=rtol)
            assert reason == 2
            its.append(k)
        u, v, a = IR.correct(P, d, u=u, ut=ut, vt=vt)
    return st, u, v, a, its


@pytest.mark.parametrize("scheme", ["newmark", "theta"])
def test_the_chained_operations_are_the_mirror_bit_for_bit_around_one_solve(box, scheme):
    """predict, rhs and correct around the mirror's own LU solve: u, v (and a) of 20 steps carry the mirror's bits"""
    st, u, v, a, _ = _chain(box, scheme, "lu", 20)
    assert np.array_equal(u, st.u) and np.array_equal(v, st.v)
    if scheme == "newmark":
        assert np.array_equal(a, st.a)


@pytest.mark.parametrize("scheme", ["newmark", "theta"])
def test_the_chained_cg_follows_pcg_shifted(box, scheme):
    """the CG written with the per-operation update, direction and sums against pcg_shifted, 50 steps at rtol = 1e-13: the bound
    of test_the_pcg_mirror_follows_the_lu_mirror (steps x rtol x kappa x magnitude), the iteration counts printed"""
    steps = 50
    st, u, v, a, its = _chain(box, scheme, "pcg", steps)
    dt = 20.0 * box["dt"]
    om_max = box["om"][-1]
    kappa = 1.0 + (0.25 * (om_max * dt) ** 2 if scheme == "newmark" else om_max ** 2 * dt)
    mag = np.abs(st.u).max()
    err = np.abs(u - st.u).max()
    diff = np.abs(np.array(its) - np.array(st.iterations)).max()
    print(f"{scheme}: chained vs pcg_shifted {err:.3e} of {mag:.3e}, bound {steps * 1e-13 * kappa * mag:.3e}; iteration counts differ by {diff}")
    assert err <= steps * 1e-13 * kappa * mag


def test_block_sums_and_the_longdouble_forms():
    """block_sums gives block b the rows r with (r // 1024) % blocks == b; the longdouble forms of update and direction are the
    float64 ones to a rounding"""
    rng = np.random.default_rng(3)
    n, g = 5 * 1024 + 77, 2
    t = rng.integers(-9, 10, n).astype(np.float64)
    want = [t[(np.arange(n) // 1024) % g == b].sum() for b in range(g)]
    assert np.array_equal(IR.block_sums(t, g), want) and IR.block_sums(t, g, IR.LD).dtype == IR.LD
    assert np.finfo(IR.LD).eps <= 2.0 ** -63          # the extended type the GPU tests measure against
    P = IR.Par("newmark", 0.5)
    p, w, m, r, dinv, d = (rng.standard_normal(n) for _ in range(6))
    m = np.abs(m)
    lo, mag = IR.update(P, 0.3, p, w, m, r, np.float64)
    hi, _ = IR.update(P, 0.3, p, w, m, r)
    assert (np.abs(hi - lo) <= 2 * EPS * mag).all()
    d2, p2, mag = IR.direction(0.3, 0.7, r, dinv, p, d, np.float64)
    e2, q2, _ = IR.direction(0.3, 0.7, r, dinv, p, d)
    assert (np.abs(q2 - p2) <= 2 * EPS * mag).all() and (np.abs(e2 - d2) <= 2 * EPS * (np.abs(d) + 0.3 * np.abs(p))).all()
