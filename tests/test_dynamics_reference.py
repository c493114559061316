"""The numpy mirror of the explicit dynamics (tests/dynamics_reference.py) against closed forms, so that the yardstick of the
GPU tests is itself checked: total mass, a single mode, the discrete invariant, the static limit under critical damping, the
Gershgorin step.  Mesh: the 10^3 x 6-tet Poisson box (729 free dofs; dense eigh is cheap)."""
import numpy as np
import pytest

import dynamics_reference as DR
import materials_reference as MR
from pfemfort_amd import host as H


@pytest.fixture(scope="module")
def box():
    mesh, p, m = DR.poisson_box(H, 10)
    A = DR.csr(p)
    om, phi = DR.modes(A, m)
    return {"mesh": mesh, "p": p, "m": m, "A": A, "om": om, "phi": phi, "dt": DR.gershgorin_dt(A, m)}


def test_total_mass_is_density_times_volume(box):
    """(a) sum of the nodal masses = rho |Omega|; the float Gauss weight 1/6 sets the accuracy (6e-8 relative)."""
    p = box["p"]
    _, _, mn = DR.free_dof_mass(p, 2.5)
    w = float(np.float32(1.0) / np.float32(6.0)) * 6.0
    assert mn.sum() == pytest.approx(2.5 * 8.0 * w, rel=1e-12)
    assert abs(mn.sum() - 2.5 * 8.0) < 1e-6 * 20.0
    assert box["p"].dm.size_global == 729 and (box["m"] > 0).all()


def modal_error(A, m, om, phi, dt, k, n_steps):
    """max |u_n - phi_k cos(n theta)| / max |phi_k| after n_steps from u0 = phi_k, v0 = 0, no load: cos theta = 1 - (omega dt)^2 / 2"""
    st = DR.Stepper(A, np.zeros(A.shape[0]), m, dt, u0=phi[:, k])
    st.run(n_steps)
    theta = np.arccos(1.0 - 0.5 * (om[k] * dt) ** 2)
    return np.abs(st.u - phi[:, k] * np.cos(n_steps * theta)).max() / np.abs(phi[:, k]).max()


def test_a_single_mode_keeps_its_shape_and_the_discrete_frequency(box):
    """(b) 3e-12 relative after 2000 steps when tried; the bound leaves a factor of 30 for another BLAS."""
    err = modal_error(box["A"], box["m"], box["om"], box["phi"], 0.5 * box["dt"], 3, 2000)
    print("modal error", err)
    assert err < 1e-10


def energy_spread(A, m, dt, u0, v0, n_steps):
    st = DR.Stepper(A, np.zeros(A.shape[0]), m, dt, u0=u0, v0=v0)
    h = st.run(n_steps, 1)
    e = h[:, 1] + h[:, 2]
    return (e.max() - e.min()) / abs(e).max()


def test_T_plus_S_is_the_invariant_of_the_undamped_unloaded_scheme(box):
    """(c) relative spread 1.6e-15 over 3000 steps when tried; the naive 1/2 v M v + 1/2 u K u wanders by percents."""
    rng = np.random.default_rng(5)
    N = box["A"].shape[0]
    spread = energy_spread(box["A"], box["m"], 0.9 * box["dt"], rng.standard_normal(N), rng.standard_normal(N), 3000)
    print("energy spread", spread)
    assert spread < 1e-13


def static_error(p, A, m, om, dt, n_steps):
    st = DR.Stepper(A, p.rhs, m, dt, alpha=2.0 * om[0])
    st.run(n_steps)
    x = MR.direct_solve(p)
    return np.abs(st.u - x).max() / np.abs(x).max()


def test_critical_damping_reaches_the_static_solution(box):
    """(d) alpha = 2 omega_min, dt = 0.9 x the Gershgorin step: 1.6e-9 after 100 steps, rounding level after 200 when tried."""
    e100 = static_error(box["p"], box["A"], box["m"], box["om"], 0.9 * box["dt"], 100)
    e200 = static_error(box["p"], box["A"], box["m"], box["om"], 0.9 * box["dt"], 200)
    print("static limit", e100, e200)
    assert e100 < 1e-7 and e200 < 1e-12


def test_the_gershgorin_step_is_never_above_the_critical_one(box):
    """(e) 0.90 of 2 / omega_max on this box."""
    crit = 2.0 / box["om"][-1]
    print("dt / critical", box["dt"] / crit)
    assert 0.5 * crit < box["dt"] <= crit


def test_load_curve():
    c = ([0.0, 1.0, 3.0], [0.0, 2.0, -2.0])
    assert DR.load_factor(None, 7.0) == 1.0
    assert [DR.load_factor(c, t) for t in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 9.0)] == [0.0, 0.0, 1.0, 2.0, 0.0, -2.0, -2.0]


# ---- the per-operation functions of tests/test_gpu_stepper_kernels.py, chained over steps, against Stepper ----------------------
def test_the_chained_step_kernel_is_the_stepper_bit_for_bit(box):
    """300 damped, loaded steps under a ramp: u of every step carries Stepper's bits; T, S, W from block_sums of the terms
    agree with Stepper's sums within (n + 3) eps x the sum of the terms' magnitudes (another order of an n-term sum)."""
    A, m, f = box["A"], box["m"], box["p"].rhs
    N = A.shape[0]
    rng = np.random.default_rng(17)
    dt, alpha, t0 = 0.9 * box["dt"], 0.3, 0.25
    curve = ([0.0, 100.5 * dt], [0.0, 1.0])
    st = DR.Stepper(A, f, m, dt, alpha=alpha, t0=t0, u0=rng.standard_normal(N), v0=rng.standard_normal(N), curve=curve)
    u, up = st.u.copy(), st.up.copy()
    for n in range(300):
        lam = DR.load_factor(curve, t0 + float(n) * dt)
        w = A @ u
        x, tT, tS, tW = DR.step_kernel(dt, alpha, lam, f, m, st.minv, w, u, up)
        t, T, S, W = st.step()
        assert np.array_equal(x, st.u)
        nb = -(-N // DR.BLOCK_ROWS)
        row = DR.step_row(t0, dt, n, DR.block_sums(tT, nb).sum(), DR.block_sums(tS, nb).sum(), DR.block_sums(tW, nb).sum(), x, u, [0, N - 1])
        assert row[0] == t and np.array_equal(row[4:6], x[[0, N - 1]]) and np.array_equal(row[6:], ((x - u) / dt)[[0, N - 1]])
        for got, ref, mag in zip(row[1:4], (T, S, W), st.magnitudes):          # (the magnitudes carry the rows' factors 1/2)
            assert abs(got - ref) <= (N + 3) * DR.EPS * mag
        up, u = u, x
    tl = DR.step_terms_ld(dt, x, f, m, w, up)
    assert all(abs(float(a.sum()) - b.sum()) <= (N + 3) * DR.EPS * np.abs(b).sum() for a, b in zip(tl, (tT, tS, tW)))
