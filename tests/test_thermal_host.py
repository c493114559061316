"""Thermal strains of one element on the host (pfem_elem_thermal_load, pfem_elem_post_thermal) against the numpy mirror
(tests/thermal_reference.py) and against the host's own stiffness matrices, their error codes, the argument checks of the device
entry points that come before the device is touched, and the stand-alone sanitizer program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import thermal_reference as TR
from pfemfort_amd import _lib as L
from pfemfort_amd import host as H
from test_surface_host import _random_element, _xyz

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [L.ELAST_TET, L.ELAST_TRIA]


def _oriented(rng, kind):
    """A random element with a positive Jacobian (test_surface_host's draws come in both orientations)."""
    p = _random_element(rng, kind)
    g, jac = TR.geometry(kind, p, np.arange(L.NPELEM[kind])[:, None])
    if jac[0] < 0:
        p[:, [0, 1]] = p[:, [1, 0]]
    return p


def _stiffness(kind, p, ed):
    ns = L.NPELEM[kind] * L.NDOF[kind]
    if kind == L.ELAST_TET:
        return H.StiffnessResidualElasticityLinearTetra(p[0], p[1], p[2], ed, H.TIMEDATA, np.zeros(ns))[0]
    return H.StiffnessResidualElasticityLinearTria(p[0], p[1], ed, H.TIMEDATA, np.zeros(ns))[0]


def test_thermal_load_equals_the_mirror_and_the_stiffness_times_the_free_expansion():
    """200 random elements of both kinds.  Against the mirror, which follows the written order: within 64 eps |F| entrywise,
    and expected to be the same bits (counted and printed).  Independently: B u = eps_th for u = e_th (x - x0), so
    F_th = K_e u with the K_e of the host's stiffness routine -- the claim test_post_host makes for fint, with its bound
    64 eps (|K_e| |u|).  pfem_elem_post_thermal: flux = -(sigma_th) + D B valC, fint = K_e valC - F_th within
    64 eps (|K_e| |valC| + |F_th|), grad the plain routine's bits."""
    rng = np.random.default_rng(20261020)
    exact = total = 0
    worst = {"mirror": 0.0, "K u": 0.0, "fint": 0.0}
    for kind in KINDS:
        npe, ndof = L.NPELEM[kind], L.NDOF[kind]
        conn = np.arange(npe)[:, None]
        for _ in range(200):
            p = _oriented(rng, kind)
            ed = np.array([rng.uniform(50, 500), rng.uniform(0.1, 0.4), rng.uniform(0.3, 2.0), 0.1, -0.2, 0.3])[:6 if kind == L.ELAST_TET else 5]
            alpha = rng.uniform(1e-4, 1e-2)
            theta = rng.uniform(-50, 80, npe)
            F, sg = H.ThermalLoad(kind, *_xyz(p), ed, alpha, theta)
            rows = ed[None, :]
            eth = TR.thermal_strain(kind, np.array([alpha]), theta, conn)
            Fm, sgm = TR.element_loads(kind, p, conn, rows, eth)
            assert np.all(np.abs(F - Fm[0]) <= 64 * EPS * np.abs(Fm[0])), (kind, F, Fm)
            assert np.all(np.abs(sg - sgm[:, 0]) <= 64 * EPS * np.abs(sgm[:, 0]))
            total += 1
            exact += np.array_equal(F, Fm[0]) and np.array_equal(sg, sgm[:, 0])
            K = _stiffness(kind, p, ed)
            u = (eth[0] * (p - p.mean(1, keepdims=True))).T.ravel()
            bound = 64 * EPS * (np.abs(K) @ np.abs(u))
            assert np.all(np.abs(F - K @ u) <= bound), (kind, F, K @ u, bound)
            worst["K u"] = max(worst["K u"], (np.abs(F - K @ u) / bound).max())
            # the fields under the state
            valC = rng.standard_normal(npe * ndof)
            g, f, sc, fi = H.ElementPostThermal(kind, *_xyz(p), ed, valC, alpha, theta)
            g0, f0, _, fi0 = H.ElementPost(kind, *_xyz(p), ed, valC)
            assert np.array_equal(g, g0)
            gm, fm, scm, fim = TR.element_post(kind, p, conn, rows, eth, valC.reshape(npe, ndof))
            assert np.array_equal(f, fm[:, 0]) and sc == scm[0] and np.array_equal(fi, fim[0])
            fb = 64 * EPS * (np.abs(K) @ np.abs(valC) + np.abs(F))
            assert np.all(np.abs(fi - (K @ valC - F)) <= fb)
            worst["fint"] = max(worst["fint"], (np.abs(fi - (K @ valC - F)) / fb).max())
            assert H.PostScalar(kind, f) == sc
            # a state that expands nothing: the plain routine's bits
            for a, b in zip(H.ElementPostThermal(kind, *_xyz(p), ed, valC, 0.0, theta), (g0, f0, None, fi0)):
                assert b is None or np.array_equal(a, b)
            for a, b in zip(H.ElementPostThermal(kind, *_xyz(p), ed, valC, alpha, np.zeros(npe)), (g0, f0, None, fi0)):
                assert b is None or np.array_equal(a, b)
    print(f"{exact} of {total} elements equal the mirror bit for bit; worst error / bound: {worst}")
    assert exact == total


def test_restrained_element_stress_is_minus_sigma_th_bit_for_bit():
    rng = np.random.default_rng(3)
    for kind in KINDS:
        npe, ndof = L.NPELEM[kind], L.NDOF[kind]
        for _ in range(100):
            p = _oriented(rng, kind)
            ed = np.array([rng.uniform(50, 500), rng.uniform(0.1, 0.4), rng.uniform(0.3, 2.0), 0.0, 0.0, 0.0])[:6 if kind == L.ELAST_TET else 5]
            alpha, theta = rng.uniform(1e-4, 1e-2), rng.uniform(-50, 80, npe)
            _, sg = H.ThermalLoad(kind, *_xyz(p), ed, alpha, theta)
            _, f, _, _ = H.ElementPostThermal(kind, *_xyz(p), ed, np.zeros(npe * ndof), alpha, theta)
            assert np.array_equal(f, -sg)


def test_error_codes():
    x, y, z = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
    th = np.ones(4)
    ed = np.array([100.0, 0.3, 1.0, 0.0, 0.0, 0.0])

    def code(fn):
        with pytest.raises(L.PfemError) as ei:
            fn()
        return ei.value.code

    H.ThermalLoad(L.ELAST_TET, x, y, z, ed, 1e-3, th)                       # (the element is fine)
    # a Poisson kind, a kind that does not exist
    for kind in (L.POISSON_TRIA, L.POISSON_TET, L.POISSON_TRIA_INLINE):
        assert code(lambda: H.ThermalLoad(kind, x, y, z, ed, 1e-3, th)) == L.ERR_ARG
        assert code(lambda: H.ElementPostThermal(kind, x, y, z, ed, np.zeros(12), 1e-3, th)) == L.ERR_ARG
    for kind in (0, 6, -1):
        assert L.lib().pfem_elem_thermal_load(kind, None, None, None, None, 0.0, None, None, None) == L.ERR_ARG
        assert L.lib().pfem_elem_post_thermal(kind, None, None, None, None, None, 0.0, None, None, None, None, None) == L.ERR_ARG
    # missing z / elemData / theta
    assert code(lambda: H.ThermalLoad(L.ELAST_TET, x, y, None, ed, 1e-3, th)) == L.ERR_ARG
    assert code(lambda: H.ThermalLoad(L.ELAST_TET, x, y, z, None, 1e-3, th)) == L.ERR_ARG
    assert code(lambda: H.ThermalLoad(L.ELAST_TET, x, y, z, ed, 1e-3, None)) == L.ERR_ARG
    # an inverted element
    sw = [1, 0, 2, 3]
    assert code(lambda: H.ThermalLoad(L.ELAST_TET, x[sw], y[sw], z[sw], ed, 1e-3, th)) == L.ERR_NEG_JAC
    assert code(lambda: H.ElementPostThermal(L.ELAST_TET, x[sw], y[sw], z[sw], ed, np.zeros(12), 1e-3, th)) == L.ERR_NEG_JAC
    xt, yt = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    H.ThermalLoad(L.ELAST_TRIA, xt, yt, None, ed[:5], 1e-3, th[:3])
    assert code(lambda: H.ThermalLoad(L.ELAST_TRIA, xt[[1, 0, 2]], yt[[1, 0, 2]], None, ed[:5], 1e-3, th[:3])) == L.ERR_NEG_JAC
    # any output may be NULL
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.lib().pfem_elem_thermal_load(L.ELAST_TET, p(x), p(y), p(z), p(ed), 1e-3, p(th), None, None) == L.OK


def test_device_entry_points_check_their_arguments_before_the_device():
    """What the thermal entry points refuse without looking at a handle or a device: a NULL handle, NULL arrays, n_alpha < 1."""
    lib = L.lib()
    a, th = np.array([1e-3]), np.zeros(4)
    p = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.pfem_thermal_set(None, 1, p(a), p(th)) == L.ERR_ARG
    assert lib.pfem_thermal_set_from_solver(None, 1, p(a), None, 0.0) == L.ERR_ARG
    assert lib.pfem_thermal_get(None, None, None, None) == L.ERR_ARG
    assert lib.pfem_thermal_clear(None) == L.ERR_ARG
    assert lib.pfem_rhs_add_thermal_load(None, p(a)) == L.ERR_ARG


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_thermal_load_under_asan_ubsan(tmp_path):
    """The host entry points with their shared arithmetic, compiled for the CPU with AddressSanitizer + UBSan together with a
    stand-alone program that walks both kinds on exact-size buffers (tests/native/thermal_sanitize.cpp)."""
    exe = tmp_path / "thermal_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fopenmp",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "thermal_sanitize.cpp"),
           os.path.join(ROOT, "pfemfort_amd", "csrc", "pfem_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "thermal_sanitize: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
