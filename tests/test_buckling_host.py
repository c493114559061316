"""The geometric stiffness of one element on the host (pfem_elem_geometric) against the numpy mirror
(tests/buckling_reference.py: element_g), its symmetry and its error codes, and the stand-alone sanitizer program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import buckling_reference as BR
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
    if TR.geometry(kind, p, np.arange(L.NPELEM[kind])[:, None])[1][0] < 0:
        p[:, [0, 1]] = p[:, [1, 0]]
    return p


def test_geometric_stiffness_equals_the_mirror_bit_for_bit():
    """200 random elements of both kinds under random stresses.  The mirror follows the written order of elem_geometric, so every
    entry has the host's bits (a zero may differ in its sign, which array_equal does not see).  g is symmetric to rounding only:
    g_ab and g_ba are sums of the same nine (four) products in another order.  With mag = dvol max|sigma| (sum_d max_a |dN_a/dx_d|)^2,
    which bounds the sum of the magnitudes of those products, one evaluation is within (terms + 2) eps / 2 mag <= 6 eps mag of
    the exact value, so two differ by at most 12 eps mag: asserted with 16.  A row or column sum vanishes exactly (sum_b grad N_b
    = 0) and is computed from npe such entries and gradients that sum to zero within 2 eps: asserted with 64 eps mag."""
    rng = np.random.default_rng(20261021)
    worst = 0.0
    for kind in KINDS:
        npe = L.NPELEM[kind]
        conn = np.arange(npe)[:, None]
        for _ in range(200):
            p = _oriented(rng, kind)
            ed = np.array([rng.uniform(50, 500), rng.uniform(0.1, 0.4), rng.uniform(0.3, 2.0), 0.1, -0.2, 0.3])[:6 if kind == L.ELAST_TET else 5]
            sig = rng.standard_normal(L.NG[kind]) * 10.0 ** rng.uniform(-2, 2)
            g = H.GeometricStiffness(kind, *_xyz(p), ed, sig)
            gm = BR.element_g(kind, p, conn, ed[None, :], sig[:, None])[0]
            assert g.shape == (npe, npe) and np.array_equal(g, gm), (kind, g, gm)
            # symmetry and the rigid translations, against the sum of the magnitudes of the terms
            gr, _ = TR.geometry(kind, p, conn)
            mag = TR.dvol(kind, p, conn, ed[None, :])[0] * np.abs(sig).max() * sum(np.abs(np.array(d)[:, 0]).max() for d in gr) ** 2
            assert np.abs(g - g.T).max() <= 16 * EPS * mag
            assert np.abs(g.sum(0)).max() <= 64 * EPS * mag and np.abs(g.sum(1)).max() <= 64 * EPS * mag
            worst = max(worst, np.abs(g - g.T).max() / (EPS * mag))
    print(f"largest asymmetry / (eps x magnitude of the terms): {worst:.3f}")


def test_a_uniaxial_stress_on_the_unit_elements():
    """the reference tet and triangle under sigma_xx = s: g_ab = dvol s dN_a/dx dN_b/dx, by hand"""
    x, y, z = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])      # gx = (1, 0, -1, 0)
    g = H.GeometricStiffness(L.ELAST_TET, x, y, z, None, [3.0, 0, 0, 0, 0, 0])
    dvol = float(np.float32(1.0) / np.float32(6.0))
    gx = np.array([1.0, 0.0, -1.0, 0.0])
    assert np.array_equal(g, dvol * 3.0 * np.outer(gx, gx) + 0.0)
    xt, yt = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])                                                   # gy = (-1, 0, 1)
    g = H.GeometricStiffness(L.ELAST_TRIA, xt, yt, None, np.array([100.0, 0.3, 0.25]), [0.0, 2.0, 0.0])
    gy = np.array([-1.0, 0.0, 1.0])
    assert np.array_equal(g, 0.5 * 0.25 * 2.0 * np.outer(gy, gy) + 0.0)


def test_error_codes():
    x, y, z = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
    ed = np.array([100.0, 0.3, 1.0, 0.0, 0.0, 0.0])
    sg = np.ones(6)

    def code(fn):
        with pytest.raises(L.PfemError) as ei:
            fn()
        return ei.value.code

    H.GeometricStiffness(L.ELAST_TET, x, y, z, ed, sg)                       # (the element is fine)
    for kind in (L.POISSON_TRIA, L.POISSON_TET, L.POISSON_TRIA_INLINE, 0, 6, -1):
        assert code(lambda: H.GeometricStiffness(kind, x, y, z, ed, sg)) == L.ERR_ARG
    assert code(lambda: H.GeometricStiffness(L.ELAST_TET, x, y, None, ed, sg)) == L.ERR_ARG
    assert code(lambda: H.GeometricStiffness(L.ELAST_TET, x, y, z, ed, None)) == L.ERR_ARG
    assert L.lib().pfem_elem_geometric(L.ELAST_TET, x.ctypes.data, y.ctypes.data, z.ctypes.data, ed.ctypes.data, sg.ctypes.data, None) == L.ERR_ARG
    sw = [1, 0, 2, 3]
    assert code(lambda: H.GeometricStiffness(L.ELAST_TET, x[sw], y[sw], z[sw], ed, sg)) == L.ERR_NEG_JAC
    xt, yt = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    H.GeometricStiffness(L.ELAST_TRIA, xt, yt, None, ed[:5], sg[:3])
    assert code(lambda: H.GeometricStiffness(L.ELAST_TRIA, xt, yt, None, None, sg[:3])) == L.ERR_ARG          # the thickness
    assert code(lambda: H.GeometricStiffness(L.ELAST_TRIA, xt[[1, 0, 2]], yt[[1, 0, 2]], None, ed[:5], sg[:3])) == L.ERR_NEG_JAC


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_geometric_stiffness_under_asan_ubsan(tmp_path):
    """The host entry point with its shared arithmetic, compiled for the CPU with AddressSanitizer + UBSan together with a
    stand-alone program that walks both kinds on exact-size buffers (tests/native/buckling_sanitize.cpp)."""
    exe = tmp_path / "buckling_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fopenmp",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "buckling_sanitize.cpp"),
           os.path.join(ROOT, "pfemfort_amd", "csrc", "pfem_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "buckling_sanitize: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
