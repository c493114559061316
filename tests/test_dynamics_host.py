"""pfem_elem_lumped_mass on the host (no GPU): the numpy mirror bit for bit on every element of the fixture meshes, argument
errors, and the stand-alone sanitizer walk (tests/native/dynamics_sanitize.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import dynamics_reference as DR
from pfemfort_amd import _lib as L
from pfemfort_amd import host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meshes(golden_dir):
    return {
        "tet10": (L.POISSON_TET, H.read_mesh(f"{golden_dir}/input/tet10")),
        "beam": (L.ELAST_TET, H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)),
        "tria20": (L.POISSON_TRIA, H.read_mesh(f"{golden_dir}/input/tria20x20")),
        "tria20inline": (L.POISSON_TRIA_INLINE, H.read_mesh(f"{golden_dir}/input/tria20x20")),
        "cook": (L.ELAST_TRIA, H.read_mesh(f"{golden_dir}/input/cookmembranetria32")),
    }


def _host_mass(kind, mesh, dens, thick):
    out = np.empty((L.NPELEM[kind] * L.NDOF[kind], mesh.nElem))
    for e in range(mesh.nElem):
        nd = mesh.conn[:, e]
        z = mesh.xyz[2, nd] if mesh.xyz.shape[0] == 3 else None
        ed = np.array([1.0, 0.3, thick[e], 0.0, 0.0]) if kind == L.ELAST_TRIA else None
        out[:, e] = H.MassMatrixLinear(kind, mesh.xyz[0, nd], mesh.xyz[1, nd], z, ed, dens[e])
    return out


@pytest.mark.parametrize("name", ["tet10", "beam", "tria20", "tria20inline", "cook"])
def test_lumped_mass_equals_the_mirror_bit_for_bit(name, golden_dir):
    """One density, then a two-material table (density and -- the plane-stress triangle -- thickness per element)."""
    kind, mesh = _meshes(golden_dir)[name]
    ndof = L.NDOF[kind]
    mat = (np.arange(mesh.nElem) % 3 == 1).astype(np.int64)
    for dens_tab, thick_tab in (((7.5, 7.5), (1.0, 1.0)), ((2.0, 11.0), (0.5, 1.25))):
        dens = np.array(dens_tab)[mat]
        thick = np.array(thick_tab)[mat] if kind == L.ELAST_TRIA else np.ones(mesh.nElem)
        got = _host_mass(kind, mesh, dens, thick)
        want = DR.element_lumped_mass(mesh.xyz, mesh.conn, dens, thick)
        assert np.array_equal(got, np.repeat(want, ndof, axis=0))
        # the shares add up to density x measure (the REAL(4) Gauss data: 1e-7 relative)
        w = DR.element_weights(mesh.xyz, mesh.conn, thick)
        assert np.allclose(want.sum(0), dens * w, rtol=1e-6, atol=0)


def test_argument_errors():
    x, y, z = np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
    xt, yt, zt = x, y, z                     # rows a-c, b-c, d-c of the routine's mapping: determinant +1
    x, y, z = x[[0, 1, 3, 2]], y[[0, 1, 3, 2]], z[[0, 1, 3, 2]]          # ... and -1 with two nodes swapped
    assert H.MassMatrixLinear(L.ELAST_TET, xt, yt, zt, None, 3.0).shape == (12,)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(L.PfemError) as ei:
            H.MassMatrixLinear(L.POISSON_TET, xt, yt, zt, None, bad)
        assert ei.value.code == L.ERR_ARG
    with pytest.raises(L.PfemError) as ei:
        H.MassMatrixLinear(L.POISSON_TET, xt, yt, None, None, 1.0)              # 3-D without z
    assert ei.value.code == L.ERR_ARG
    with pytest.raises(L.PfemError) as ei:
        H.MassMatrixLinear(L.ELAST_TRIA, x[:3], y[:3], None, None, 1.0)         # the triangle's thickness is in elemData
    assert ei.value.code == L.ERR_ARG
    M = np.empty(12)
    for kind in (0, 6, 7):                   # (the wrapper sizes Mlocal by the kind: the library itself)
        assert L.lib().pfem_elem_lumped_mass(kind, xt.ctypes.data, yt.ctypes.data, zt.ctypes.data, None, 1.0, M.ctypes.data) == L.ERR_ARG
    with pytest.raises(L.PfemError) as ei:
        H.MassMatrixLinear(L.POISSON_TET, x, y, z, None, 1.0)                   # inverted
    assert ei.value.code == L.ERR_NEG_JAC


def test_lumped_mass_under_address_and_ub_sanitizers(tmp_path):
    """pfem_host.cpp's pfem_elem_lumped_mass under ASan + UBSan: a stand-alone program that walks every kind on exact-size
    buffers (tests/native/dynamics_sanitize.cpp)."""
    exe = tmp_path / "dynamics_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fopenmp",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "dynamics_sanitize.cpp"),
           os.path.join(ROOT, "pfemfort_amd", "csrc", "pfem_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "dynamics_sanitize: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
