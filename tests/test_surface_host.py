"""One side of one element on the host (pfem_face_load) against the numpy mirror (tests/surface_reference.py), against an
independent evaluation (P1 mass matrix of the side, numpy's own norm), against geometric identities, and on the reference's
Cook's-membrane input, whose ForceBC file is a uniform traction on the edge x = 48 integrated by hand."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surface_reference as SR
from pfemfort_amd import _lib as L
from pfemfort_amd import host as H

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [L.POISSON_TRIA, L.POISSON_TET, L.ELAST_TET, L.POISSON_TRIA_INLINE, L.ELAST_TRIA]
LOADS = {L.POISSON_TRIA: [L.LOAD_FLUX], L.POISSON_TET: [L.LOAD_FLUX], L.POISSON_TRIA_INLINE: [L.LOAD_FLUX],
         L.ELAST_TET: [L.LOAD_TRACTION, L.LOAD_PRESSURE], L.ELAST_TRIA: [L.LOAD_TRACTION, L.LOAD_PRESSURE]}


def _random_element(rng, kind):
    """A non-degenerate element of either orientation: a reference simplex under a random affine map with |det| >= 0.05."""
    npe, ndim = L.NPELEM[kind], L.NDIM[kind]
    while True:
        A = rng.standard_normal((ndim, ndim))
        if abs(np.linalg.det(A)) >= 0.05:
            break
    ref = np.vstack([np.zeros(ndim), np.eye(ndim)])                       # (npe, ndim)
    pts = ref[rng.permutation(npe)] @ A.T + rng.uniform(-2, 2, ndim)
    return pts.T.copy()                                                   # (ndim, npe)


def _xyz(p):
    return p[0], p[1], (p[2] if p.shape[0] == 3 else None)


def test_face_load_equals_the_mirror_and_an_independent_evaluation():
    """pfem_face_load on 200 random elements of every kind (both orientations), all sides, all loads that fit.

    The bound.  u = eps/2 is the unit roundoff.  A cross-product component is c = p - q with p, q products of coordinate
    differences: the two differences carry u each, the product u, the subtraction u of |c| <= |p| + |q|, so
    |dc_i| <= 4u (|p| + |q|) = 2 eps a_i.  len = |c|_2 adds its own 3u len, hence |d len| <= 2 eps |a|_2 + 1.5 eps len
    <= 3.5 eps |a|_2, and with mabs = measure evaluated on the a_i (surface_reference.geometry) |d measure| <= 3.5 eps mabs on
    each side of a comparison: 8 eps mabs between two evaluations.  A normal component n_i = c_i / len moves by at most
    (2 eps a_i + 3.5 eps |a|_2 + 0.5 eps len) / len <= 6 eps mabs / measure per evaluation: 16 eps mabs / measure between two.
    F_a = (m (2 g_a + g_b + g_c)) / div: the bracket carries 2u of its absolute sum, product and quotient u each, m its
    3.5 eps mabs; with T_a = mabs (2|g_a| + |g_b| + |g_c|) / div (the mirror's T, thickness included) that is
    <= 5.5 eps T_a per evaluation, 16 eps T_a between two (the mass-matrix form has two more additions).  A pressure first
    forms g = -p n: the normal's 16 eps mabs / measure multiplies |p|, so its bound is 16 eps (1 + mabs / measure) T_a.
    The mirror follows the written order, so against it the difference is expected to be zero; the independent evaluation
    uses the bound in earnest."""
    rng = np.random.default_rng(20261019)
    worst = {"mirror": 0.0, "indep F": 0.0, "indep measure": 0.0, "indep normal": 0.0}
    exact = total = 0
    for kind in KINDS:
        npe, ndof, ndim = L.NPELEM[kind], L.NDOF[kind], L.NDIM[kind]
        ns = npe - 1
        for _ in range(200):
            p = _random_element(rng, kind)
            thick = rng.uniform(0.3, 2.0)
            ed = np.array([100.0, 0.3, thick, 0.0, 0.0])
            for side in range(npe):
                for load in LOADS[kind]:
                    ncomp = SR.load_components(kind, load)
                    vals = rng.standard_normal((ns, ncomp))
                    F, meas, nrm = H.FaceLoad(kind, *_xyz(p), side, load, vals, ed if kind == L.ELAST_TRIA else None)
                    th = thick if kind == L.ELAST_TRIA else 1.0
                    Fm, mm, nm, T, mabs = SR.face_load(kind, *_xyz(p), side, load, vals, th)
                    cond = mabs / mm
                    fb = 16 * EPS * T * ((1 + cond) if load == L.LOAD_PRESSURE else 1.0)
                    assert np.all(np.abs(F - Fm) <= fb), (kind, side, load, F, Fm)
                    assert abs(meas - mm) <= 8 * EPS * mabs and np.all(np.abs(nrm - nm) <= 16 * EPS * cond)
                    total += 1
                    exact += np.array_equal(F, Fm) and meas == mm and np.array_equal(nrm, nm)
                    worst["mirror"] = max(worst["mirror"], (np.abs(F - Fm) / np.where(fb > 0, fb, 1)).max())
                    # independent: numpy's norm, the outward normal from the centroid, the side's P1 mass matrix
                    sn = [a for a in range(npe) if a != side]
                    q = p[:, sn]
                    if ndim == 3:
                        c = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
                        mi = 0.5 * np.linalg.norm(c)
                    else:
                        t = q[:, 1] - q[:, 0]
                        c = np.array([t[1], -t[0]])
                        mi = np.linalg.norm(t)
                    ni = c / np.linalg.norm(c)
                    if ni @ (q.mean(1) - p.mean(1)) < 0:
                        ni = -ni
                    M = (np.ones((ns, ns)) + np.eye(ns)) * (mi * th / (12.0 if ndim == 3 else 6.0))
                    g = -vals[:, :1] * ni[None, :] if load == L.LOAD_PRESSURE else vals
                    Fi = np.zeros(npe * ndof)
                    Fi.reshape(npe, ndof)[sn] = M @ g
                    assert np.all(np.abs(F - Fi) <= fb), (kind, side, load, F, Fi, fb)
                    assert abs(meas - mi) <= 8 * EPS * mabs and np.all(np.abs(nrm - ni) <= 16 * EPS * cond)
                    assert np.all(F.reshape(npe, ndof)[side] == 0.0)
                    worst["indep F"] = max(worst["indep F"], (np.abs(F - Fi) / np.where(fb > 0, fb, 1)).max())
                    worst["indep measure"] = max(worst["indep measure"], abs(meas - mi) / (8 * EPS * mabs))
                    worst["indep normal"] = max(worst["indep normal"], (np.abs(nrm - ni) / (16 * EPS * cond)).max())
    print(f"{exact} of {total} sides equal the mirror bit for bit; worst error / bound: {worst}")


def test_normals_are_outward_for_both_orientations_and_close_the_element():
    """The normal points away from the opposite node whatever the order of the nodes: for an element and for the same element
    with two nodes swapped (inverted), n . (side centroid - opposite node) > 0 on every side, and the swapped element's sides
    have the same measure and normal.  sum_sides measure normal = 0 for a closed element: each term carries the 8 eps mabs of
    its measure and the 16 eps mabs / measure of its normal, so the sum stays below 24 eps sum_sides mabs."""
    rng = np.random.default_rng(7)
    for kind in (L.POISSON_TRIA, L.POISSON_TET):
        npe, ndim = L.NPELEM[kind], L.NDIM[kind]
        for _ in range(200):
            p = _random_element(rng, kind)
            swapped = p[:, [1, 0] + list(range(2, npe))]
            tot = np.zeros(ndim); tot_abs = 0.0
            for side in range(npe):
                _, meas, nrm = H.FaceLoad(kind, *_xyz(p), side)
                sn = [a for a in range(npe) if a != side]
                assert nrm @ (p[:, sn].mean(1) - p[:, side]) > 0 and meas > 0
                assert abs(np.linalg.norm(nrm) - 1.0) <= 4 * EPS
                s2 = {0: 1, 1: 0}.get(side, side)                         # the same geometric side of the swapped element
                _, meas2, nrm2 = H.FaceLoad(kind, *_xyz(swapped), s2)
                mabs = SR.face_load(kind, *_xyz(p), side, L.LOAD_FLUX, np.zeros(npe - 1))[4]
                assert abs(meas2 - meas) <= 8 * EPS * mabs and np.all(np.abs(nrm2 - nrm) <= 16 * EPS * mabs / meas)
                tot += meas * nrm
                tot_abs += mabs
            assert np.all(np.abs(tot) <= 24 * EPS * tot_abs), (tot, tot_abs)


def test_nodal_loads_sum_to_the_integral_of_the_linear_field():
    """sum_a F_a = measure (thick) mean(g): the integral of the linear interpolant over the side.  Every F_a is within
    5.5 eps T_a of its exact value (see above) and the sums add (ns - 1) u each: 8 eps sum_a T_a."""
    rng = np.random.default_rng(8)
    for kind in KINDS:
        npe, ndof = L.NPELEM[kind], L.NDOF[kind]
        ns = npe - 1
        for _ in range(100):
            p = _random_element(rng, kind)
            thick = rng.uniform(0.3, 2.0)
            ed = np.array([100.0, 0.3, thick, 0.0, 0.0])
            th = thick if kind == L.ELAST_TRIA else 1.0
            for side in range(npe):
                for load in LOADS[kind]:
                    ncomp = SR.load_components(kind, load)
                    vals = rng.standard_normal((ns, ncomp))
                    F, meas, nrm = H.FaceLoad(kind, *_xyz(p), side, load, vals, ed if kind == L.ELAST_TRIA else None)
                    T = SR.face_load(kind, *_xyz(p), side, load, vals, th)[3]
                    g = -vals[:, :1] * nrm[None, :] if load == L.LOAD_PRESSURE else vals
                    want = meas * th * g.mean(0)
                    got = F.reshape(npe, ndof).sum(0)
                    assert np.all(np.abs(got - want) <= 8 * EPS * T.reshape(npe, ndof).sum(0)), (kind, side, load, got, want)


def test_error_codes():
    x, y, z = np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])

    def code(fn):
        with pytest.raises(L.PfemError) as ei:
            fn()
        return ei.value.code

    one = np.ones(9)
    ed = np.array([1.0, 0.3, 1.0, 0.0, 0.0])
    # a load that does not fit the element kind
    for kind in (L.POISSON_TRIA, L.POISSON_TRIA_INLINE):
        for load in (L.LOAD_TRACTION, L.LOAD_PRESSURE, 0, 4):
            assert code(lambda: H.FaceLoad(kind, x[:3], y[:3], None, 0, load, one)) == L.ERR_ARG
    for load in (L.LOAD_TRACTION, L.LOAD_PRESSURE, 0, 4):
        assert code(lambda: H.FaceLoad(L.POISSON_TET, x, y, z, 0, load, one)) == L.ERR_ARG
    for load in (L.LOAD_FLUX, 0, 4):
        assert code(lambda: H.FaceLoad(L.ELAST_TET, x, y, z, 0, load, one)) == L.ERR_ARG
        assert code(lambda: H.FaceLoad(L.ELAST_TRIA, x[:3], y[:3], None, 0, load, one, ed)) == L.ERR_ARG
    # side out of range, bad kind, missing z / values / thickness
    assert code(lambda: H.FaceLoad(L.POISSON_TET, x, y, z, 4)) == L.ERR_ARG
    assert code(lambda: H.FaceLoad(L.POISSON_TET, x, y, z, -1)) == L.ERR_ARG
    assert code(lambda: H.FaceLoad(L.POISSON_TRIA, x[:3], y[:3], None, 3)) == L.ERR_ARG
    assert code(lambda: H.FaceLoad(L.POISSON_TET, x, y, None, 0)) == L.ERR_ARG
    assert code(lambda: H.FaceLoad(L.POISSON_TET, x, y, z, 0, L.LOAD_FLUX, None)) == L.ERR_ARG
    assert code(lambda: H.FaceLoad(L.ELAST_TRIA, x[:3], y[:3], None, 0, L.LOAD_PRESSURE, one, None)) == L.ERR_ARG
    assert L.lib().pfem_face_load(0, None, None, None, 0, 0, None, None, None, None, None) == L.ERR_ARG
    assert L.lib().pfem_face_load(6, None, None, None, 0, 0, None, None, None, None, None) == L.ERR_ARG
    # a side of zero measure (two of its nodes coincide), and a flat element whose sides have no outside
    xd = x.copy(); yd = y.copy(); zd = z.copy()
    xd[2], yd[2], zd[2] = xd[1], yd[1], zd[1]
    assert code(lambda: H.FaceLoad(L.POISSON_TET, xd, yd, zd, 0)) == L.ERR_NEG_JAC
    assert code(lambda: H.FaceLoad(L.POISSON_TRIA, xd[:3], yd[:3], None, 0)) == L.ERR_NEG_JAC
    assert code(lambda: H.FaceLoad(L.POISSON_TRIA, np.array([0.0, 1.0, 2.0]), np.zeros(3), None, 0)) == L.ERR_NEG_JAC
    # the other sides of an element with one degenerate side are fine, and elemData is not needed off the plane-stress triangle
    F, meas, nrm = H.FaceLoad(L.ELAST_TET, x, y, z, 3, L.LOAD_PRESSURE, np.ones(3))
    assert meas == 0.5 and np.array_equal(nrm, [0.0, 0.0, -1.0]) and np.array_equal(F.reshape(4, 3)[3], np.zeros(3))


def test_cook_membrane_traction_is_the_reference_force_file(golden_dir):
    """cookmembranetria32: the mirror's boundary has 128 edges, 32 of them on x = 48; a uniform traction (0, 6.25) at unit
    thickness, integrated edge by edge with pfem_face_load and summed per node, is the committed ForceBC file bit for bit
    (33 forces of 3.125 and 1.5625, 100 in all): every edge is 0.5 long, 0.5 * 18.75 is exact and 9.375 / 6 is 1.5625 exactly,
    and a node adds at most two equal terms."""
    mesh = H.read_mesh(os.path.join(golden_dir, "input", "cookmembranetria32"))
    be, bs = SR.boundary_sides(mesh.conn)
    assert len(be) == 128
    _, _, nodes, _ = SR.geometry(mesh.xyz, mesh.conn, be, bs)
    on = np.all(mesh.xyz[0][nodes] == 48.0, axis=0)
    assert on.sum() == 32
    ed = H.ELAST2D_ELEMDATA
    assert ed[2] == 1.0
    f = np.zeros((mesh.nNode, 2))
    for e, s in zip(be[on], bs[on]):
        nd = mesh.conn[:, e]
        F, meas, nrm = H.FaceLoad(L.ELAST_TRIA, mesh.xyz[0, nd], mesh.xyz[1, nd], None, s, L.LOAD_TRACTION, [[0.0, 6.25], [0.0, 6.25]], ed)
        assert meas == 0.5 and np.array_equal(nrm, [1.0, 0.0])
        f[nd] += F.reshape(3, 2)
    # the mirror's vectorised form gives the same nodal forces
    Fs, _ = SR.consistent_loads(L.ELAST_TRIA, L.LOAD_TRACTION, *SR.geometry(mesh.xyz, mesh.conn, be[on], bs[on])[:2],
                                np.broadcast_to([0.0, 6.25], (32, 2, 2)).copy(), 1.0)
    fm = np.zeros_like(f)
    np.add.at(fm, nodes[:, on].T, Fs)
    assert np.array_equal(f, fm)
    want = np.zeros_like(f)
    assert len(mesh.force_node) == 33
    want[mesh.force_node, mesh.force_dof] = mesh.force_val
    assert np.array_equal(f, want)
    assert f.sum() == 100.0 and set(np.unique(f[f != 0])) == {3.125, 1.5625}


def test_plane_stress_uniaxial_state_balances_the_edge_traction():
    """The 2-D closed form of tests/test_gpu_surface.py, checked without a solver: on a jiggled triangle mesh of [0,2] x [0,1],
    plane stress, thickness 0.5, the field u = (t x / E, -nu t y / E) is shear-free, so the reference's D(3,3) = b1 (1 - nu)
    does not enter, and sum_e K_e u_e equals the mirror's load vector of the traction (t, 0) on x = 2 at every dof that is free
    under the rollers u_x(x = 0) = u_y(y = 0) = 0.  K_e from host.StiffnessResidualElasticityLinearTria.  Tolerance: the
    entries of K u are sums of products E thick grad grad u ~ 50 * 0.4, a dozen per node: 1e-12 absolute is 1e4 roundings."""
    E, nu, thick, t = 50.0, 0.3, 0.5, 2.0
    xyz, conn = SR.tria_strip(4, 3, 2.0, 1.0)
    ed = np.array([E, nu, thick, 0.0, 0.0])
    u = np.stack([t * xyz[0] / E, -nu * t * xyz[1] / E], axis=1)            # (nNode, 2)
    fint = np.zeros_like(u)
    for e in range(conn.shape[1]):
        nd = conn[:, e]
        K, F = H.StiffnessResidualElasticityLinearTria(xyz[0, nd], xyz[1, nd], ed, H.TIMEDATA, np.zeros(6))
        assert np.all(F == 0.0)
        fint[nd] += (K @ u[nd].ravel()).reshape(3, 2)
    be, bs = SR.boundary_sides(conn)
    nodes = SR.geometry(xyz, conn, be, bs)[2]
    on = np.all(xyz[0][nodes] == 2.0, axis=0)
    assert on.sum() == 3
    edof = (2 * conn[np.repeat(np.arange(3), 2)] + np.tile(np.arange(2), 3)[:, None]).astype(np.int32)   # every dof free
    b, _ = SR.load_vector(L.ELAST_TRIA, xyz, conn, edof, 2 * xyz.shape[1], be[on], bs[on], L.LOAD_TRACTION, [t, 0.0], SR.UNIFORM, thick)
    free = np.ones_like(u, bool)
    free[xyz[0] == 0.0, 0] = False
    free[xyz[1] == 0.0, 1] = False
    assert abs(b.sum() - t * thick * 1.0) <= 1e-14
    assert np.abs(fint - b.reshape(-1, 2))[free].max() <= 1e-12
    assert np.abs(fint[~free]).max() > 1e-3                                  # the rollers do carry reactions


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_face_load_under_asan_ubsan(tmp_path):
    """The host entry point with its shared arithmetic, compiled for the CPU with AddressSanitizer + UBSan together with a
    stand-alone program that walks every kind, side and load on exact-size buffers (tests/native/surface_sanitize.cpp)."""
    exe = tmp_path / "surface_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fopenmp",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "surface_sanitize.cpp"),
           os.path.join(ROOT, "pfemfort_amd", "csrc", "pfem_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "surface_sanitize: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
