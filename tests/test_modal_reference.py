"""The numpy mirror of the modal analysis (tests/modal_reference.py) against the dense eigh of the same pencil
(dynamics_reference.modes), so that the yardstick of the GPU tests is itself checked -- and what pfem_modal_solve answers
without a handle, with bad parameters and without a device.

Fixtures: the 729-dof Poisson box of the golden tet10 mesh with an anisotropic conductivity, Cook's membrane (2 112 dofs,
kappa(M^-1 K) = 3.2e5) and the 576-dof beam of two materials; K from materials_reference.setup_problem, m from
dynamics_reference.free_dof_mass.  Asserted: reason 1, every residual <= tol, and the relative eigenvalue error
<= max(1e-12, tol) -- a residual of tol bounds the eigenvalue error by about tol^2 / gap, so tol itself is generous, and 1e-12
is where the rounding of the dense reference (n eps) takes over.  The iteration counts are printed and pinned where they were
measured, within a band of an eighth: rounding moves the stopping iteration, a change of scheme moves it further."""
import ctypes as C

import numpy as np
import pytest

import dynamics_reference as DR
import materials_reference as MR
import modal_reference as MO
from oracle import pfem_oracle as O
from pfemfort_amd import _lib
from pfemfort_amd import host as H

ANISO = np.array([1.3, 0.7, 2.1])
COOK_DATA = np.array([H.ELAST_ELEMDATA[0], H.ELAST_ELEMDATA[1], 0.5, 0.05, -0.02])
BEAM_TABLE = np.array([[300.0, 0.3, 1.0, 0.0, -0.1, 0.0], [900.0, 0.2, 1.0, 0.05, 0.0, 0.0]])

_FIX = {}


def fixture_of(name, golden_dir):
    """(K as CSR, m, eigenvalues, M-orthonormal eigenvectors), made once"""
    if name not in _FIX:
        if name == "tet10":
            mesh = H.read_mesh(f"{golden_dir}/input/tet10")
            p = MR.setup_problem(O.POISSON_TET, mesh, ANISO[None, :], np.zeros(mesh.nElem, np.int32))
            m = DR.free_dof_mass(p, 2.5)[0]
        elif name == "cook":
            mesh = H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
            p = MR.setup_problem(O.ELAST_TRIA, mesh, COOK_DATA[None, :], np.zeros(mesh.nElem, np.int32))
            m = DR.free_dof_mass(p, 2.5, COOK_DATA[2])[0]
        elif name == "box19k":
            mesh = H.gen_box_tets(-1, 1, 28, -0.9, 0.9, 27, -0.8, 0.8, 29)
            p = MR.setup_problem(O.POISSON_TET, mesh, ANISO[None, :], np.zeros(mesh.nElem, np.int32))
            m = DR.free_dof_mass(p, 2.5)[0]
        else:
            mesh = H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
            ids = (mesh.xyz[1][mesh.conn].mean(0) > 2.0).astype(np.int32)
            p = MR.setup_problem(O.ELAST_TET, mesh, BEAM_TABLE, ids)
            m = DR.free_dof_mass(p, np.array([3.0, 11.0])[ids])[0]
        A = DR.csr(p)
        if name == "box19k":                 # (the lowest 13 by eigsh; dense eigh is out of reach)
            _FIX[name] = (A, m) + MO.lowest_modes(A, m, 13)
        else:
            om, phi = DR.modes(A, m)
            _FIX[name] = (A, m, om ** 2, phi)
    return _FIX[name]


# (fixture, n_modes, tol) -> (block, iterations of the mirror)
CASES = [("tet10", 2, 1e-6, 4, 60), ("tet10", 6, 1e-6, 8, 62), ("tet10", 12, 1e-6, 16, 50),
         ("tet10", 2, 1e-9, 4, 86), ("tet10", 6, 1e-9, 8, 93), ("tet10", 12, 1e-9, 16, 74),
         ("beam2", 6, 1e-6, 8, 182), ("beam2", 12, 1e-6, 16, 86),
         ("cook", 6, 1e-6, 8, 1001), ("cook", 12, 1e-6, 16, 693)]


@pytest.mark.parametrize("name,n_modes,tol,block,its", CASES)
def test_the_mirror_against_dense_eigh(name, n_modes, tol, block, its, golden_dir):
    A, m, lam, phi = fixture_of(name, golden_dir)
    assert A.shape[0] == {"tet10": 729, "cook": 2112, "beam2": 576}[name]
    r = MO.lobpcg(A, m, n_modes, tol, 4 * its)
    err = MO.eig_error(r.omega2, lam)
    dist = MO.subspace_distance(r.modes, phi[:, :n_modes], m)
    print(f"{name}: MB {r.block}, tol {tol:g}: {r.iterations} iterations, {r.restarts} restarts, largest residual {r.residuals.max():.3e}, "
          f"eigenvalue error {err:.3e}, subspace distance {dist:.3e}, orthonormality {MO.orthonormality(r.modes, m):.3e}")
    assert r.block == block and r.reason == 1
    assert (r.residuals <= tol).all()
    assert err <= max(1e-12, tol)
    assert (np.diff(r.omega2) >= 0.0).all()
    # the convention of the end: M-normalised, the largest entry positive
    assert MO.orthonormality(r.modes, m) <= 64 * A.shape[0] * MO.EPS
    big = np.abs(r.modes).argmax(0)
    assert (r.modes[big, np.arange(n_modes)] > 0.0).all()
    # a residual of tol bounds the vectors by about tol / relative gap (>= 0.015 for the lowest 12 of tet10 and cook; the
    # beam's bending modes come in near-equal pairs, its subspaces are only printed)
    if name != "beam2":
        assert dist <= 10 * tol / 0.015
    # the count as measured; the band is for another BLAS's order of summation in the Gram products
    assert abs(r.iterations - its) <= max(2, its // 8)


# (n_modes, tol) -> (block, iterations of the mirror) on box19k
BOX19K = [(12, 1e-6, 16, 157), (2, 1e-6, 4, 184)]


@pytest.mark.parametrize("n_modes,tol,block,its", BOX19K)
def test_the_mirror_against_eigsh_beyond_one_grid_pass(n_modes, tol, block, its, golden_dir):
    """box19k: the 28 x 27 x 29 Poisson box, 19 656 dofs -- more rows than one pass of the device's capped grids covers
    (k_modal_gram from 8 192 rows at every MB; k_modal_update and k_modal_residual from 16 384 at MB 16), so that the yardstick
    of test_gpu_modal.py's runs there is checked too.  The reference is eigsh (shift-invert about 0) for the lowest 13; the gap
    from mode 12 to 13 (0.125 relative) makes the distance from the span of the lowest 12 well posed."""
    A, m, lam, phi = fixture_of("box19k", golden_dir)
    assert A.shape[0] == 19656 and len(lam) == 13
    gaps = np.diff(lam) / lam[:-1]
    print(f"box19k: lowest eigenvalues {lam[0]:.4f}, {lam[1]:.4f}, {lam[2]:.4f}; relative gap 12 -> 13 {gaps[11]:.3f}, smallest of the first 12 {gaps[:11].min():.3f}")
    assert gaps[11] >= 0.05
    r = MO.lobpcg(A, m, n_modes, tol, 4 * its)
    err = MO.eig_error(r.omega2, lam)
    dist = MO.subspace_distance(r.modes, phi[:, :n_modes], m)
    print(f"box19k: MB {r.block}, tol {tol:g}: {r.iterations} iterations, {r.restarts} restarts, largest residual {r.residuals.max():.3e}, "
          f"eigenvalue error {err:.3e}, subspace distance {dist:.3e}, orthonormality {MO.orthonormality(r.modes, m):.3e}")
    assert r.block == block and r.reason == 1
    assert (r.residuals <= tol).all()
    assert err <= max(1e-12, tol)
    assert (np.diff(r.omega2) >= 0.0).all()
    assert abs(r.iterations - its) <= max(2, its // 8)


def test_the_refresh_is_what_makes_cook_converge(golden_dir):
    """without the explicit K X every 10th iteration the recurrence for K X drifts: at twice the refreshed run's count the
    run without it has not converged"""
    A, m, lam, _ = fixture_of("cook", golden_dir)
    r = MO.lobpcg(A, m, 12, 1e-6, 2 * 693, refresh=10 ** 9)
    print(f"cook, MB 16, no refresh: reason {r.reason} after {r.iterations} iterations, largest residual {r.residuals.max():.3e}")
    assert r.reason == -1 and r.residuals.max() > 1e-6


def test_block_sizes_and_the_start_block():
    assert [MO.block_size(k) for k in (1, 2, 3, 6, 7, 12)] == [4, 4, 8, 8, 16, 16]
    assert MO.block_size(2, 16) == 16 and MO.block_size(6, 8) == 8
    for bad in ((0, 0), (13, 0), (6, 4), (2, 5), (12, 8)):
        with pytest.raises(ValueError):
            MO.block_size(*bad)
    with pytest.raises(ValueError):
        MO.block_size(2, 0, n=3)
    # splitmix64's published first outputs from the state 0 are the hashes of 0, gamma, 2 gamma, ...: the first is that of 0
    assert int(MO.splitmix64(0)) == 0xE220A8397B1DCDAF
    X = MO.start_block(50, 8)
    assert X.shape == (50, 8) and (X >= -1.0).all() and (X < 1.0).all() and abs(X.mean()) < 0.15
    assert X[3, 5] == (int(MO.splitmix64(3 * 8 + 5)) >> 11) * 2.0 ** -52 - 1.0
    assert np.linalg.matrix_rank(X) == 8


def test_a_given_start_equal_to_the_hash_changes_nothing(golden_dir):
    A, m, _, _ = fixture_of("tet10", golden_dir)
    a = MO.lobpcg(A, m, 2, 1e-6, 200)
    b = MO.lobpcg(A, m, 2, 1e-6, 200, x0=MO.start_block(A.shape[0], 4))
    assert a.iterations == b.iterations and np.array_equal(a.omega2, b.omega2) and np.array_equal(a.modes, b.modes)


def test_a_rank_deficient_start_is_a_breakdown(golden_dir):
    A, m, _, _ = fixture_of("tet10", golden_dir)
    x0 = MO.start_block(A.shape[0], 4)
    x0[:, 3] = x0[:, 0]
    r = MO.lobpcg(A, m, 2, 1e-6, 50, x0=x0)
    assert r.reason == -2 and r.iterations == 0


def test_jacobi_sweeps_agree_with_eigh():
    """the plain restatement of the library's Jacobi sweeps against numpy's eigh on a Gram-sized matrix"""
    rng = np.random.default_rng(3)
    G = rng.standard_normal((12, 12))
    S = G + G.T
    w, V = MO.jacobi_eigh(S)
    assert np.abs(w - np.linalg.eigvalsh(S)).max() <= 64 * 12 * MO.EPS * np.abs(w).max()
    assert np.abs(V.T @ V - np.eye(12)).max() <= 64 * 12 * MO.EPS
    assert np.abs(S @ V - V * w[None, :]).max() <= 64 * 12 * MO.EPS * np.abs(w).max()


# ---- the entry point without a handle, with bad parameters, without a device --------------------------------------------------
def _call(handle, n_modes=2, block=0, tol=1e-6, maxit=10, pc=-1, outputs=True):
    om, res = np.zeros(12), np.zeros(12)
    its, rst, why = C.c_int(7), C.c_int(7), C.c_int(7)
    rc = _lib.lib().pfem_modal_solve(handle, n_modes, block, tol, maxit, pc, None, om.ctypes.data if outputs else None, None, res.ctypes.data,
                                     C.byref(its), C.byref(rst), C.byref(why))
    return rc, its.value, rst.value, why.value


def test_the_entry_point_without_a_handle():
    assert _call(None) == (_lib.ERR_ARG, 0, 0, 0)


def test_bad_parameters_and_no_device():
    """argument errors come before the device is looked for; with good arguments a machine without a device answers
    PFEM_ERR_NOGPU, one with a device PFEM_ERR_STATE (no mesh, no mass on this handle)"""
    lib = _lib.lib()
    h = C.c_void_p()
    rc = lib.pfem_solver_create(C.byref(h), 100, 100, 0, None, None, 0)
    if rc == _lib.ERR_NOGPU:               # no handle without a device: the argument checks of the NULL handle are all there is
        assert _call(None, n_modes=0)[0] == _lib.ERR_ARG
        return
    assert rc == _lib.OK
    try:
        for kw in (dict(n_modes=0), dict(n_modes=13), dict(block=5), dict(block=32), dict(n_modes=6, block=4), dict(tol=0.0), dict(tol=-1.0),
                   dict(tol=float("inf")), dict(tol=float("nan")), dict(maxit=0), dict(pc=7), dict(pc=-2), dict(outputs=False)):
            assert _call(h, **kw)[0] == _lib.ERR_ARG, kw
        assert _call(h)[0] == _lib.ERR_STATE
    finally:
        lib.pfem_solver_destroy(h)
