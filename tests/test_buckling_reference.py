"""The numpy mirror of the buckling analysis (tests/buckling_reference.py) against the dense scipy.linalg.eigh(K_g, K) of the same
pencil, so that the yardstick of the GPU tests is itself checked; closed forms of the geometric stiffness; and what the entry
points answer without a handle and with bad arguments.

Fixtures.  column2 / column3: the clamped 1 x 6 x 1 column (E = 300, nu = 0.3) on 2 x 12 x 2 and 3 x 12 x 3 cells, 324 and 576
dofs, under a unit end compression spread evenly over the nodes of the free end.  beam2: the 576-dof beam of two materials with
its body forces and the same end compression.  cook: Cook's membrane (2 112 dofs) under its body force and the traction
(0.5, 6.25) on the edge x = 48, as consistent nodal forces.  K and the load are materials_reference's, the reference state is
the sparse LU solve, its stresses thermal_reference.element_post's with no thermal strain.

Asserted, as test_modal_reference.py does: reason 1, every residual <= tol, |theta - theta_dense| / |theta_1| <= max(1e-12, tol)
-- a residual of tol bounds the eigenvalue error by about tol^2 / gap, and 1e-12 is where the rounding of the dense reference
takes over.  The iteration counts are printed and pinned where they were measured, within that file's band of an eighth.  T is
the point Jacobi of K for 2 modes on the columns; elsewhere the mirror is given T = splu(K).solve, the stand-in for gamg's cycle
(an approximate K^-1 is the natural preconditioner of this pencil; under Jacobi these cases need thousands of iterations)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import buckling_reference as BR
import materials_reference as MR
import thermal_reference as TR
from oracle import pfem_oracle as O
from pfemfort_amd import _lib
from pfemfort_amd import host as H

EPS = np.finfo(np.float64).eps
COLUMN = np.array([[300.0, 0.3, 1.0, 0.0, 0.0, 0.0]])
COOK_DATA = np.array([H.ELAST_ELEMDATA[0], H.ELAST_ELEMDATA[1], 0.5, 0.05, -0.02])
BEAM_TABLE = np.array([[300.0, 0.3, 1.0, 0.0, -0.1, 0.0], [900.0, 0.2, 1.0, 0.05, 0.0, 0.0]])
EULER = np.pi ** 2 * 300.0 * (1.0 / 12.0) / (4.0 * 6.0 ** 2)          # pi^2 E I / (4 L^2) of the cantilever: 1.713

_FIX = {}


def end_compression(p, total=1.0, sign=-1.0):
    """nodal forces of sum `total` along -y (sign = +1: tension), spread evenly over the nodes at y = 6, at their free y dofs"""
    top = np.nonzero(p.xyz_new[1] == 6.0)[0]
    f = np.zeros(len(p.rowptr) - 1)
    f[p.dm.NodeDofArrayNew[top, 1]] = sign * total / len(top)
    return f


def cook_traction(p, traction=(0.5, 6.25), thick=0.5):
    """consistent nodal forces of a uniform traction on the edges at x = 48: thick * length / 2 * traction at either node"""
    x, y = p.xyz_new[0], p.xyz_new[1]
    f = np.zeros(len(p.rowptr) - 1)
    nda = p.dm.NodeDofArrayNew
    for a, b in ((0, 1), (1, 2), (2, 0)):
        na, nb = p.conn_new[a], p.conn_new[b]
        on = (x[na] == 48.0) & (x[nb] == 48.0)
        for n0, n1 in zip(na[on], nb[on]):
            w = thick * abs(y[n1] - y[n0]) / 2.0
            for node in (n0, n1):
                for d in range(2):
                    if nda[node, d] >= 0:
                        f[nda[node, d]] += w * traction[d]
    assert f.any()
    return f


def build(kind, mesh, table, ids, load):
    """the fixture of one mesh: K, the reference state of K u = rhs + load(p), its stresses, K_g in ascending element order"""
    p = MR.setup_problem(kind, mesh, table, ids)
    N = len(p.rowptr) - 1
    K = sp.csr_matrix((p.vals, p.cols, p.rowptr), shape=(N, N))
    f = p.rhs + load(p)
    u = spl.splu(K.tocsc()).solve(f)
    rows = TR.rows_of(table, mesh.nElem, ids)
    full = MR.full_field(p, u)
    sig = TR.element_post(kind, p.xyz_new, p.conn_new, rows, 0.0, full)[1]
    g = BR.element_g(kind, p.xyz_new, p.conn_new, rows, sig)
    vals, sabs, count = BR.assemble(g, p.edof, O.NDOF[kind], p.rowptr, p.cols)
    Kg = sp.csr_matrix((vals, p.cols, p.rowptr), shape=(N, N))
    return dict(p=p, K=K, Kg=Kg, f=f, u=u, sig=sig, g=g, rows=rows, sabs=sabs, count=count)


def fixture_of(name, golden_dir):
    if name not in _FIX:
        if name in ("column2", "column3"):
            nc = int(name[-1])
            mesh = H.gen_box_tets(-0.5, 0.5, nc, 0.0, 6.0, 12, -0.5, 0.5, nc, bc_mode=1, ndof=3)
            F = build(O.ELAST_TET, mesh, COLUMN, np.zeros(mesh.nElem, np.int32), end_compression)
        elif name == "beam2":
            mesh = H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
            ids = (mesh.xyz[1][mesh.conn].mean(0) > 2.0).astype(np.int32)
            F = build(O.ELAST_TET, mesh, BEAM_TABLE, ids, end_compression)
        else:
            mesh = H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
            F = build(O.ELAST_TRIA, mesh, COOK_DATA[None, :], np.zeros(mesh.nElem, np.int32), cook_traction)
        F["dense"] = BR.dense_pairs(F["Kg"], F["K"])[0]
        F["lu"] = spl.splu(F["K"].tocsc())
        _FIX[name] = F
    return _FIX[name]


# (fixture, n_modes, T, dofs) -> (block, iterations of the mirror)
CASES = [("column2", 2, "jacobi", 324, 4, 519), ("column3", 2, "jacobi", 576, 4, 1376), ("column3", 6, "lu", 576, 8, 13),
         ("beam2", 2, "jacobi", 576, 4, 795), ("beam2", 6, "lu", 576, 8, 14), ("cook", 6, "lu", 2112, 8, 44)]
TOL = 1e-6


@pytest.mark.parametrize("name,n_modes,pc,dofs,block,its", CASES)
def test_the_mirror_against_dense_eigh(name, n_modes, pc, dofs, block, its, golden_dir):
    F = fixture_of(name, golden_dir)
    assert F["K"].shape[0] == dofs
    T = None if pc == "jacobi" else F["lu"].solve
    r = BR.lobpcg(F["Kg"], F["K"], n_modes, TOL, 4 * its, T=T)
    err = BR.theta_error(r.theta, F["dense"])
    print(f"{name}: MB {r.block}, T {pc}: {r.iterations} iterations, {r.restarts} restarts, largest residual {r.residuals.max():.3e}, "
          f"theta error {err:.3e}, theta_1 {r.theta[0]:.6e}, lowest factor {r.factors[0]:.6f}")
    assert r.block == block and r.reason == 1
    assert (r.residuals <= TOL).all()
    assert err <= max(1e-12, TOL)
    assert (np.diff(r.theta) >= 0.0).all()
    assert np.array_equal(r.factors, BR.factors(r.theta))
    # the convention of the end: phi^T K phi = 1, the largest entry positive
    assert np.abs((r.modes * (F["K"] @ r.modes)).sum(0) - 1.0).max() <= 64 * dofs * EPS
    big = np.abs(r.modes).argmax(0)
    assert (r.modes[big, np.arange(n_modes)] > 0.0).all()
    # the count as measured; the band is for another BLAS's order of summation in the Gram products
    assert abs(r.iterations - its) <= max(2, its // 8)


# ---- closed forms --------------------------------------------------------------------------------------------------------------
def _free_mesh(kind, golden_dir):
    """(xyz, conn, elemData rows) of a mesh in its own numbering, no dof constrained: a box of tets, Cook's triangles"""
    if kind == O.ELAST_TET:
        mesh = H.gen_box_tets(-0.5, 0.7, 3, 0.0, 1.1, 2, -0.3, 0.5, 2, bc_mode=1, ndof=3)
        return mesh.xyz, mesh.conn, np.broadcast_to(COLUMN[0], (mesh.nElem, 6))
    mesh = H.read_mesh(f"{golden_dir}/input/cookmembranetria32")
    return mesh.xyz[:2], mesh.conn, np.broadcast_to(COOK_DATA, (mesh.nElem, 5))


@pytest.mark.parametrize("kind", [O.ELAST_TET, O.ELAST_TRIA])
def test_rigid_translations_and_linear_fields(kind, golden_dir):
    """On the unconstrained mesh with one uniform stress: the row sums of every element's g vanish to rounding (K_g annihilates
    rigid translations: sum_b grad N_b = 0), and for a linear field phi_k = c_k + G_k . x the energy is exact,
    phi^T K_g phi = volume x sum_k G_k . sigma G_k -- the gradient of a linear field is reproduced by linear elements."""
    xyz, conn, rows = _free_mesh(kind, golden_dir)
    nd = 3 if kind == O.ELAST_TET else 2
    rng = np.random.default_rng(7)
    voigt = rng.standard_normal(6 if nd == 3 else 3)
    sig = np.broadcast_to(voigt[:, None], (len(voigt), conn.shape[1]))
    g = BR.element_g(kind, xyz, conn, rows, sig)
    scale = np.abs(g).sum(2)
    assert (np.abs(g.sum(2)) <= 8 * EPS * scale).all() and (np.abs(g.sum(1)) <= 8 * EPS * np.abs(g).sum(1)).all()
    assert np.abs(g - g.transpose(0, 2, 1)).max() <= 16 * EPS * np.abs(g).max()
    S = np.array([[voigt[0], voigt[3], voigt[5]], [voigt[3], voigt[1], voigt[4]], [voigt[5], voigt[4], voigt[2]]]) if nd == 3 else \
        np.array([[voigt[0], voigt[2]], [voigt[2], voigt[1]]])
    G = rng.standard_normal((nd, nd))                        # G[k] = grad phi_k
    phi = rng.standard_normal(nd)[None, :] + xyz.T @ G.T      # (nNode, component k)
    pe = phi[conn]                                            # [a, e, k]
    energy = np.einsum("aek,eab,bek->", pe, g, pe)
    volume = TR.dvol(kind, xyz, conn, rows).sum()
    want = volume * sum(G[k] @ S @ G[k] for k in range(nd))
    print(f"kind {kind}: energy of a linear field {energy:.12e}, closed form {want:.12e}")
    # every g_ab is within 6 eps of its exact value (at most nine products and their sums), the triple products add 3 eps and
    # the sum over the elements its own share: 16 eps x the sum of the magnitudes, which is what cancels when phi is large
    bound = 16 * EPS * np.einsum("aek,eab,bek->", np.abs(pe), np.abs(g), np.abs(pe))
    print(f"    |difference| {abs(energy - want):.3e}, bound {bound:.3e}")
    assert abs(energy - want) <= bound and bound <= 1e-8 * abs(want)


def test_reversing_the_load_flips_theta(golden_dir):
    F = fixture_of("column2", golden_dir)
    p = F["p"]
    K = F["K"]
    u = F["lu"].solve(p.rhs + end_compression(p, sign=+1.0))
    sig = TR.element_post(O.ELAST_TET, p.xyz_new, p.conn_new, F["rows"], 0.0, MR.full_field(p, u))[1]
    assert np.array_equal(sig, -F["sig"])                     # (no body force: the state is odd in the load)
    g = BR.element_g(O.ELAST_TET, p.xyz_new, p.conn_new, F["rows"], sig)
    vals = BR.assemble(g, p.edof, 3, p.rowptr, p.cols)[0]
    assert np.array_equal(vals, -F["Kg"].data)
    dense = BR.dense_pairs(sp.csr_matrix((vals, p.cols, p.rowptr), shape=K.shape), K)[0]
    assert np.abs(dense + F["dense"][::-1]).max() <= 1e-12 * np.abs(dense).max()
    # in tension the lowest pairs are the compressed column's highest with the sign changed: the column's own buckling modes now
    # sit at the top of the spectrum
    assert dense[-1] == pytest.approx(-F["dense"][0], rel=1e-12)


def test_the_lowest_factor_falls_towards_euler(golden_dir):
    """linear tets lock in bending: the factor comes down from above under refinement and stays above pi^2 E I / (4 L^2)"""
    lam = [BR.factors(fixture_of(n, golden_dir)["dense"][:1])[0] for n in ("column2", "column3")]
    print(f"lowest load factor: {lam[0]:.4f} on 324 dofs, {lam[1]:.4f} on 576 dofs; Euler {EULER:.4f}")
    assert lam[0] > lam[1] > EULER
    assert fixture_of("column2", golden_dir)["dense"][0] < 0.0


def test_factors_of_theta():
    assert np.array_equal(BR.factors([-0.5, -0.25, 0.0, 2.0]), [2.0, 4.0, np.inf, np.inf])


# ---- the entry points without a handle, with bad parameters, without a device ------------------------------------------------
def _solve(handle, n_modes=2, block=0, tol=1e-6, maxit=10, pc=-1, outputs=True):
    th, fac, res = np.zeros(12), np.zeros(12), np.zeros(12)
    its, rst, why = C.c_int(7), C.c_int(7), C.c_int(7)
    rc = _lib.lib().pfem_buckling_solve(handle, n_modes, block, tol, maxit, pc, None, th.ctypes.data if outputs else None, fac.ctypes.data, None,
                                        res.ctypes.data, C.byref(its), C.byref(rst), C.byref(why))
    return rc, its.value, rst.value, why.value


def test_the_entry_points_without_a_handle():
    lib = _lib.lib()
    v = np.zeros(16)
    p = v.ctypes.data
    assert _solve(None) == (_lib.ERR_ARG, 0, 0, 0)
    assert lib.pfem_buckling_setup(None, p, None, None) == _lib.ERR_ARG
    assert lib.pfem_buckling_get_geometric(None, p) == _lib.ERR_ARG
    assert lib.pfem_buckling_last_pc(None, p) == _lib.ERR_ARG
    assert lib.pfem_buck_probe_gram(None, 4, 1, *([p] * 10)) == _lib.ERR_ARG
    assert lib.pfem_buck_probe_residual(None, 4, 1, p, p, None, p, p, p) == _lib.ERR_ARG
    assert lib.pfem_buck_probe_update(None, 4, 1, *([p] * 10)) == _lib.ERR_ARG


def test_bad_parameters_and_no_device():
    """argument errors come before the device is looked for; with good arguments a machine without a device answers
    PFEM_ERR_NOGPU, one with a device PFEM_ERR_STATE (no set-up on this handle)"""
    lib = _lib.lib()
    h = C.c_void_p()
    rc = lib.pfem_solver_create(C.byref(h), 100, 100, 0, None, None, 0)
    if rc == _lib.ERR_NOGPU:               # no handle without a device: the argument checks of the NULL handle are all there is
        assert _solve(None, n_modes=0)[0] == _lib.ERR_ARG
        return
    assert rc == _lib.OK
    try:
        for kw in (dict(n_modes=0), dict(n_modes=13), dict(block=5), dict(block=32), dict(n_modes=6, block=4), dict(tol=0.0), dict(tol=-1.0),
                   dict(tol=float("inf")), dict(tol=float("nan")), dict(maxit=0), dict(pc=7), dict(pc=-2), dict(outputs=False)):
            assert _solve(h, **kw)[0] == _lib.ERR_ARG, kw
        assert _solve(h)[0] == _lib.ERR_STATE
        assert lib.pfem_buckling_setup(h, np.zeros(6).ctypes.data, None, None) == _lib.ERR_STATE      # no mesh
        assert lib.pfem_buckling_get_geometric(h, np.zeros(6).ctypes.data) == _lib.ERR_STATE
    finally:
        lib.pfem_solver_destroy(h)
