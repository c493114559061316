"""The references of tests/amg_reference.py checked against the oracle on the CPU, and what they can see.

Synthetic 7-point Laplacians with 2 x 2 x 2 bricks (11^3 rows: 1331 -> 216 -> 27; 27^3 rows: 19683 -> 2744 -> 343 -> 64) and a
small clamped beam with ``oracle.rbm_prolongator`` on node bricks (243 -> 120 -> 18 rows; the thin bricks at the beam's edge are
lines of nodes, whose rotation dofs are idle).

* ``cycle_ld`` agrees with ``oracle.amg_cycle`` to the rounding level of fp64 (e64 <= 64 eps), over V and W, the degrees, a last
  level above the dense limit, and explicit prolongators.
* Sensitivity: every mutation test_gpu_amg_pieces.py exists to catch, applied to the fp64 evaluation, moves z by more than that
  file's tolerance of one application (32 x e64, at least 64 eps) -- with ONE exception that no vector can see and that the
  comparison of the coarse operators catches instead: the diagonal of an idle rotation dof (see the test).
"""
import functools

import numpy as np
import scipy.sparse as sp

import amg_reference as R
from oracle import pfem_oracle as O

EPS = R.EPS


def _laplacian(n):
    one = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    eye = sp.identity(n)
    return (sp.kron(sp.kron(one, eye), eye) + sp.kron(sp.kron(eye, one), eye) + sp.kron(sp.kron(eye, eye), one)).tocsr()


def _bricks(n):
    """2 x 2 x 2 bricks of an n^3 lattice, level after level down to at most 128 rows"""
    out = []
    while n ** 3 > 128:
        nc = (n + 1) // 2
        i = np.arange(n) // 2
        out.append((i[:, None, None] * nc * nc + i[None, :, None] * nc + i[None, None, :]).ravel())
        n = nc
    return out


@functools.lru_cache(maxsize=None)
def _lap_case(n):
    return _laplacian(n), _bricks(n)


@functools.lru_cache(maxsize=None)
def _beam_case():
    """3 x 9 x 3 free nodes of 3 dofs; node bricks of 2 (the last one of a line of 3 alone): 2 x 5 x 2 aggregates, some of them
    lines or single nodes (idle rotations); then bricks of 2 x 2 x 2 coarse nodes with the fifth joined: 1 x 3 x 1."""
    mesh = O.gen_box_tets(-0.5, 0.5, 2, 0.0, 4.5, 9, -0.5, 0.5, 2, bc_mode=1, ndof=3)
    prob = O.setup_problem(O.ELAST_TET, mesh)
    nd = prob.dm.NodeDofArrayNew.reshape(-1, 3)
    free = np.where(nd[:, 0] >= 0)[0]
    x0 = prob.xyz_new[:, free]
    pos = [np.searchsorted(np.unique(x0[d]), x0[d]) for d in range(3)]
    assert [int(p.max()) + 1 for p in pos] == [3, 9, 3]
    a0 = (pos[0] // 2) * 10 + (pos[1] // 2) * 2 + pos[2] // 2
    a0 = np.searchsorted(np.unique(a0), a0)
    P0, cen = O.rbm_prolongator(a0, x0, 3, 3)
    cpos = [np.searchsorted(np.unique(np.round(cen[d], 9)), np.round(cen[d], 9)) for d in range(3)]
    a1 = np.minimum(cpos[1] // 2, 2)
    a1 = np.searchsorted(np.unique(a1), a1)
    P1, _ = O.rbm_prolongator(a1, cen, 3, 6)
    A = sp.csr_matrix((prob.vals, prob.cols, prob.rowptr))
    assert (A.shape[0], P0.shape[1], P1.shape[1]) == (243, 120, 18)
    return A, [P0, P1], np.asarray(prob.rhs)


def _vectors(n, extra=()):
    v = [np.random.default_rng(5).standard_normal(n), np.ones(n)]
    for i in (0, n - 1) + tuple(extra):
        e = np.zeros(n)
        e[i] = 1.0
        v.append(e)
    return v


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble must be the 80-bit x87 format (x86-64)"


def test_gauss_elimination_with_partial_pivoting():
    rng = np.random.default_rng(3)
    for n in (1, 2, 27, 128):
        M = rng.standard_normal((n, n))
        M[0, 0] = 0.0 if n > 1 else 1.0          # (the first pivot has to come from below)
        b = rng.standard_normal(n)
        LU, perm = R._lu(M.astype(np.longdouble))
        x = R._lu_solve(LU, perm, b.astype(np.longdouble))
        res = np.abs(M.astype(np.longdouble) @ x - b).max()
        assert float(res) <= 1e3 * n * float(np.finfo(np.longdouble).eps) * float(np.abs(M).max() * np.abs(x).max() + np.abs(b).max())
        assert np.abs(x.astype(np.float64) - np.linalg.solve(M, b)).max() <= 1e-8 * max(1.0, float(np.abs(x).max()))


def test_galerkin_reference_is_the_oracles_product():
    """Ac against a dense product in extended precision within the derived tolerance 2 (K + 2) eps Aabs; K counts the terms; the
    bounds of the levels it forms are the ones ``amg_cycle`` reports (the same levels); a rigid-body level gets the unit
    diagonal on its idle rotation dofs and nowhere else."""
    A, aggs = _lap_case(11)
    Ac, Aabs, K = R.galerkin_reference(A, aggs[0])
    P = R.prolongator(aggs[0]).toarray().astype(np.longdouble)
    exact = P.T @ A.toarray().astype(np.longdouble) @ P
    T = 2.0 * (K.toarray() + 2.0) * EPS * Aabs.toarray()
    assert (np.abs(Ac.toarray() - exact) <= T).all()
    assert K.toarray()[0, 0] == 8 + 2 * 12 and K.toarray()[0, 1] == 4          # a brick's 8 diagonals and 12 inner edges; 4 edges to the next brick
    M = R.oracle_cycle(A, aggs)
    lev = R.oracle_levels(A, aggs)
    assert M.lam_true == [R.gershgorin(X) for X in [A] + lev]
    Ab, Ps, _ = _beam_case()
    levb = R.oracle_levels(Ab, Ps)
    assert R.oracle_cycle(Ab, Ps).lam_true == [R.gershgorin(X, rbm=True) for X in [Ab] + levb]
    raw = (Ps[0].T @ Ab @ Ps[0]).tocsr()
    idle = np.where(raw.diagonal() == 0.0)[0]
    assert len(idle) and (idle % 6 >= 3).all()
    d = levb[0].diagonal()
    assert (d[idle] == 1.0).all() and abs(levb[0] - raw - sp.diags((raw.diagonal() == 0.0).astype(float))).max() == 0.0


CASES = {
    "lap11": (11, {}),
    "lap27": (27, {}),
    "lap27_w": (27, dict(gamma=2)),
    "lap27_w_to_1": (27, dict(gamma=2, gamma_to=1)),
    "lap11_degrees": (11, dict(cheb_degree=3, fine_degree=2, eig_ratio=16.0)),
    "lap11_cheb_bottom": (11, dict(dense_limit=20)),          # 27 rows > 20: eight Chebyshev sweeps on the last level
}


def _measure(name):
    if name == "beam":
        A, tr, rhs = _beam_case()
        return (A, tr, dict(eig_ratio=16.0)), _vectors(A.shape[0]) + [rhs]
    n, knobs = CASES[name]
    A, aggs = _lap_case(n)
    return (A, aggs, knobs), _vectors(A.shape[0])


def test_cycle_ld_agrees_with_the_oracles_cycle():
    """e64 on the two Laplacians (V(1,1), degrees 2 and 1, dense bottom) measured 2e-16 to 4e-16; every variant the device can
    run stays at that level."""
    for name in list(CASES) + ["beam"]:
        case, vec = _measure(name)
        e = R.e64(case, vec)
        print(f"e64[{name}] = {e:.3e}")
        assert e <= 64 * EPS, (name, e)


def _moved(case, vec, levels=None, lam=None, knobs=None, restrictions=None):
    """How far the fp64 evaluation with the given mutation is from the extended evaluation of the unmutated cycle, per vector
    (relative, infinity norm), next to the tolerance of one application for this case."""
    A, tr, k0 = case
    M64 = R.oracle_cycle(A, tr, k0)
    lev0 = R.oracle_levels(A, tr)
    ref = R.cycle_ld(A, lev0, tr, M64.lam_true, k0)
    mut = R.cycle_ld(A, levels or lev0, tr, lam or M64.lam_true, dict(k0, **(knobs or {})), dtype=np.float64, restrictions=restrictions)
    tol = R.apply_tolerance(R.e64(case, vec))
    return [R._rel_inf(mut(v).astype(np.longdouble), ref(v)) for v in vec], tol


def _scaled_entry(M, i, j, f):
    M = M.copy().tocsr()
    M.sort_indices()
    k = M.indptr[i] + int(np.searchsorted(M.indices[M.indptr[i]:M.indptr[i + 1]], j))
    assert M.indices[k] == j and M.data[k] != 0.0
    M.data[k] *= f
    return M


def test_the_fp64_restatement_is_within_the_tolerance():
    """cycle_ld(dtype=float64) is the evaluation the mutations are applied to: unmutated it sits inside the tolerance, so what the
    sensitivity test reports is the mutation and not the restatement."""
    for name in ("lap27", "lap27_w", "beam"):
        case, vec = _measure(name)
        moved, tol = _moved(case, vec)
        assert max(moved) <= tol, (name, moved, tol)


def test_sensitivity_to_the_mutations_the_gpu_tests_exist_to_catch():
    f = 1.0 + 1e-9
    case, vec = _measure("lap27")
    A, tr, _ = case
    lev = R.oracle_levels(A, tr)
    lam = R.oracle_cycle(A, tr).lam_true
    seen = {}
    # one coarse entry of a boundary row (row 0 of every coarse level: a corner brick), diagonal and off-diagonal
    for l in range(len(lev)):
        for j in (0, 1):
            m = list(lev)
            m[l] = _scaled_entry(lev[l], 0, j, f)
            seen[f"entry[{l + 1}][0,{j}]"] = _moved(case, vec, levels=m)
    for l in range(len(lam) - 1):          # (the last level's bound is not read when its problem goes to the dense solve ...
        g = list(lam)
        g[l] *= f
        seen[f"lambda[{l}]"] = _moved(case, vec, lam=g)
    bcase, bvec = _measure("beam")          # a rigid-body level's bound: the smaller of two (amg_reference.gershgorin)
    g = list(R.oracle_cycle(*bcase).lam_true)
    g[1] *= f
    seen["lambda[1], rigid-body level"] = _moved(bcase, bvec, lam=g)
    ccase, cvec = _measure("lap11_cheb_bottom")          # ... it is when the level takes the eight Chebyshev sweeps)
    g = list(R.oracle_cycle(*ccase).lam_true)
    g[-1] *= f
    seen["lambda[last, Chebyshev bottom]"] = _moved(ccase, cvec, lam=g)
    seen["coarse_scale"] = _moved(case, vec, knobs=dict(coarse_scale=1.5 * f))
    # the last member of the last aggregate of level 0 is left out of the restriction (the prolongation keeps it)
    P0 = R.prolongator(tr[0]).tolil()
    Rt = P0.T.tolil()
    Rt[P0.shape[1] - 1, P0.shape[0] - 1] = 0.0
    seen["restriction"] = _moved(case, vec, restrictions={0: Rt.tocsr()})
    # the W-cycle's second visit left out: the reference is the W-cycle
    wcase, wvec = _measure("lap27_w")
    seen["second_visit"] = _moved(wcase, wvec, knobs=dict(gamma=1))
    for what, (moved, tol) in seen.items():
        print(f"{what}: moved {max(moved):.3e}  tol {tol:.3e}")
        assert max(moved) > tol, (what, moved, tol)


def test_an_idle_rotation_dofs_diagonal_is_seen_by_the_operator_check_only():
    """The sixth mutation -- the unit diagonal of an idle rotation dof set to 2 -- moves NO application of the cycle: the dof's
    column of P is zero (that is what makes it idle), so its coarse right-hand side is zero for every r, its row holds nothing but
    the diagonal, and the two Gershgorin ratios of the row are 1 for any positive diagonal.  z carries no trace of it, with any
    vector; what sees it is the entrywise comparison of the coarse operators, whose tolerance at that entry is
    2 (K + 16) eps Aabs = 0 (Aabs has nothing there): the device must hold exactly 1.0."""
    case, vec = _measure("beam")
    A, tr, _ = case
    lev = R.oracle_levels(A, tr)
    raw = (tr[0].T @ A @ tr[0]).tocsr()
    i = int(np.where(raw.diagonal() == 0.0)[0][0])
    e = np.zeros(A.shape[0])
    e[np.nonzero(tr[0][:, i - i % 6].toarray().ravel())[0][0]] = 1.0          # a unit vector at a dof of the mutated aggregate
    m = [_scaled_entry(lev[0], i, i, 2.0), lev[1]]
    moved, tol = _moved(case, vec + [e], levels=m)
    assert max(moved) <= tol
    _, Aabs, K = R.galerkin_reference(A, tr[0])
    assert Aabs[i, i] == 0.0 and abs(m[0][i, i] - lev[0][i, i]) == 1.0 > 2 * (K[i, i] + 16) * EPS * Aabs[i, i]
