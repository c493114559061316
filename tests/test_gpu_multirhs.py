"""Several right-hand sides in one solve on the device (pfem_solver_solve_multi): tet10, beam2, Cook's
membrane and hub_elast under the point Jacobi, tet10 and beam2 also under gamg's cycle, for 1, 3, 4, 5, 8, 9 and 13 columns --
one panel of 4, one of 8, 8 + 4 and 8 + 8 -- at rtol 1e-8.  The columns of a mesh are fixed: the assembled right-hand side, a unit
load, a zero column where one is asked for, and random vectors.

Exact properties: two runs give the same bits; a column's x / its / rnorm are the same bits alone (zero companions), with
companions and at another place of a panel of the same width; B_j 2^k gives x_j 2^k and the same its; a zero column gives
(3, 0, zeros); maxits = 3 gives -3 everywhere; a column that converges long before its neighbour is not touched afterwards (its
bits are those of the run without that neighbour).

Against the references, per column, in longdouble from getCSR (tests/multirhs_reference.py is the mirror; its T is the device's:
1 / K_ii, or amgApply):
  * reason 2 and rnorm <= ttol = rtol ||T b||: the device forms ||T b|| as a float64 sum of N fma terms, so ttol is the
    longdouble one within N eps, and that factor is allowed.
  * the true ||T (b - K x)|| <= ttol + 4 x the gap between the true and the recurrence's norm that the float64 mirror itself
    shows at its last iterate on that column (computed here, with a floor of N eps ||T b||: the rounding of forming the true
    residual at all).
  * its between the counts at which the longdouble mirror first reaches ttol (1 + delta) and ttol (1 - delta), delta = 16 x the
    largest relative difference between the float64 and the longdouble mirror's histories up to the float64 mirror's last
    iterate: the norms of consecutive iterates near ttol can lie within a few per cent of it, so a fixed "+- 0" would test
    rounding, not the kernel.  delta and the bracket are printed.  On the elastic meshes the two histories part by more
    than their own size in mid-run (delta > 1: CG's norms oscillate there, and rounding shifts the oscillation), so
    ttol (1 - delta) means nothing; the upper end is then the count at which the longdouble mirror reaches ttol / (1 + delta),
    the same factor below ttol as the lower end lies above it.
  * column 0 = getRHS() against factoriseAndSolve() + getSolution() on the same handle: |x_multi - x_single|_inf <=
    ||(D^-1 K)^-1||_inf (rho_multi + rho_single), the rho the inf-norms of the two true preconditioned residuals and the dense
    inverse formed here; the single solve's its in the same bracket.
  * maxits = 3: x against the mirror's third iterate within N eps sum_k |alpha_k| |p_k| x 16: three steps whose step lengths
    and directions carry the rounding of three products and six sums of N terms (the factor 16 covers alpha's own error)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

import multirhs_reference as MR
import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_dynamics import ANISO, case, get_case      # noqa: F401  (case: the fixture that builds a Case once)
from test_gpu_implicit import tolerances

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = MR.EPS
RTOL = 1e-8
MESHES = ["tet10", "beam2", "cook", "hub_elast"]
NRHS = [1, 3, 4, 5, 8, 9, 13]
_B, _REF, _INV = {}, {}, {}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def columns(c):
    """13 columns: the assembled right-hand side, a unit load, random vectors of different sizes"""
    if c.name not in _B:
        rng = np.random.default_rng(13)
        B = rng.standard_normal((13, c.N)) * 10.0 ** rng.uniform(-2, 2, (13, 1))
        B[0] = c.s.getRHS()
        B[1] = 0.0
        B[1, c.N // 3] = 1.0
        _B[c.name] = B
    return _B[c.name]


def csr_of(c):
    return c.p.rowptr, c.p.cols, c.p.vals


def preconditioner(c, pc, dtype):
    if pc == "jacobi":
        return MR.jacobi_of(*csr_of(c), dtype)
    return lambda r: c.s.amgApply(np.asarray(r, np.float64)).astype(dtype)


def true_residual(c, pc, b, x):
    """T (b - K x) with the product and the difference in longdouble"""
    r = b.astype(LD) - MR.matvec_of(*csr_of(c), LD)(np.asarray(x).astype(LD))
    return preconditioner(c, pc, LD)(r)


def reference(c, pc, j):
    """the float64 and the longdouble mirror on column j, ttol, delta, the bracket of its and the float64 mirror's gap: once"""
    key = (c.name, pc, j)
    if key not in _REF:
        b = columns(c)[j]
        r64 = MR.pcg(lambda x: c.A @ x, b, preconditioner(c, pc, np.float64), rtol=RTOL)
        rld = MR.pcg(MR.matvec_of(*csr_of(c), LD), b, preconditioner(c, pc, LD), rtol=RTOL / 16, dtype=LD)
        ttol = LD(RTOL) * rld.hist[0]
        upto = min(len(r64.hist), len(rld.hist))
        delta = 16.0 * float((np.abs(r64.hist[:upto].astype(LD) - rld.hist[:upto]) / rld.hist[:upto]).max())
        lo = MR.first_at_or_below(rld.hist, ttol * (1 + delta))
        if delta < 1.0:
            hi = MR.first_at_or_below(rld.hist, ttol * (1 - delta))
        else:                                  # (1 - delta) has no meaning: the same factor below ttol as above it
            rld = MR.pcg(MR.matvec_of(*csr_of(c), LD), b, preconditioner(c, pc, LD), rtol=RTOL / (2 * (1 + delta)), dtype=LD)
            hi = MR.first_at_or_below(rld.hist, ttol / (1 + delta))
        rho = true_residual(c, pc, b, r64.x)
        floor = c.N * EPS * float(rld.hist[0])
        gap = max(abs(float(np.sqrt(rho @ rho)) - float(r64.hist[-1])), floor)
        print(f"{c.name} {pc} column {j}: mirror {r64.its} (float64) iterations, ttol {float(ttol):.3e}, delta {delta:.2e}, bracket [{lo}, {hi}], "
              f"gap {gap:.2e}")
        assert r64.reason == 2 and lo is not None and hi is not None
        _REF[key] = dict(ttol=float(ttol), delta=delta, lo=lo, hi=hi, gap=gap, r64=r64)
    return _REF[key]


def in_bracket(ref, its):
    return ref["lo"] <= its <= ref["hi"]


class Gamg:
    """gamg in effect on the case's handle with a solve behind it, Jacobi again afterwards"""

    def __init__(self, c, pc):
        self.c, self.pc = c, pc

    def __enter__(self):
        if self.pc == "gamg":
            self.c.s.setPreconditioner("gamg")
            assert self.c.s.factoriseAndSolve()[1] > 0
        return self.c.s

    def __exit__(self, *a):
        self.c.s.setPreconditioner("jacobi")


def solve(c, B, pc="jacobi", **tol):
    """under gamg: inside a Gamg block, so that several runs and the mirror's T share one numeric set-up"""
    with tolerances(c.s, rtol=RTOL, **tol):
        r = c.s.solveMany(B)
    assert r.pc == pc and r.x.shape == np.atleast_2d(B).shape
    return r


# ---- against the references ------------------------------------------------------------------------------------------------------
def check_against_the_references(c, pc, nrhs):
    B = columns(c)[:nrhs]
    with Gamg(c, pc):
        r = solve(c, B, pc)
        refs = [reference(c, pc, j) for j in range(nrhs)]
        rhos = [true_residual(c, pc, B[j], r.x[j]) for j in range(nrhs)]
    for j in range(nrhs):
        ref, rho = refs[j], rhos[j]
        true = float(np.sqrt(rho @ rho))
        print(f"{c.name} {pc} nrhs {nrhs} column {j}: its {r.iterations[j]} in [{ref['lo']}, {ref['hi']}], rnorm {r.rnorm[j]:.3e}, true {true:.3e}, "
              f"ttol {ref['ttol']:.3e}")
        assert r.reasons[j] == 2
        assert r.rnorm[j] <= ref["ttol"] * (1 + c.N * EPS)
        assert true <= ref["ttol"] + 4 * ref["gap"]
        assert in_bracket(ref, r.iterations[j])
    return r


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("case", MESHES, indirect=True)
def test_jacobi_against_the_references(case, nrhs):
    check_against_the_references(case, "jacobi", nrhs)


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("case", ["tet10", "beam2"], indirect=True)
def test_gamg_against_the_references(case, nrhs):
    check_against_the_references(case, "gamg", nrhs)


@pytest.mark.parametrize("case", MESHES, indirect=True)
def test_column_0_against_the_single_solve(case):
    c = case
    b = columns(c)[0]
    ref = reference(c, "jacobi", 0)
    with tolerances(c.s, rtol=RTOL):
        its, reason, _ = c.s.factoriseAndSolve()
        x_single = c.s.getSolution()
        r = c.s.solveMany(b)
    if c.name not in _INV:
        d = c.A.diagonal()
        _INV[c.name] = float(np.abs(np.linalg.inv(c.A.toarray() / d[:, None])).sum(axis=1).max())
    rho_m = float(np.abs(true_residual(c, "jacobi", b, r.x[0])).max())
    rho_s = float(np.abs(true_residual(c, "jacobi", b, x_single)).max())
    err, bound = np.abs(r.x[0] - x_single).max(), _INV[c.name] * (rho_m + rho_s)
    print(f"{c.name}: single {its} iterations, multi {r.iterations[0]}, bracket [{ref['lo']}, {ref['hi']}]; |x_multi - x_single| {err:.3e} <= {bound:.3e}")
    assert reason == 2 and r.reasons[0] == 2
    assert err <= bound
    assert in_bracket(ref, its) and in_bracket(ref, r.iterations[0])


# ---- exact properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("case", ["tet10", "beam2"], indirect=True)
def test_two_runs_give_the_same_bits(case, pc):
    B = columns(case)[:9]
    with Gamg(case, pc):
        a, b = solve(case, B, pc), solve(case, B, pc)
    assert same_bits(a.x, b.x) and same_bits(a.rnorm, b.rnorm) and np.array_equal(a.iterations, b.iterations) and np.array_equal(a.reasons, b.reasons)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("case", MESHES, indirect=True)
def test_a_column_does_not_depend_on_its_companions_or_its_place(case, width):
    c = case
    B = columns(c)
    nrhs = 3 if width == 4 else 7              # (one panel of `width`)
    full = solve(c, B[:nrhs])
    for j in (0, 2):
        alone = np.zeros((nrhs, c.N))
        alone[j] = B[j]
        a = solve(c, alone)
        moved = np.roll(B[:nrhs], 1, axis=0)   # column j at place j + 1, other companions around it
        m = solve(c, moved)
        for r, k in ((a, j), (m, (j + 1) % nrhs)):
            assert same_bits(r.x[k], full.x[j]) and r.iterations[k] == full.iterations[j] and same_bits(r.rnorm[k], full.rnorm[j])
        others = [k for k in range(nrhs) if k != j]
        assert (a.reasons[others] == 3).all() and not a.iterations[others].any() and not a.x[others].any() and not a.rnorm[others].any()


@pytest.mark.parametrize("k", [20, -20])
@pytest.mark.parametrize("case", ["tet10", "beam2"], indirect=True)
def test_a_power_of_two_scales_the_solution_bit_for_bit(case, k):
    B = columns(case)[:5]
    a, s = solve(case, B), solve(case, B * 2.0 ** k)
    assert same_bits(a.x * 2.0 ** k, s.x) and np.array_equal(a.iterations, s.iterations) and same_bits(a.rnorm * 2.0 ** k, s.rnorm)


@pytest.mark.parametrize("case", MESHES, indirect=True)
def test_zero_columns_and_maxits_3(case):
    c = case
    B = columns(c)[:6].copy()
    B[2] = 0.0
    B[5] = 0.0
    r = solve(c, B, maxits=3)
    zero = np.array([2, 5])
    live = np.array([0, 1, 3, 4])
    assert (r.reasons[zero] == 3).all() and not r.iterations[zero].any() and not r.x[zero].any() and not r.rnorm[zero].any()
    assert (r.reasons[live] == -3).all() and (r.iterations[live] == 3).all()
    mv, T = MR.matvec_of(*csr_of(c), LD), preconditioner(c, "jacobi", LD)
    for j in live:
        m = MR.pcg(mv, B[j], T, rtol=RTOL, maxits=3, dtype=LD, keep=True)
        steps = np.diff(np.vstack([np.zeros(c.N, LD)] + m.xs), axis=0)
        bound = 16 * c.N * EPS * np.abs(steps).sum(axis=0)
        assert m.reason == -3 and (np.abs(r.x[j].astype(LD) - m.x) <= bound + 16 * c.N * EPS * np.abs(m.x).max()).all()
        assert abs(r.rnorm[j] - float(m.hist[3])) <= 64 * c.N * EPS * float(m.hist[0])


@pytest.mark.parametrize("case", ["tet10", "beam2"], indirect=True)
def test_an_early_column_is_left_alone_afterwards(case):
    """the unit load at 1e-2 of its ||z0|| converges many iterations before the assembled right-hand side at rtol 1e-8 does --
    abstol lets it: its bits are those of the run without the late neighbour"""
    c = case
    d = c.A.diagonal()
    B = columns(c)[:2][::-1].copy()            # the unit load, then the assembled right-hand side ...
    z0 = 1.0 / d[c.N // 3]
    B[1] *= 1e8 * z0 / np.sqrt(((B[1] / d) ** 2).sum())         # ... at a size where rtol ||z0|| is 100 abstol
    with tolerances(c.s, rtol=RTOL, abstol=1e-2 * z0):
        both = c.s.solveMany(B)
        early = c.s.solveMany(B[0])
    print(f"{c.name}: the unit load stops after {both.iterations[0]} iterations (reason {both.reasons[0]}), its neighbour after {both.iterations[1]}")
    assert both.iterations[0] + 5 <= both.iterations[1] and both.reasons[0] == 3
    assert same_bits(both.x[0], early.x[0]) and both.iterations[0] == early.iterations[0] and same_bits(both.rnorm[0], early.rnorm[0])


# ---- isolation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("case", ["tet10", "beam2"], indirect=True)
def test_the_single_solve_is_unchanged_around_a_multi_solve(case, pc):
    c, s = case, case.s
    B = columns(c)[:5]
    s.setPreconditioner(pc)
    try:
        with tolerances(s, rtol=RTOL):
            before = s.factoriseAndSolve()
            x0, h0, rhs0 = s.getSolution(), s.getHistory(), s.getRHS()
            r = s.solveMany(B)
            assert r.pc == pc and (r.reasons == 2).all()
            assert same_bits(s.getSolution(), x0) and same_bits(s.getRHS(), rhs0) and same_bits(s.getHistory(), h0)
            after = s.factoriseAndSolve()
            assert after == before and same_bits(s.getSolution(), x0) and same_bits(s.getHistory(), h0)
    finally:
        s.setPreconditioner("jacobi")


def test_modal_and_implicit_runs_are_unchanged_around_a_multi_solve(golden_dir):
    c = get_case("tet10", golden_dir)
    s, B = c.s, columns(c)[:5]
    a = s.modalSolve(2, tol=1e-6, max_iterations=400)
    with tolerances(s, rtol=RTOL):
        s.solveMany(B)
    b = s.modalSolve(2, tol=1e-6, max_iterations=400)
    assert a.iterations == b.iterations and same_bits(a.omega2, b.omega2) and same_bits(a.modes, b.modes)
    c = get_case("beam2", golden_dir)
    s, B = c.s, columns(c)[:5]
    rng = np.random.default_rng(3)
    u0, v0 = rng.standard_normal(c.N), rng.standard_normal(c.N)
    dt = 20.0 * c.dt
    c.device(0.0, u0, v0)
    s.implicitRun(dt, 6)
    s.implicitRun(dt, 6)
    t_a, u_a, v_a = s.dynamicsState()
    c.device(0.0, u0, v0)
    s.implicitRun(dt, 6)
    with tolerances(s, rtol=RTOL):
        s.solveMany(B)
    s.implicitRun(dt, 6)
    t_b, u_b, v_b = s.dynamicsState()
    assert t_a == t_b and same_bits(u_a, u_b) and same_bits(v_a, v_b)


# ---- renumbering -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tet10_r", "tet10_s", "box19k_r", "box19k_s"], indirect=True)
def test_columns_and_solutions_are_in_the_callers_order(case):
    """a random node numbering: with PFEM_REORDER=1 the library holds the mesh renumbered at any size, left to itself from
    4 096 owned dofs on.  x against sparse LU of getCSR's matrix -- the caller's order -- within ||(D^-1 K)^-1|| rho, with the norm
    estimated through the LU itself (scipy's onenormest of D K^-1, which is within a factor 3 of the norm: x 4)."""
    c = case
    assert c.s.reordered() == (c.name != "tet10_s")
    nrhs = 5
    B = columns(c)[:nrhs]
    r = solve(c, B)
    d = c.A.diagonal()
    lu = spl.splu(c.A.tocsc())
    # ||(D^-1 K)^-1||_inf = ||D K^-1||_1 (K is symmetric)
    op = spl.LinearOperator((c.N, c.N), matvec=lambda v: d * lu.solve(np.ravel(v)), rmatvec=lambda v: lu.solve(d * np.ravel(v)), dtype=np.float64)
    ninv = 4.0 * spl.onenormest(op)
    for j in range(nrhs):
        rho = true_residual(c, "jacobi", B[j], r.x[j])
        x_lu = lu.solve(B[j])
        err = np.abs(r.x[j] - x_lu).max()
        bound = ninv * float(np.abs(rho).max()) + c.N * EPS * ninv * np.abs(B[j] / d).max()
        ttol = RTOL * float(np.sqrt(((B[j] / d).astype(LD) ** 2).sum()))
        print(f"{c.name} column {j}: {r.iterations[j]} iterations, |x - x_LU| {err:.3e} <= {bound:.3e}, true residual {float(np.sqrt(rho @ rho)):.3e}, ttol {ttol:.3e}")
        assert r.reasons[j] == 2 and r.rnorm[j] <= ttol * (1 + c.N * EPS)
        assert err <= bound
        assert float(np.sqrt(rho @ rho)) <= 2 * ttol       # K x = b in the caller's order: a permuted x would leave ||T b|| itself


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(pf.PfemError) as ei:
        call()
    return ei.value.code


def test_state_errors(golden_dir):
    mesh = H.read_mesh(f"{golden_dir}/input/tet10")
    dm, conn, xyz, edof = D._setup(pf.POISSON_TET, mesh)
    N = dm.size_global
    b = np.ones((2, N))
    s = pf.PetscSolver().initialise(N, N)
    assert _code(lambda: s.solveMany(b)) == L.ERR_STATE                         # no pattern
    s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    assert _code(lambda: s.solveMany(b)) == L.ERR_STATE                         # no assembled matrix
    s.assemble(ANISO, H.TIMEDATA)
    for bad in (np.ones((65, N)), ):
        assert _code(lambda: s.solveMany(bad)) == L.ERR_ARG
    assert _code(lambda: s.solveMany(b, pc=9)) == L.ERR_ARG
    with pytest.raises(ValueError):
        s.solveMany(np.ones((2, N + 1)))
    assert s.solveMany(b).pc == "jacobi" and s.solveMany(b, pc="pbjacobi").pc == "jacobi"
    # gamg in effect but no gamg solve since the assemble: the point Jacobi runs, and asking for gamg by name is refused
    s.setPreconditioner("gamg")
    assert s.solveMany(b).pc == "jacobi"
    assert _code(lambda: s.solveMany(b, pc="gamg")) == L.ERR_STATE
    s.factoriseAndSolve()
    assert s.solveMany(b).pc == "gamg" and s.solveMany(b, pc="jacobi").pc == "jacobi"
    s.assemble(ANISO, H.TIMEDATA)                                               # new values: the cycle's set-up is not theirs
    assert s.solveMany(b).pc == "jacobi"
    s.setPreconditioner("jacobi")
    s.buildPattern()                                                            # a new pattern drops the state
    assert _code(lambda: s.solveMany(b)) == L.ERR_STATE
    # more than one rank: refused before anything is launched
    s.assemble(ANISO, H.TIMEDATA)
    cb = lambda *a: 0      # noqa: E731
    s.setCommHost(0, 2, cb, cb)
    assert _code(lambda: s.solveMany(b)) == L.ERR_STATE
    s.free(collective=False)
    # the MatSetValues path: refused while the staged values are not on the device, fine after the solve that uploads them
    compat = pf.tetrapoissonparallelimpl1(H.gen_box_tets(-1, 1, 3, -1, 1, 3, -1, 1, 3), rtol=1e-6, mode="compat").solver
    n = compat.matrixInfo()["n_owned"]
    rhs = compat.getRHS()
    x = compat.getSolution()
    with tolerances(compat, rtol=1e-10):
        r = compat.solveMany(rhs)
    assert r.reasons[0] == 2 and np.abs(r.x[0] - x).max() <= 1e-5 * np.abs(x).max()       # (8 dofs: both end at the solution)
    rowptr, cols, vals = compat.getCSR()
    compat.loadCSR(rowptr, cols, vals, values_only=True)
    assert _code(lambda: compat.solveMany(np.ones(n))) == L.ERR_STATE
    assert "staged" in str(pytest.raises(pf.PfemError, lambda: compat.solveMany(np.ones(n))).value)
