"""The numpy mirror of the solve for several right-hand sides (tests/multirhs_reference.py) against scipy's sparse LU, so that
the yardstick of the GPU tests is itself checked -- and what pfem_solver_solve_multi answers without a handle, with bad
arguments and without a device.

Fixtures: the 6 x 6 x 6 Poisson box (125 dofs) and the 3 x 12 x 3 clamped beam (576 dofs) through oracle.setup_problem, under
the point Jacobi at rtol 1e-8.  Columns: the assembled right-hand side, three random vectors and a unit vector.

Bounds.  x against LU: with e = x - x_LU and rho = D^-1 (b - K x), e = (D^-1 K)^-1 rho, so |e|_inf <= ||(D^-1 K)^-1||_inf
|rho|_inf with the dense inverse formed here and rho in longdouble -- plus the LU's own error, taken as n eps ||(D^-1 K)^-1||_inf
|D^-1 b|_inf.  The recurrence's norm against the true one: the last ||z|| of the history is <= ttol by the stopping test; the
true ||rho||_2 may differ from it by what the recurrence has drifted, which is printed and bounded by 1e-3 ttol: every update
rounds r to eps of its size, so after `its` steps the drift is of the order its eps max_k ||z_k||; with ttol = 1e-8 ||z0|| and
260 steps that is 3e-6 ttol where the norms never exceed ||z0||, and 1e-3 leaves room for the growth CG shows in between."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import multirhs_reference as MR
from oracle import pfem_oracle as O
from pfemfort_amd import _lib

LD = np.longdouble
RTOL = 1e-8
_FIX = {}


def fixture_of(name):
    """(problem, K as CSR, the five columns), made once"""
    if name not in _FIX:
        if name == "box":
            p = O.setup_problem(O.POISSON_TET, O.gen_box_tets(0, 1, 6, 0, 1, 6, 0, 1, 6))
        else:
            p = O.setup_problem(O.ELAST_TET, O.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3))
        n = len(p.rowptr) - 1
        A = sp.csr_matrix((p.vals, p.cols, p.rowptr), shape=(n, n))
        rng = np.random.default_rng(16)
        unit = np.zeros(n)
        unit[n // 3] = 1.0
        B = np.vstack([p.rhs, rng.standard_normal((3, n)), unit])
        _FIX[name] = (p, A, B)
    return _FIX[name]


def run(p, b, dtype=np.float64, **kw):
    return MR.pcg(MR.matvec_of(p.rowptr, p.cols, p.vals, dtype), b, MR.jacobi_of(p.rowptr, p.cols, p.vals, dtype), dtype=dtype, **kw)


@pytest.mark.parametrize("name,n", [("box", 125), ("beam", 576)])
def test_the_mirror_against_sparse_lu(name, n):
    p, A, B = fixture_of(name)
    assert A.shape[0] == n
    d = A.diagonal()
    inv = np.linalg.inv(A.toarray() / d[:, None])
    ninv = np.abs(inv).sum(axis=1).max()
    lu = spl.splu(A.tocsc())
    mv = MR.matvec_of(p.rowptr, p.cols, p.vals, LD)
    for j, b in enumerate(B):
        r64, rld = run(p, b, rtol=RTOL), run(p, b, LD, rtol=RTOL)
        x_lu = lu.solve(b)
        for tag, r in (("float64", r64), ("longdouble", rld)):
            rho = (b.astype(LD) - mv(r.x.astype(LD))) / d
            true = float(np.sqrt(rho @ rho))
            gap = abs(true - float(r.hist[-1]))
            err = np.abs(r.x - x_lu).max()
            bound = ninv * float(np.abs(rho).max()) + n * MR.EPS * ninv * np.abs(b / d).max()
            print(f"{name} column {j} {tag}: {r.its} iterations, ||z|| {float(r.hist[-1]):.3e} <= ttol {float(r.ttol):.3e}, true {true:.3e} (gap {gap:.1e}); "
                  f"|x - x_LU| {err:.3e} <= {bound:.3e}")
            assert r.reason == 2 and r.its == len(r.hist) - 1
            assert r.hist[-1] <= r.ttol and (r.hist[:-1] > r.ttol).all()
            assert gap <= 1e-3 * float(r.ttol)
            assert err <= bound
        # the two precisions stop within a few iterations of each other (rounding moves the stopping iteration, no more)
        assert abs(r64.its - rld.its) <= 4
    if name == "box":
        assert 20 <= run(p, B[0], rtol=RTOL).its <= 30
    else:
        assert 240 <= run(p, B[0], rtol=RTOL).its <= 280


def test_the_reasons():
    p, A, B = fixture_of("box")
    n = A.shape[0]
    # -3: maxits 3 in every nonzero column, with the third iterate
    for b in B:
        r = run(p, b, rtol=RTOL, maxits=3, keep=True)
        assert r.reason == -3 and r.its == 3 and len(r.hist) == 4 and np.array_equal(r.x, r.xs[2])
    # 3: a zero column finishes at the start with x = 0 exactly
    r = run(p, np.zeros(n), rtol=RTOL)
    assert r.reason == 3 and r.its == 0 and not r.x.any() and len(r.hist) == 1 and r.hist[0] == 0.0
    # -10: (p, Kp) <= 0 -- a matrix with a negative diagonal entry, T = 1, the unit vector there
    K = A.tolil(copy=True)
    K[7, 7] = -K[7, 7]
    K = K.tocsr()
    e7 = np.zeros(n)
    e7[7] = 1.0
    r = MR.pcg(lambda x: K @ x, e7, lambda v: v.copy(), rtol=RTOL)
    assert r.reason == -10 and r.its == 1 and not r.x.any()
    # -8: a T that is not positive
    r = MR.pcg(lambda x: A @ x, B[1], lambda v: -v, rtol=RTOL)
    assert r.reason == -8 and r.its == 0
    # -4: dtol
    r = run(p, B[1], rtol=RTOL, dtol=1e-3)
    assert r.reason == -4 and r.its == 1
    # 3 through abstol
    r = run(p, B[1], rtol=RTOL, abstol=1e-3)
    assert r.reason == 3 and r.hist[-1] <= 1e-3


@pytest.mark.parametrize("k", [20, -20])
def test_a_power_of_two_scales_every_iterate_bit_for_bit(k):
    p, _, B = fixture_of("beam")
    for b in B[[0, 2]]:
        a = run(p, b, rtol=RTOL, keep=True)
        s = run(p, b * 2.0 ** k, rtol=RTOL, keep=True)
        assert a.its == s.its and a.reason == s.reason
        assert np.array_equal(a.hist * 2.0 ** k, s.hist)
        assert all(np.array_equal(x * 2.0 ** k, y) for x, y in zip(a.xs, s.xs))


def test_the_exact_fma():
    """multirhs_reference.fma against exact rationals, also where the sum cancels and where it falls on a tie"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000) * 10.0 ** rng.uniform(-3, 3, 4000)
    b = rng.standard_normal(4000) * 10.0 ** rng.uniform(-3, 3, 4000)
    c = rng.standard_normal(4000) * 10.0 ** rng.uniform(-3, 3, 4000)
    c[:500] = -(a[:500] * b[:500])                       # the rounded product cancels: the result is the product's rounding error
    a[500:600], b[500:600], c[500:600] = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -23, 2.0 ** -53       # 54 bits and a tie behind them
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    assert np.array_equal(MR.fma(a, b, c), want)
    assert (want[:500] != 0.0).any()


def test_the_one_block_sums_and_the_operations():
    """finish / start / verdict / direction of the mirror on a panel worked by hand"""
    part = np.zeros((3, 2, 4))
    part[:, 0] = [[1, 2, 3, 4], [10, 20, 30, 40], [100, 200, 300, 400]]
    part[:, 1] = [[1, 0, 4, 9], [0, 0, 0, 0], [3, 0, 12, 16]]
    tot = MR.finish(part)
    assert np.array_equal(tot, [[111, 222, 333, 444], [4, 0, 16, 25]])
    c = MR.start_op(tot, 0.5, 1e-50)
    assert np.array_equal(c["rn0"], [2, 0, 4, 5]) and np.array_equal(c["flag"], [0, 3, 0, 0]) and c["running"] == 3 and c["step"] == 0
    assert np.array_equal(c["ttol"], [1, 1e-50, 2, 2.5]) and np.array_equal(c["beta"][:, 0], tot[0])
    # the next sums: column 0 converges, column 2 goes on, column 3 carries the breakdown marker
    v = MR.verdict_op(c, np.array([[55.5, 7.0, 111.0, 0.0], [0.25, 9.0, 9.0, -1.0]]), 1e5, 100)
    assert np.array_equal(v["flag"], [2, 3, 0, -10]) and np.array_equal(v["verdict"], [MR.LAST_STEP, MR.IDLE, MR.GOES_ON, MR.BROKE])
    assert np.array_equal(v["its"], [1, 0, 1, 1]) and v["running"] == 1 and v["step"] == 1
    assert v["bb"][0] == 0.5 and v["bb"][2] == 111.0 / 333.0 and v["beta"][2][1] == 111.0 and v["beta"][3][1] == 0.0
    v["alpha"][:] = [2.0, 9.0, 0.5, 9.0]
    R = np.ones((5, 4)); P = np.full((5, 4), 3.0); X = np.full((5, 4), 10.0)
    P2, X2 = MR.direction_op(v, R, P, X, dinv=np.full(5, 0.25))
    assert np.array_equal(X2[0], [16.0, 10.0, 11.5, 10.0]) and np.array_equal(P2[0], [3.0, 3.0, 0.25 + 3.0 * (111.0 / 333.0), 3.0])
    # a launch after the last verdict: nothing runs, every verdict idle
    v["running"] = 0
    assert (MR.verdict_op(v, tot, 1e5, 100)["verdict"] == MR.IDLE).all()


# ---- the entry point without a handle, with bad arguments, without a device ---------------------------------------------------
def _call(handle, nrhs=2, pc=-1, n=100, skip=None):
    B, X, rn = np.zeros((max(nrhs, 1), n)), np.zeros((max(nrhs, 1), n)), np.zeros(max(nrhs, 1))
    its, why = np.zeros(max(nrhs, 1), np.int32), np.zeros(max(nrhs, 1), np.int32)
    args = {"B": B, "X": X, "its": its, "why": why, "rn": rn}
    ptr = {k: (None if k == skip else v.ctypes.data) for k, v in args.items()}
    return _lib.lib().pfem_solver_solve_multi(handle, nrhs, ptr["B"], pc, ptr["X"], ptr["its"], ptr["why"], ptr["rn"])


def test_the_new_symbols_bind():
    lib = _lib.lib()
    for name in ("pfem_solver_solve_multi", "pfem_multi_probe_init", "pfem_multi_probe_start", "pfem_multi_probe_fold", "pfem_multi_probe_update",
                 "pfem_multi_probe_dots", "pfem_multi_probe_verdict", "pfem_multi_probe_direction", "pfem_multi_spmm_dot", "pfem_multi_last_pc",
                 "pfem_multi_bench"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert _lib.MULTI_MAX_RHS == 64 and C.sizeof(_lib.McgCtl) == 8 * (16 + 5 * 8) + 4 * (3 * 8 + 2)


def test_the_entry_point_without_a_handle():
    assert _call(None) == _lib.ERR_ARG
    assert _lib.lib().pfem_multi_last_pc(None, None) == _lib.ERR_ARG


def test_bad_arguments_and_no_device():
    """argument errors come before the device is looked for; with good arguments a machine without a device answers
    PFEM_ERR_NOGPU (there already for the handle), one with a device PFEM_ERR_STATE (no pattern on this handle)"""
    lib = _lib.lib()
    h = C.c_void_p()
    rc = lib.pfem_solver_create(C.byref(h), 100, 100, 0, None, None, 0)
    if rc == _lib.ERR_NOGPU:               # no handle without a device: the argument checks of the NULL handle are all there is
        assert _call(None, nrhs=0) == _lib.ERR_ARG
        return
    assert rc == _lib.OK
    try:
        for kw in (dict(nrhs=0), dict(nrhs=-1), dict(nrhs=_lib.MULTI_MAX_RHS + 1), dict(pc=7), dict(pc=-2), dict(skip="B"), dict(skip="X"),
                   dict(skip="its"), dict(skip="why"), dict(skip="rn")):
            assert _call(h, **kw) == _lib.ERR_ARG, kw
        assert _call(h) == _lib.ERR_STATE
        used = C.c_int(0)
        assert lib.pfem_multi_last_pc(h, C.byref(used)) == _lib.ERR_STATE
    finally:
        lib.pfem_solver_destroy(h)
