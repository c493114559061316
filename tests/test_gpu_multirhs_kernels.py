"""One launch of each kernel of pfem_solver_solve_multi (pfem_multi_probe_*) against the operations of
tests/multirhs_reference.py, for panels of 4 and 8 columns.

Row counts, on both sides of every switch of the vector kernels (thread t owns column t % mb; a block holds 256 / mb rows; the
grid is capped at 1 024 blocks): 1, 256/mb - 1, 256/mb, 256/mb + 1, one pass of the capped grid (1 024 x 256/mb rows), one more
row, and two passes + 77.

Integer data (panels in [-4, 4], dinv and alpha powers of two, no zero in the first and last row of a tile and in the last
row): every output and every partial sum is numpy's exact evaluation, bit for bit -- all intermediate values are integers times
a power of two far below 2^53.  Random data (normals x 10^U(-3, 3) per row): the vector outputs are the bits of the written-down
float64 sequence (multirhs_reference.fma is an exact fused multiply-add); a sum of m fma terms is within m eps sum |terms| of
the longdouble sum, the any-order bound of the modal kernel tests.  The one-block kernels add in a fixed order, which the mirror
repeats: their outputs are compared bit for bit, the square roots within one unit in the last place.

A finished column's X, R and P come back with their bits and its W is never read: it is NaN here.  Every device block carries
NaN guard tiles; a launch that reads or writes them fails the probe or poisons a sum."""
import itertools

import numpy as np
import pytest

import multirhs_reference as MR
import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from test_gpu_dynamics import NAMES, case      # noqa: F401  (case: the fixture that builds a Case once)

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = MR.EPS
MBS = [4, 8]


def rows_of(mb):
    t, one_pass = 256 // mb, 1024 * (256 // mb)
    return [1, t - 1, t, t + 1, one_pass, one_pass + 1, 2 * one_pass + 77]


SHAPES = [(mb, n) for mb in MBS for n in rows_of(mb)]
SMALL = [(mb, 256 // mb + 1) for mb in MBS]

_H = {}


def handle():
    if "s" not in _H:
        _H["s"] = pf.PetscSolver().initialise(8, 8)
    return _H["s"]


def int_panel(rng, n, mb):
    """integers in [-4, 4]; no zero in the first and last row of every tile of 256 / mb rows and in the last row"""
    P = rng.integers(-4, 5, (n, mb)).astype(np.float64)
    t = 256 // mb
    edge = np.unique(np.concatenate([np.arange(0, n, t), np.arange(t - 1, n, t), [n - 1]]))
    P[edge] = np.where(P[edge] == 0.0, 3.0, P[edge])
    return P


def rnd_panel(rng, n, mb):
    return rng.standard_normal((n, mb)) * 10.0 ** rng.uniform(-3, 3, (n, 1))


def pow2(rng, n, lo=-3, hi=3):
    return 2.0 ** rng.integers(lo, hi + 1, n).astype(np.float64)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_sums(part, terms, exact, what):
    """part[gv][mb] of the device against the blocks' sums of `terms` (n x mb, longdouble for rounding data)"""
    n, mb = terms.shape
    if exact:
        want = MR.block_partials(np.asarray(terms, np.float64))
        assert np.array_equal(part, want), what
        return
    want = MR.block_partials(terms, LD)
    mag = MR.block_partials(np.abs(terms), LD)
    count = MR.block_partials(np.ones((n, mb)))
    bound = count * EPS * mag
    worst = float((np.abs(part.astype(LD) - want) / np.where(bound > 0, bound, 1)).max())
    print(f"{what}: largest error / bound {worst:.3f}")
    assert (np.abs(part.astype(LD) - want) <= bound).all(), what


def ctl_of(mb, flags, step=0, rng=None):
    c = MR.new_ctl(mb)
    c["flag"][:] = flags
    c["running"] = int((np.asarray(flags) == 0).sum())
    c["step"] = step
    if rng is not None:
        c["beta"][:] = rng.uniform(0.5, 2.0, (mb, 2))
    return c


def masks_of(mb, every):
    if every:
        return [np.array(m) for m in itertools.product([0, 2], repeat=mb)]
    mixed = np.array([0, 2, 0, -3, 0, 0, 3, 0][:mb])
    return [np.zeros(mb, int), mixed]


# ---- k_mcg_init --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["integer", "random"])
@pytest.mark.parametrize("mb,n", SHAPES)
def test_init(mb, n, data):
    rng = np.random.default_rng(100 + mb + n % 1000)
    exact = data == "integer"
    B = int_panel(rng, n, mb) if exact else rnd_panel(rng, n, mb)
    dinv = pow2(rng, n) if exact else rng.uniform(0.1, 10.0, n)
    X, R, P, part = handle().multiProbeInit(B, dinv)
    X0, R0, P0, Z0 = MR.init_op(B, dinv)
    assert part.shape == (MR.vec_grid(n, mb), 2, mb)
    assert same_bits(X, X0) and same_bits(R, R0) and same_bits(P, P0)
    rz, zz = MR.dot_terms(R0, Z0)
    check_sums(part[:, 0], rz, exact, f"init mb {mb} n {n} (r,z)")
    check_sums(part[:, 1], zz, exact, f"init mb {mb} n {n} (z,z)")


@pytest.mark.parametrize("mb,n", SMALL)
def test_init_without_dinv_leaves_p_and_the_partials(mb, n):
    B = rnd_panel(np.random.default_rng(3), n, mb)
    X, R, P, part = handle().multiProbeInit(B, None)
    assert not X.any() and same_bits(R, B) and np.isnan(P).all() and np.isnan(part).all()


# ---- k_mcg_fold and k_mcg_start ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", MBS)
@pytest.mark.parametrize("nb", [1, 31, 32, 33, 77, 1000, 4099])
def test_fold(mb, nb):
    rng = np.random.default_rng(nb + mb)
    pi = rng.integers(-1000, 1001, (nb, mb)).astype(np.float64)
    assert np.array_equal(handle().multiProbeFold(pi), MR.fold_chunks(pi))
    pr = rng.standard_normal((nb, mb)) * 10.0 ** rng.uniform(-3, 3, (nb, 1))
    got, want, mag = handle().multiProbeFold(pr), MR.fold_chunks(pr, LD), MR.fold_chunks(np.abs(pr), LD)
    chunk = -(-nb // MR.FOLD)
    assert (np.abs(got.astype(LD) - want) <= chunk * EPS * mag).all()


@pytest.mark.parametrize("mb", MBS)
@pytest.mark.parametrize("nparts", [1, 7, 256 // 8, 1024])
def test_start(mb, nparts):
    rng = np.random.default_rng(nparts + mb)
    part = rng.uniform(0.0, 2.0, (nparts, 2, mb))
    part[:, :, 1] = 0.0                        # a zero column: reason 3 at the start
    part[:, 0, 2] *= -1.0                      # (r,z) < 0: -8
    c = handle().multiProbeStart(part, 1e-8, 1e-50)
    w = MR.start_op(MR.finish(part), 1e-8, 1e-50)
    assert np.array_equal(c["flag"], w["flag"]) and c["flag"][1] == 3 and c["flag"][2] == -8 and c["running"] == mb - 2 and c["step"] == 0
    assert same_bits(c["beta"], w["beta"]) and not c["its"].any() and not c["verdict"].any()
    for f, ulps in (("rn0", 1), ("rn", 1), ("ttol", 2)):       # (ttol = rtol rn0 carries rn0's unit and its own rounding)
        assert (np.abs(c[f] - w[f]) <= ulps * np.spacing(w[f])).all(), f
    assert same_bits(c["rn"], c["rn0"])


# ---- k_mcg_update --------------------------------------------------------------------------------------------------------------------
def check_update(mb, n, data, flags, broke_col=None, jacobi=True, step=0):
    rng = np.random.default_rng(200 + mb + n % 1000 + step)
    exact = data == "integer"
    make = int_panel if exact else rnd_panel
    W, R = make(rng, n, mb), make(rng, n, mb)
    dinv = (pow2(rng, n) if exact else rng.uniform(0.1, 10.0, n)) if jacobi else None
    ctl = ctl_of(mb, flags, step, rng)
    fold = np.zeros((MR.FOLD, mb))
    if exact:
        ctl["beta"][:] = pow2(rng, 2 * mb, -1, 1).reshape(mb, 2)
        fold[5] = pow2(rng, mb, -1, 1)
    else:
        fold[:] = rng.uniform(0.1, 1.0, (MR.FOLD, mb))
    if broke_col is not None:
        fold[:, broke_col] *= -1.0
    off = np.asarray(flags) != 0
    W[:, off] = np.nan                         # a finished column's W is not read
    c, R2, part = handle().multiProbeUpdate(ctl, fold, W, R, dinv)
    w, Rw, broke = MR.update_op(ctl, fold, W, R, dinv)
    assert same_bits(R2, Rw)
    if ctl["running"] == 0:                    # the launch returns at once
        assert same_bits(R2, R) and np.isnan(part).all()
        return
    assert same_bits(R2[:, off], R[:, off])
    on = ~off & ~broke
    assert same_bits(c["alpha"][on], w["alpha"][on]) and np.array_equal(c["flag"], ctl["flag"]) and c["running"] == ctl["running"] and c["step"] == step
    assert same_bits(c["beta"], ctl["beta"])
    if not jacobi:
        assert np.isnan(part).all()
        return
    assert part.shape == (MR.vec_grid(n, mb), 2, mb) and not np.isnan(part).any()
    Z = np.where(on[None, :], Rw * dinv[:, None], 0.0)
    rz, zz = MR.dot_terms(np.where(on[None, :], Rw, 0.0), Z)
    check_sums(part[:, 0], rz, exact, f"update mb {mb} n {n} (r,z)")
    if broke.any():                            # the marker: -1 from every block, nothing else
        assert (part[:, 1, broke] == -1.0).all() and not part[:, 0, broke].any()
        zz = zz.copy()
        zz[:, broke] = 0
        part = part.copy()
        part[:, 1, broke] = 0.0
    check_sums(part[:, 1], zz, exact, f"update mb {mb} n {n} (z,z)")


@pytest.mark.parametrize("data", ["integer", "random"])
@pytest.mark.parametrize("mb,n", SHAPES)
def test_update(mb, n, data):
    for flags in masks_of(mb, False):
        check_update(mb, n, data, flags, step=n & 1)


@pytest.mark.parametrize("mb,n", SMALL)
def test_update_under_every_mask(mb, n):
    for flags in masks_of(mb, True):
        check_update(mb, n, "random", flags)


@pytest.mark.parametrize("mb,n", SMALL)
def test_update_marks_a_breakdown_and_the_gamg_form(mb, n):
    flags = np.zeros(mb, int)
    flags[1] = 2
    check_update(mb, n, "random", flags, broke_col=2, step=1)
    check_update(mb, n, "random", flags, broke_col=1)            # (p,w) <= 0 in a finished column: nobody looks
    check_update(mb, n, "random", flags, broke_col=0, jacobi=False)
    check_update(mb, n, "integer", flags, jacobi=False, step=1)


def test_update_with_nothing_running():
    mb, n = 4, 300
    rng = np.random.default_rng(9)
    R = rnd_panel(rng, n, mb)
    ctl = ctl_of(mb, [2, 3, -3, 2])
    c, R2, part = handle().multiProbeUpdate(ctl, np.full((MR.FOLD, mb), np.nan), np.full((n, mb), np.nan), R, np.full(n, np.nan))
    assert same_bits(R2, R) and np.isnan(part).all() and c["running"] == 0


# ---- k_mcg_dots ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["integer", "random"])
@pytest.mark.parametrize("mb,n", SHAPES)
def test_dots(mb, n, data):
    rng = np.random.default_rng(300 + mb + n % 1000)
    exact = data == "integer"
    make = int_panel if exact else rnd_panel
    R, Z = make(rng, n, mb), make(rng, n, mb)
    part = handle().multiProbeDots(R, Z)
    rz, zz = MR.dot_terms(R, Z)
    check_sums(part[:, 0], rz, exact, f"dots mb {mb} n {n} (r,z)")
    check_sums(part[:, 1], zz, exact, f"dots mb {mb} n {n} (z,z)")


@pytest.mark.parametrize("mb,n", SMALL)
def test_dots_under_masks_and_the_marker(mb, n):
    rng = np.random.default_rng(31)
    for flags in masks_of(mb, mb == 4):
        off = flags != 0
        R, Z = rnd_panel(rng, n, mb), rnd_panel(rng, n, mb)
        R[:, off] = np.nan
        Z[:, off] = np.nan
        fold = rng.uniform(0.1, 1.0, (MR.FOLD, mb))
        broke = np.zeros(mb, bool)
        if (~off).any():
            j = int(np.flatnonzero(~off)[0])
            fold[:, j] *= -1.0
            broke[j] = True
        part = handle().multiProbeDots(R, Z, ctl_of(mb, flags), fold)
        if off.all():
            assert np.isnan(part).all()
            continue
        on = ~off & ~broke
        assert not part[:, :, off].any() and (part[:, 1, broke] == -1.0).all() and not part[:, 0, broke].any()
        rz, zz = MR.dot_terms(np.where(on[None, :], R, 0.0), np.where(on[None, :], Z, 0.0))
        part = part.copy()
        part[:, 1, broke] = 0.0
        check_sums(part[:, 0], rz, False, "dots under a mask (r,z)")
        check_sums(part[:, 1], zz, False, "dots under a mask (z,z)")


# ---- k_mcg_verdict -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("nparts", [1, 5, 1024])
@pytest.mark.parametrize("mb", MBS)
def test_every_verdict(mb, nparts, parity):
    """column 0 goes on, 1 converges (2), 2 diverges (-4), 3 has (r,z) < 0 (-8); of 8: 4 was finished before (idle), 5 carries
    the breakdown marker (-10), 6 and 7 go on.  With maxits = step + 1 the columns that would go on get -3."""
    step = 6 + parity
    flags = np.zeros(mb, int)
    ctl = ctl_of(mb, flags, step)
    ctl["rn0"][:] = 8.0
    ctl["ttol"][:] = 0.5
    ctl["beta"][:, step & 1] = 4.0
    ctl["beta"][:, (step + 1) & 1] = 777.0
    rz = np.full(mb, 2.0)
    zz = np.full(mb, 9.0)                      # ||z|| = 3: neither converged nor diverged
    zz[1], zz[2], rz[3] = 0.0625, 128.0 ** 2, -2.0      # ||z|| = 0.25 <= ttol; = 128 = dtol ||z0||; (r,z) < 0
    if mb == 8:
        ctl["flag"][4] = 2
        ctl["running"] = 7
    part = np.zeros((nparts, 2, mb))
    if nparts & (nparts - 1) == 0:             # equal shares, a power of two each: the sums are exact in any order
        part[:, 0], part[:, 1] = rz / nparts, zz / nparts
    else:                                      # the first row carries it all
        part[0, 0], part[0, 1] = rz, zz
    if mb == 8:
        part[:, 1, 5] = -1.0
        part[:, 0, 5] = 0.0
    for maxits in (1000, step + 1):
        c = handle().multiProbeVerdict(ctl, part, 16.0, maxits)
        w = MR.verdict_op(ctl, MR.finish(part), 16.0, maxits)
        goes = MR.GOES_ON if maxits == 1000 else MR.LAST_STEP
        want = [goes, MR.LAST_STEP, MR.LAST_STEP, MR.LAST_STEP] + ([MR.IDLE, MR.BROKE, goes, goes] if mb == 8 else [])
        assert list(c["verdict"]) == want and np.array_equal(c["verdict"], w["verdict"])
        last = 0 if maxits == 1000 else -3
        assert list(c["flag"]) == [last, 2, -4, -8] + ([2, -10, last, last] if mb == 8 else [])
        assert np.array_equal(c["flag"], w["flag"]) and np.array_equal(c["its"], w["its"]) and c["step"] == step + 1 == w["step"]
        assert c["running"] == w["running"] == ((1 if mb == 4 else 3) if maxits == 1000 else 0)
        for f in ("beta", "rn", "bb", "rn0", "ttol", "alpha"):
            assert same_bits(c[f], w[f]), f
        assert c["bb"][0] == 0.5 and c["rn"][0] == 3.0 and c["beta"][0][(step + 1) & 1] == 2.0 and c["beta"][0][step & 1] == 4.0
        assert c["its"][0] == step + 1 and (mb == 4 or (c["its"][4] == 0 and c["beta"][5][(step + 1) & 1] == 777.0))


@pytest.mark.parametrize("mb", MBS)
def test_verdict_on_random_partials(mb):
    rng = np.random.default_rng(77)
    for nparts in (3, 100, 1024):
        part = rng.uniform(0.0, 1.0, (nparts, 2, mb))
        ctl = ctl_of(mb, np.zeros(mb, int), 3, rng)
        ctl["rn0"][:] = np.sqrt(part[:, 1].sum(0))
        ctl["ttol"][:] = 1e-8 * ctl["rn0"]
        c = handle().multiProbeVerdict(ctl, part, 1e5, 1000)
        w = MR.verdict_op(ctl, MR.finish(part), 1e5, 1000)
        assert np.array_equal(c["flag"], w["flag"]) and (c["verdict"] == MR.GOES_ON).all() and c["running"] == mb
        assert same_bits(c["beta"], w["beta"]) and same_bits(c["bb"], w["bb"])
        assert (np.abs(c["rn"] - w["rn"]) <= np.spacing(w["rn"])).all()


@pytest.mark.parametrize("mb", MBS)
def test_a_verdict_launch_after_the_last_one_idles_every_column(mb):
    ctl = ctl_of(mb, np.full(mb, 2))
    ctl["verdict"][:] = MR.LAST_STEP
    ctl["its"][:] = 5
    c = handle().multiProbeVerdict(ctl, np.full((4, 2, mb), np.nan), 1e5, 1000)
    assert (c["verdict"] == MR.IDLE).all() and (c["its"] == 5).all() and (c["flag"] == 2).all() and c["running"] == 0 and c["step"] == 0


# ---- k_mcg_direction -----------------------------------------------------------------------------------------------------------------
def check_direction(mb, n, data, verdicts, jacobi=True):
    rng = np.random.default_rng(400 + mb + n % 1000)
    exact = data == "integer"
    make = int_panel if exact else rnd_panel
    R, P, X = make(rng, n, mb), make(rng, n, mb), make(rng, n, mb)
    dinv = (pow2(rng, n) if exact else rng.uniform(0.1, 10.0, n)) if jacobi else None
    Z = None if jacobi else make(rng, n, mb)
    ctl = ctl_of(mb, np.zeros(mb, int))
    ctl["verdict"][:] = verdicts
    ctl["alpha"][:] = pow2(rng, mb) if exact else rng.uniform(0.1, 2.0, mb)
    ctl["bb"][:] = pow2(rng, mb) if exact else rng.uniform(0.1, 2.0, mb)
    still = np.asarray(verdicts) != MR.GOES_ON
    R = R.copy()
    R[:, still] = np.nan                       # z is formed for the columns that go on, for no other
    if Z is not None:
        Z[:, still] = np.nan
    P2, X2 = handle().multiProbeDirection(ctl, R, P, X, dinv=dinv, Z=Z)
    Pw, Xw = MR.direction_op(ctl, R, P, X, dinv=dinv, Z=Z)
    assert same_bits(P2, Pw) and same_bits(X2, Xw)
    quiet = np.isin(verdicts, (MR.IDLE, MR.BROKE))
    assert same_bits(P2[:, still], P[:, still]) and same_bits(X2[:, quiet], X[:, quiet])


@pytest.mark.parametrize("data", ["integer", "random"])
@pytest.mark.parametrize("mb,n", SHAPES)
def test_direction(mb, n, data):
    check_direction(mb, n, data, np.array([1, 2, 0, 3, 1, 1, 2, 1][:mb]))
    check_direction(mb, n, data, np.ones(mb, int), jacobi=False)


@pytest.mark.parametrize("mb,n", SMALL)
def test_direction_under_every_combination_of_verdicts(mb, n):
    combos = list(itertools.product(range(4), repeat=4))
    for k, v in enumerate(combos):
        v = np.array(v + (v[::-1] if mb == 8 else ()))
        check_direction(mb, n, "random", v, jacobi=bool(k & 1))


# ---- k_spmm_dot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", MBS)
@pytest.mark.parametrize("case", ["tet10", "beam2", "cook", "hub_elast", "box19k"], indirect=True)
def test_product_against_the_block_product_and_the_csr(case, mb):
    c = case
    rng = np.random.default_rng(50 + mb)
    P = rng.standard_normal((c.N, mb))
    W, pw = c.s.multiSpmmDot(P)
    assert same_bits(W, c.s.modalSpmm(P))
    rowptr, cols, vals = c.s.getCSR()
    mv = MR.matvec_of(rowptr, cols, vals, LD)
    mva = MR.matvec_of(rowptr, cols, np.abs(vals), LD)
    rowlen = int(np.diff(rowptr).max())
    for j in range(mb):
        want = P[:, j].astype(LD) @ mv(P[:, j].astype(LD))
        mag = np.abs(P[:, j]).astype(LD) @ mva(np.abs(P[:, j]).astype(LD))
        bound = (rowlen + c.N) * EPS * mag
        print(f"{c.name}: MB {mb} column {j}: (p, Kp) error / bound {float(abs(LD(pw[j]) - want) / bound):.3f}")
        assert abs(LD(pw[j]) - want) <= bound


@pytest.mark.parametrize("mb", MBS)
def test_product_on_an_integer_matrix_bit_for_bit(mb):
    """a banded integer matrix through loadCSR and a solve that uploads it: W and (p, Kp) are exact"""
    n = 3 * 256 + 41
    rng = np.random.default_rng(6)
    rows, cols, vals = [], [], []
    for i in range(n):
        cc = sorted({i} | {(i + d) % n for d in (-17, -2, 1, 5, 300)})
        rows += [i] * len(cc)
        cols += cc
        vals += [float(rng.integers(1, 5)) if c == i else float(rng.integers(-3, 4)) for c in cc]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    s = pf.PetscSolver().initialise(n, n)
    try:
        s.loadCSR(rowptr, np.array(cols, np.int32), np.array(vals))
        with pytest.raises(pf.PfemError) as e:               # the staged values are not on the device yet
            s.multiSpmmDot(np.ones((n, mb)))
        assert e.value.code == L.ERR_STATE
        s.setTolerances(maxits=0)
        s.factoriseAndSolve()
        P = int_panel(rng, n, mb)
        W, pw = s.multiSpmmDot(P)
        import scipy.sparse as sp
        A = sp.csr_matrix((np.array(vals), np.array(cols), rowptr), shape=(n, n))
        assert np.array_equal(W, A @ P) and np.array_equal(pw, (P * (A @ P)).sum(0))
    finally:
        s.free()
