"""One launch of each vector kernel of the steppers (stepperProbe*: pfem_imp_probe_* and pfem_dyn_probe_step, DESIGN.md sections
11 and 12) against a plain evaluation of the same operation, at row counts on both sides of every point where a kernel takes
another path: one row, the tail of a thread's four rows, a block less one row, a block, a block and a row, the last count one
trip of the capped grid covers (2 048 blocks x 1 024 rows), one more, and a count at which some blocks take three trips and
others two with a ragged last chunk -- for the explicit step, which has no loop, 4 100 blocks and as many partials.  The meshes
of test_gpu_implicit.py and test_gpu_dynamics.py end at 19 656 rows: 20 blocks, one trip, 20 partials; and a CG that sums a
slightly wrong (p, Ap) still converges.  Here every launch stands alone on vectors the test supplies, through the run's own grid
function, parameter block and launch line, and the probes themselves watch the 8 NaNs in front of and the 1 024 behind every
vector and the bits of every vector a kernel takes as const.

Exact data.  Small integers (vectors in [-4, 4], m in [1, 4], dinv and 1 / m powers of two, dt = 1, beta = 1/4, gamma = 1/2:
sigma = 4, beta dt^2 = 1/4, gamma dt = 1/2; theta = 1/2: sigma = 2; the step lengths and beta ratios powers of two): every term
is a multiple of a power of two and every sum of magnitudes stays below 2^53 in those units -- asserted on the reference --, so
no result depends on the order of a sum: output vectors, every block's partial (block b owns the rows r with
(r // 1024) % gv == b; the explicit step: r // 1024 == b) and the consumer's total must carry the reference's bits.  Rows 0,
n - 1 and the first and last row of every block of 1 024 hold no zero.

Rounding data.  Standard normals times 10**uniform(-3, 3) per row, m > 0.  What the kernels compute without fma -- predict,
correct, b and z of the right-hand side, the explicit step -- carries the bits of the float64 reference.  The fma recurrences
are measured against numpy longdouble on the same float64 inputs, eps = 2^-52:
  r' = fma(-alpha, fma(sigma m, p, w), r)   eps (|alpha| (|sigma m p| + |w|) + |r'|)
  p' = fma(bb, p, r dinv)                   eps (|bb p| + |r dinv| + |p'|)
  d' = fma(alpha, p, d)                     eps |d'|
(each is two roundings, or one, of at most eps / 2 of a part of the bound; the last bound holds no part of the operands, so where
d + alpha p cancels the 64 bits of a longdouble product would not do: IR.direction forms those rows in exact rationals); every sum of n terms (n + 3) eps x the sum of the
terms' magnitudes, the terms formed in longdouble from the float64 vectors the kernel itself stored; ||z_0|| from a sum of
squares: ((n + 3) / 2 + 1) eps ||z_0||.  alpha and bb are one float64 division of sums of integer partials, so the reference
holds the kernel's values of them.  The largest error / bound per kernel and count is printed; a second call gives the same
bits."""
import ctypes as C

import numpy as np
import pytest

import dynamics_reference as DR
import implicit_reference as IR
import pfemfort_amd as pf
from pfemfort_amd import _lib as L

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
B, MAX_GRID = 1024, 2048
ONE = MAX_GRID * B
COUNTS = [1, 3, 4, 5, B - 1, B, B + 1, ONE, ONE + 1, 2 * ONE + 3 * B + 4 * 37 + 3]
# both schemes at every count up to a block and a row; the three counts past the grid cap under Newmark, the last also under theta
CASES = [(s, n) for n in COUNTS for s in ("newmark", "theta") if n <= B + 1 or s == "newmark" or n == COUNTS[-1]]
# rows without mass (a share of the rows, and row n - 1): at every count up to a block and a row and at the last
WITH_MASSLESS = [(n, ml) for n in COUNTS for ml in (False, True) if not (ml and ONE <= n < COUNTS[-1])]
RHS_CASES = [(s, n, ml) for s, n in CASES for ml in (False, True) if (n, ml) in WITH_MASSLESS]
SCHEME = {"newmark": dict(scheme="newmark", beta=0.25, gamma=0.5), "theta": dict(scheme="theta", theta=0.5)}      # with dt = 1: sigma 4, 2


def grid(n):
    return min(MAX_GRID, -(-n // B))


_WORST = {}


def note(kernel, n, ratio):
    _WORST[kernel] = max(_WORST.get(kernel, 0.0), float(ratio))
    print(f"{kernel}: n {n}: largest error / bound {float(ratio):.3f} (so far {_WORST[kernel]:.3f})")


def ratio_of(err, bound):
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    assert (err <= bound).all(), float(np.max(err / np.where(bound > 0, bound, 1)))
    return np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0))


@pytest.fixture(scope="module")
def solver():
    assert np.finfo(LD).eps <= 2.0 ** -63
    s = pf.PetscSolver().initialise(8, 8)        # a handle is all the probes need
    yield s
    s.free()


def marked(n):
    rows = np.arange(n)
    return (rows % B == 0) | (rows % B == B - 1) | (rows == n - 1)


def ints(rng, n, count=1, lo=-4, hi=4):
    """`count` vectors of integers in [lo, hi]; no zero in row 0, row n - 1 and the first and last row of every block"""
    mk = marked(n)
    out = []
    for _ in range(count):
        v = rng.integers(lo, hi + 1, n)
        fill = rng.integers(1, hi + 1, n) * (rng.choice([-1, 1], n) if lo < 0 else 1)
        out.append(np.where(mk & (v == 0), fill, v).astype(np.float64))
    return out if count > 1 else out[0]


def reals(rng, n, count=1):
    out = [rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n) for _ in range(count)]
    return out if count > 1 else out[0]


def masses(rng, n, exact, massless):
    """m and the rows without mass: a fixed share of the rows that are not marked, and row n - 1"""
    m = rng.integers(1, 5, n).astype(np.float64) if exact else 10.0 ** rng.uniform(-1, 1, n)
    free = np.zeros(n, bool)
    if massless:
        free = (np.arange(n) % 7 == 3) & ~marked(n)
        free[n - 1] = True
        m[free] = 0.0
    return m, free


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def exact_terms(*terms, unit=2.0 ** -8):
    """every term a multiple of `unit`, every sum of magnitudes below 2^53 units: no sum depends on its order"""
    for t in terms:
        s = np.asarray(t) / unit
        assert np.array_equal(s, np.rint(s)) and np.abs(s).sum() < 2.0 ** 53
    return True


def tail_is_nan(part, used):
    return np.isnan(part[used:]).all() and not np.isnan(part[:used]).any()


def sums_ratio(n, got, terms, blocks):
    """largest error / bound of the blocks' partials `got` against the longdouble sums of the block's own terms"""
    terms = np.asarray(terms, dtype=LD)
    ref, mag = DR.block_sums(terms, blocks), DR.block_sums(np.abs(terms), blocks)
    cnt = DR.block_sums(np.ones(n), blocks)
    return ratio_of(np.abs(got.astype(LD) - ref), (cnt + 3) * EPS * mag)


def total_ratio(n, got, terms):
    terms = np.asarray(terms, dtype=LD)
    return ratio_of(abs(LD(got) - terms.sum()), (n + 3) * EPS * np.abs(terms).sum())


def ctl_of(**kw):
    c = dict(beta=(0.0, 0.0), rn0=0.0, ttol=0.0, rn=0.0, dtol=0.0, alpha=0.0, flag=0, its=0, its_dir=0)
    c.update(kw)
    return c


def same_ctl(a, b):
    return all(same_bits(a[k], b[k]) if k == "beta" or isinstance(b[k], float) else a[k] == b[k] for k in b)


# ---- k_imp_predict, k_imp_correct ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("n", COUNTS)
def test_predict(solver, n, exact):
    rng = np.random.default_rng(100 + n)
    u, v, a = ints(rng, n, 3) if exact else reals(rng, n, 3)
    dt, beta, gamma = (1.0, 0.25, 0.5) if exact else (0.37, 0.3, 0.6)
    P = IR.Par("newmark", dt, beta=beta, gamma=gamma)
    ut, vt = IR.predict(P, u, v, a)
    if exact:
        assert np.array_equal(4 * ut, 4 * u + 4 * v + a) and np.array_equal(2 * vt, 2 * v + a)
    got = solver.stepperProbePredict(dt, u, v, a, beta=beta, gamma=gamma)
    assert same_bits(got[0], ut) and same_bits(got[1], vt)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("scheme,n", CASES)
def test_correct(solver, scheme, n, exact):
    rng = np.random.default_rng(200 + n)
    d, u, ut, vt = ints(rng, n, 4) if exact else reals(rng, n, 4)
    dt = 1.0 if exact else 0.37
    kw = SCHEME[scheme] if exact else dict(scheme=scheme, beta=0.3, gamma=0.6, theta=0.7)
    P = IR.Par(scheme, dt, **{k: v for k, v in kw.items() if k != "scheme"})
    wu, wv, wa = IR.correct(P, d, u=u, ut=ut, vt=vt)
    if exact and scheme == "newmark":
        assert np.array_equal(wa, 4 * d) and np.array_equal(wv, vt + 2 * d)
    gu, gv_, ga = solver.stepperProbeCorrect(dt, d, u=u, ut=ut, vt=vt, **kw)
    assert same_bits(gu, wu) and same_bits(gv_, wv)
    assert same_bits(ga, wa) if scheme == "newmark" else np.isnan(ga).all()         # (the theta-method writes no a)


# ---- k_imp_rhs, k_cg_start -------------------------------------------------------------------------------------------------------------
def rhs_case(scheme, n, exact, massless, seed):
    rng = np.random.default_rng(seed + n)
    f, vt, w = ints(rng, n, 3) if exact else reals(rng, n, 3)
    m, free = masses(rng, n, exact, massless)
    dinv = 2.0 ** rng.integers(-2, 3, n) if exact else 10.0 ** rng.uniform(-2, 2, n)
    dinv[free] = 1.0
    if exact:          # Newmark with damping alpha = 2: sigma = (1 + 1) / (1/4) = 8; lambda = 2 from a curve of one knot
        kw, dt, alpha, curve = SCHEME[scheme], 1.0, 2.0 if scheme == "newmark" else 0.0, ([0.0], [2.0])
    else:
        kw, dt, alpha = dict(scheme=scheme, beta=0.3, gamma=0.6, theta=0.7), 0.37, 0.21 if scheme == "newmark" else 0.0
        curve = ([0.0, 10.0], [0.3, 1.9])
    P = IR.Par(scheme, dt, alpha=alpha, **{k: v for k, v in kw.items() if k != "scheme"})
    lam = IR.rhs_load_factor(P, curve, 0.25, 2)
    b, z = IR.rhs(P, lam, f, m, vt, w, dinv)
    args = dict(vt=vt if scheme == "newmark" else None, alpha=alpha, curve=curve, t_base=0.25, step=2, rtol=1e-5, abstol=1e-50, dtol=1e5, **kw)
    return P, (dt, f, m, w, dinv), args, b, z, free, dinv, m


def rhs_vectors(out, b, z, free, g):
    assert same_bits(out["r"], b) and same_bits(out["p"], z) and same_bits(out["d"], np.zeros_like(b))
    assert not out["r"][free].any() and not np.signbit(out["r"][free]).any()          # a row without mass: b = +0
    assert out["gv"] == g and all(tail_is_nan(out[k], g) for k in ("part_rz", "part_zz", "part_mp"))


@pytest.mark.parametrize("scheme,n,massless", RHS_CASES)
def test_rhs_exact(solver, scheme, n, massless):
    P, vec, args, b, z, free, dinv, m = rhs_case(scheme, n, True, massless, 300)
    if scheme == "newmark":
        assert P.sigma == 8.0
    g = grid(n)
    terms = IR.dot_terms(P, b, dinv, m, z, np.float64)
    assert exact_terms(*terms)
    out = solver.stepperProbeRhs(*vec, **args)
    rhs_vectors(out, b, z, free, g)
    for k, t in zip(("part_rz", "part_zz", "part_mp"), terms):
        assert same_bits(out[k][:g], DR.block_sums(t, g))
    rz, zz = terms[0].sum(), terms[1].sum()
    rn0 = np.sqrt(zz)
    want = ctl_of(beta=(rz, 0.0), rn0=rn0, rn=rn0, ttol=max(1e-5 * rn0, 1e-50), dtol=1e5, flag=3 if rn0 <= 1e-50 else 0)
    assert same_ctl(out["ctl"], {k: want[k] for k in ("beta", "rn0", "rn", "ttol", "dtol", "flag", "its")})
    if massless and n == 1:          # the one row has no mass: b = 0, converged before the first iteration
        assert out["ctl"]["flag"] == 3 and rn0 == 0.0


@pytest.mark.parametrize("scheme,n,massless", RHS_CASES)
def test_rhs_rounding(solver, scheme, n, massless):
    P, vec, args, b, z, free, dinv, m = rhs_case(scheme, n, False, massless, 400)
    g = grid(n)
    out = solver.stepperProbeRhs(*vec, **args)
    rhs_vectors(out, b, z, free, g)
    terms = IR.dot_terms(P, b, dinv, m, z)
    worst = max(sums_ratio(n, out[k][:g], t, g) for k, t in zip(("part_rz", "part_zz", "part_mp"), terms))
    c = out["ctl"]
    worst = max(worst, total_ratio(n, c["beta"][0], terms[0]))
    nz = np.sqrt(terms[1].sum())
    worst = max(worst, ratio_of(abs(LD(c["rn0"]) - nz), ((n + 3) / 2 + 1) * EPS * nz))
    assert same_bits(c["rn"], c["rn0"]) and same_bits(c["ttol"], max(1e-5 * c["rn0"], 1e-50)) and c["flag"] == (3 if c["rn0"] <= 1e-50 else 0)
    note(f"k_imp_rhs {scheme}", n, worst)
    again = solver.stepperProbeRhs(*vec, **args)
    assert all(same_bits(again[k], out[k]) for k in ("d", "r", "p", "part_rz", "part_zz", "part_mp")) and same_ctl(again["ctl"], c)


# ---- k_imp_update ------------------------------------------------------------------------------------------------------------------------
N_PW = [1, 255, 256, 257, MAX_GRID]          # the folded scalar, one trip of sum_partials less one, one trip, two, the cap


def update_case(scheme, n, exact, seed):
    rng = np.random.default_rng(seed + n)
    p, w, r = ints(rng, n, 3) if exact else reals(rng, n, 3)
    m, _ = masses(rng, n, exact, False)
    dinv = 2.0 ** rng.integers(-2, 3, n) if exact else 10.0 ** rng.uniform(-2, 2, n)
    g, n_pw = grid(n), N_PW[COUNTS.index(n) % len(N_PW)]
    part_mp = rng.integers(0, 9, g).astype(np.float64)
    part_pw = rng.integers(-8, 9, n_pw).astype(np.float64)
    it = 3
    if exact:          # (p, Ap) = 2^22 whatever the partials hold, beta = alpha 2^22 with alpha 1/2, 1 or 2
        pw, alpha = 2.0 ** 22, [0.5, 1.0, 2.0][COUNTS.index(n) % 3]
        beta = alpha * pw
    else:              # integer partials: their sum is exact, alpha one float64 division
        pw, beta = 2.0 ** 22 + 7.0, 3.0e5
        alpha = beta / pw
    part_pw[-1] += pw - (part_pw.sum() + part_mp.sum())
    assert part_pw.sum() + part_mp.sum() == pw
    ctl = ctl_of(beta=(-99.0, beta), rn0=5.0, ttol=1e-3, rn=4.0, dtol=1e5, alpha=-77.0, its=it, its_dir=-5)
    kw = SCHEME[scheme] if exact else dict(scheme=scheme, beta=0.3, gamma=0.6, theta=0.7)
    dt = 1.0 if exact else 0.37
    P = IR.Par(scheme, dt, **{k: v for k, v in kw.items() if k != "scheme"})
    return P, dt, kw, ctl, it, alpha, part_pw, part_mp, (p, w, m, dinv, r), g


@pytest.mark.parametrize("scheme,n", CASES)
def test_update_exact(solver, scheme, n):
    P, dt, kw, ctl, it, alpha, part_pw, part_mp, (p, w, m, dinv, r), g = update_case(scheme, n, True, 500)
    assert P.sigma == (4.0 if scheme == "newmark" else 2.0)
    want_r = r - alpha * ((P.sigma * m) * p + w)
    terms = IR.dot_terms(P, want_r, dinv, m, p, np.float64)[:2]
    assert exact_terms(want_r, *terms)
    got_r, prz, pzz, c = solver.stepperProbeUpdate(dt, ctl, it, part_pw, part_mp, p, w, m, dinv, r, **kw)
    assert same_bits(got_r, want_r)
    assert tail_is_nan(prz, g) and tail_is_nan(pzz, g)
    assert same_bits(prz[:g], DR.block_sums(terms[0], g)) and same_bits(pzz[:g], DR.block_sums(terms[1], g))
    assert same_ctl(c, dict(ctl, alpha=alpha, its_dir=it))
    # the form of a replayed graph: the iteration index from the control block
    other = solver.stepperProbeUpdate(dt, ctl, -1, part_pw, part_mp, p, w, m, dinv, r, **kw)
    assert same_bits(other[0], got_r) and same_bits(other[1], prz) and same_bits(other[2], pzz) and same_ctl(other[3], c)


@pytest.mark.parametrize("scheme,n", CASES)
def test_update_rounding(solver, scheme, n):
    P, dt, kw, ctl, it, alpha, part_pw, part_mp, (p, w, m, dinv, r), g = update_case(scheme, n, False, 600)
    got_r, prz, pzz, c = solver.stepperProbeUpdate(dt, ctl, it, part_pw, part_mp, p, w, m, dinv, r, **kw)
    assert same_ctl(c, dict(ctl, alpha=alpha, its_dir=it))
    ref, mag = IR.update(P, alpha, p, w, m, r)
    worst_r = ratio_of(np.abs(got_r.astype(LD) - ref), EPS * mag)
    terms = IR.dot_terms(P, got_r, dinv, m, p)[:2]
    assert tail_is_nan(prz, g) and tail_is_nan(pzz, g)
    note(f"k_imp_update {scheme}: r'", n, worst_r)
    note(f"k_imp_update {scheme}: sums", n, max(sums_ratio(n, prz[:g], terms[0], g), sums_ratio(n, pzz[:g], terms[1], g)))
    again = solver.stepperProbeUpdate(dt, ctl, it, part_pw, part_mp, p, w, m, dinv, r, **kw)
    assert same_bits(again[0], got_r) and same_bits(again[1], prz) and same_bits(again[2], pzz)


# ---- k_imp_direction ---------------------------------------------------------------------------------------------------------------------
def direction_case(scheme, n, exact, seed):
    rng = np.random.default_rng(seed + n)
    r, p, d = ints(rng, n, 3) if exact else reals(rng, n, 3)
    m, _ = masses(rng, n, exact, False)
    dinv = 2.0 ** rng.integers(-2, 3, n) if exact else 10.0 ** rng.uniform(-2, 2, n)
    g, it = grid(n), 3
    part_rz = rng.integers(0, 9, g).astype(np.float64)
    part_zz = rng.integers(0, 9, g).astype(np.float64)
    part_rz[-1] += 2.0 ** 20 - part_rz.sum()
    part_zz[-1] += 2.0 ** 24 + 5.0 - part_zz.sum()
    rz, zz = 2.0 ** 20, 2.0 ** 24 + 5.0
    if exact:
        bb, alpha = [0.5, 1.0, 2.0][COUNTS.index(n) % 3], [2.0, 0.5, 1.0][COUNTS.index(n) % 3]
        beta_old = rz / bb
    else:
        beta_old, alpha = 3.0e5, 0.37
        bb = rz / beta_old
    ctl = ctl_of(beta=(-99.0, beta_old), rn0=5000.0, ttol=1e-3, rn=-1.0, dtol=1e5, alpha=alpha, its=it, its_dir=it)
    kw = SCHEME[scheme] if exact else dict(scheme=scheme, beta=0.3, gamma=0.6, theta=0.7)
    dt = 1.0 if exact else 0.37
    P = IR.Par(scheme, dt, **{k: v for k, v in kw.items() if k != "scheme"})
    want = dict(ctl, beta=(rz, beta_old), rn=np.sqrt(zz), flag=0, its=it + 1)
    return P, dt, kw, ctl, want, it, alpha, bb, part_rz, part_zz, (r, dinv, m, p, d), g


@pytest.mark.parametrize("scheme,n", CASES)
def test_direction_exact(solver, scheme, n):
    P, dt, kw, ctl, want, it, alpha, bb, part_rz, part_zz, (r, dinv, m, p, d), g = direction_case(scheme, n, True, 700)
    want_d, want_p = d + alpha * p, bb * p + r * dinv
    terms = IR.dot_terms(P, r, dinv, m, want_p, np.float64)[2]
    assert exact_terms(want_d, want_p, terms)
    gp, gd, pmp, c = solver.stepperProbeDirection(dt, ctl, it, part_rz, part_zz, r, dinv, m, p, d, 10000, **kw)
    assert same_bits(gp, want_p) and same_bits(gd, want_d)
    assert tail_is_nan(pmp, g) and same_bits(pmp[:g], DR.block_sums(terms, g))
    assert same_ctl(c, want)
    other = solver.stepperProbeDirection(dt, ctl, -1, part_rz, part_zz, r, dinv, m, p, d, 10000, **kw)
    assert same_bits(other[0], gp) and same_bits(other[1], gd) and same_bits(other[2], pmp) and same_ctl(other[3], c)


@pytest.mark.parametrize("scheme,n", CASES)
def test_direction_rounding(solver, scheme, n):
    P, dt, kw, ctl, want, it, alpha, bb, part_rz, part_zz, (r, dinv, m, p, d), g = direction_case(scheme, n, False, 800)
    gp, gd, pmp, c = solver.stepperProbeDirection(dt, ctl, it, part_rz, part_zz, r, dinv, m, p, d, 10000, **kw)
    assert same_ctl(c, want)
    ref_d, ref_p, mag = IR.direction(alpha, bb, r, dinv, p, d)
    note(f"k_imp_direction {scheme}: d'", n, ratio_of(np.abs(gd.astype(LD) - ref_d), EPS * np.abs(ref_d)))
    note(f"k_imp_direction {scheme}: p'", n, ratio_of(np.abs(gp.astype(LD) - ref_p), EPS * mag))
    assert tail_is_nan(pmp, g)
    note(f"k_imp_direction {scheme}: sum", n, sums_ratio(n, pmp[:g], IR.dot_terms(P, r, dinv, m, gp)[2], g))
    again = solver.stepperProbeDirection(dt, ctl, it, part_rz, part_zz, r, dinv, m, p, d, 10000, **kw)
    assert same_bits(again[0], gp) and same_bits(again[1], gd) and same_bits(again[2], pmp)


# ---- verdicts ------------------------------------------------------------------------------------------------------------------------------
def all_nan(a):
    return np.isnan(a).all()


@pytest.mark.parametrize("n", [5, B + 1])
def test_update_verdicts(solver, n):
    P, dt, kw, ctl, it, alpha, part_pw, part_mp, vec, g = update_case("newmark", n, True, 900)
    p, w, m, dinv, r = vec
    # finished in an earlier iteration of this graph unit: its_dir = -2, nothing else
    done = dict(ctl, flag=2)
    gr, prz, pzz, c = solver.stepperProbeUpdate(dt, done, -1, part_pw, part_mp, *vec, **kw)
    assert same_ctl(c, dict(done, its_dir=-2)) and same_bits(gr, r) and all_nan(prz) and all_nan(pzz)
    # (p, Ap) <= 0 (zero, then negative): the breakdown signal in every block, r untouched, no alpha
    for shift in (2.0 ** 22, 2.0 ** 23):
        bad = part_pw.copy()
        bad[0] -= shift
        assert bad.sum() + part_mp.sum() == 2.0 ** 22 - shift
        gr, prz, pzz, c = solver.stepperProbeUpdate(dt, ctl, it, bad, part_mp, *vec, **kw)
        assert same_bits(gr, r) and same_ctl(c, dict(ctl, its_dir=it))
        assert same_bits(prz[:g], np.zeros(g)) and same_bits(pzz[:g], -np.ones(g)) and all_nan(prz[g:]) and all_nan(pzz[g:])


@pytest.mark.parametrize("n", [5, B + 1])
def test_direction_verdicts(solver, n):
    P, dt, kw, ctl, want, it, alpha, bb, part_rz, part_zz, vec, g = direction_case("newmark", n, True, 950)
    r, dinv, m, p, d = vec
    run = lambda c, prz=part_rz, pzz=part_zz, maxits=10000, it_arg=it: solver.stepperProbeDirection(dt, c, it_arg, prz, pzz, *vec, maxits, **kw)
    # after the update's breakdown signal: -10 with its = it + 1, vectors untouched
    gp, gd, pmp, c = run(ctl, np.zeros(g), -np.ones(g))
    assert same_ctl(c, dict(ctl, flag=-10, its=it + 1)) and same_bits(gp, p) and same_bits(gd, d) and all_nan(pmp)
    # finished in an earlier iteration of this graph unit (the update left its_dir = -2): nothing is written
    done = dict(ctl, flag=2, its=2, its_dir=-2)
    gp, gd, pmp, c = run(done, it_arg=-1)
    assert same_ctl(c, done) and same_bits(gp, p) and same_bits(gd, d) and all_nan(pmp)
    # the four verdicts of this iteration: d += alpha p is done, p and the partials are not
    rn = np.sqrt(2.0 ** 24 + 5.0)
    neg = part_rz.copy()
    neg[0] -= 2.0 ** 21
    cases = [(2, dict(ctl, ttol=rn), part_rz, 10000), (-4, dict(ctl, rn0=rn / 2e5), part_rz, 10000), (-8, ctl, neg, 10000), (-3, ctl, part_rz, it + 1)]
    for flag, c_in, prz, maxits in cases:
        gp, gd, pmp, c = run(c_in, prz, maxits=maxits)
        assert c["flag"] == flag and c["its"] == it + 1 and same_bits(c["rn"], rn) and same_bits(c["beta"][0], prz.sum())
        assert same_bits(gd, d + alpha * p) and same_bits(gp, p) and all_nan(pmp)
        other = run(dict(c_in), prz, maxits=maxits, it_arg=-1)
        assert same_ctl(other[3], c) and same_bits(other[1], gd) and same_bits(other[0], gp) and all_nan(other[2])
    # one short of each bound: the iteration goes on
    gp, gd, pmp, c = run(dict(ctl, ttol=np.nextafter(rn, 0.0)), maxits=it + 2)
    assert c["flag"] == 0 and not same_bits(gp, p) and tail_is_nan(pmp, g)


# ---- k_imp_energy, k_imp_row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("scheme,n", CASES)
def test_energy(solver, scheme, n, exact):
    rng = np.random.default_rng(1000 + n)
    f, u, v, w = ints(rng, n, 4) if exact else reals(rng, n, 4)
    m, _ = masses(rng, n, exact, False)
    P = IR.Par(scheme, 1.0, theta=0.5)
    probes = [0, n - 1, n // 2]
    g = grid(n)
    row, part = solver.stepperProbeEnergy(f, m, u, v, w, scheme=scheme, probes=probes, t=1.75)
    assert part.shape == (3, g) and row[0] == 1.75 and same_bits(row[4:7], u[probes]) and same_bits(row[7:], v[probes])
    if exact:
        terms = IR.energy_terms(P, f, m, u, v, w, np.float64)
        assert exact_terms(*terms)
        assert all(same_bits(part[k], DR.block_sums(terms[k], g)) for k in range(3))
        assert same_bits(row[1:4], [0.5 * terms[0].sum(), 0.5 * terms[1].sum(), terms[2].sum()])
    else:
        terms = IR.energy_terms(P, f, m, u, v, w)
        worst = max(sums_ratio(n, part[k], terms[k], g) for k in range(3))
        worst = max(worst, *(total_ratio(n, row[1 + k] * s, terms[k]) for k, s in enumerate((2.0, 2.0, 1.0))))
        note(f"k_imp_energy {scheme}", n, worst)
        again = solver.stepperProbeEnergy(f, m, u, v, w, scheme=scheme, probes=probes, t=1.75)
        assert same_bits(again[0], row) and same_bits(again[1], part)


# ---- k_dyn_step, k_dyn_flush ----------------------------------------------------------------------------------------------------------------
def step_case(n, exact, massless, seed):
    rng = np.random.default_rng(seed + n)
    f, w, u, up = ints(rng, n, 4) if exact else reals(rng, n, 4)
    if exact:          # dt = 1, alpha = 2: c0 = c1 = 1, c0 + c1 = 2; 1 / m a power of two; lambda = 2 from a curve of one knot
        minv = 2.0 ** rng.integers(-2, 1, n)
        m = 1.0 / minv
        dt, alpha, t0, curve = 1.0, 2.0, 0.5, ([0.0], [2.0])
    else:
        m = 10.0 ** rng.uniform(-1, 1, n)
        minv = 1.0 / m
        dt, alpha, t0, curve = 0.37, 0.21, 0.5, ([0.0, 10.0], [0.3, 1.9])
    free = np.zeros(n, bool)
    if massless:
        free = (np.arange(n) % 7 == 3) & ~marked(n)
        free[n - 1] = True
        m[free], minv[free] = 0.0, 0.0
    return (dt, f, m, minv, w, u, up), dict(alpha=alpha, t0=t0, curve=curve), free


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("n,massless", WITH_MASSLESS)
def test_explicit_step(solver, n, massless, exact):
    vec, kw, free = step_case(n, exact, massless, 1100 + (0 if exact else 50))
    dt, f, m, minv, w, u, up = vec
    nb = -(-n // B)
    probes = [0, n - 1, n // 2]
    worst = 0.0
    # both parities of the partials and of the counter; past the cap one parity a count, to keep the case short
    for step in ((4, 5) if n <= B + 1 else (4 + COUNTS.index(n) % 2,)):
        par = step & 1
        lam = DR.load_factor(kw["curve"], kw["t0"] + float(step) * dt)
        x, tT, tS, tW = DR.step_kernel(dt, kw["alpha"], lam, f, m, minv, w, u, up)
        c0, c1, a = DR.step_par(dt, kw["alpha"])
        inert = ((2.0 * u - up) * c0 + c1 * up) / a
        assert np.array_equal(x[free], (inert + 0.0)[free])                      # a row without mass keeps its inertia terms only
        if exact:
            assert lam == 2.0 and exact_terms(x, tT, tS, tW)
        # a sampled step: the third of a run that began at step - 2
        ctl_in = [-7, -7]
        un, row, part, cs = solver.stepperProbeStep(*vec, step=step, run_start=step - 2, sample_every=3, probes=probes, ctl_step=ctl_in, **kw)
        assert same_bits(un, x) and part.shape == (3, nb) and row is not None
        assert cs[par ^ 1] == step + 1 and cs[par] == -7
        ref_row = DR.step_row(kw["t0"], dt, step, 0.0, 0.0, 0.0, x, u, probes)
        assert same_bits(row[0], ref_row[0]) and same_bits(row[4:], ref_row[4:])
        if exact:
            assert all(same_bits(part[k], DR.block_sums(t, nb)) for k, t in enumerate((tT, tS, tW)))
            assert same_bits(row[1:4], [0.5 * tT.sum(), 0.5 * tS.sum(), tW.sum()])
        else:
            terms = DR.step_terms_ld(dt, x, f, m, w, u)
            worst = max(worst, *(sums_ratio(n, part[k], terms[k], nb) for k in range(3)))
            worst = max(worst, *(total_ratio(n, row[1 + k] * s, terms[k]) for k, s in enumerate((2.0, 2.0, 1.0))))
        # the step index from the control block, as in a replayed graph: the same bits
        ctl_in[par] = step
        other = solver.stepperProbeStep(*vec, step=step, run_start=step - 2, sample_every=3, probes=probes, use_ctl=True, ctl_step=ctl_in, **kw)
        assert same_bits(other[0], un) and same_bits(other[1], row) and same_bits(other[2], part)
        assert other[3][par ^ 1] == step + 1 and other[3][par] == step
        # a step that is not sampled: no partials, no row (at the small counts and the last; the vectors are the same)
        if n <= B + 1 or n == COUNTS[-1]:
            for every in (4, 0):
                un2, row2, part2, cs2 = solver.stepperProbeStep(*vec, step=step, run_start=step - 2, sample_every=every, probes=probes, **kw)
                assert same_bits(un2, x) and row2 is None and all_nan(part2) and cs2[par ^ 1] == step + 1 and cs2[par] == -7
    if not exact:
        note("k_dyn_step", n, worst)


# ---- the load curve ---------------------------------------------------------------------------------------------------------------------------
CURVES = [None, ([1.0], [0.3]), ([1.0, 4.0], [0.3, 5.3]), ([1.0, 1.5, 2.5, 3.0, 4.0], [0.3, -1.7, 2.9, 0.1, 5.3])]


@pytest.mark.parametrize("curve", CURVES, ids=["0", "1", "2", "5"])
def test_load_curve(solver, curve):
    """dt = 1/2 from t_base = 0: the times 0.5 .. 5.0 lie before the first knot, on it, on the interior knots, between two, on
    the last and behind it; from t_base = 1/8 strictly between knots at uneven fractions.  w = 0: b = lambda f and
    u_{n+1} = lambda f / c0 show lambda(t) itself."""
    n, dt = 5, 0.5
    rng = np.random.default_rng(7)
    f = reals(rng, n)
    one, zero = np.ones(n), np.zeros(n)
    seen = set()
    for t_base in (0.0, 0.125):
        for step in range(10):
            for scheme in ("newmark", "theta"):
                kw = dict(scheme=scheme, beta=0.25, gamma=0.5, theta=0.5)
                P = IR.Par(scheme, dt, theta=0.5)
                lam = IR.rhs_load_factor(P, curve, t_base, step)
                b, z = IR.rhs(P, lam, f, one, zero, zero, one)
                out = solver.stepperProbeRhs(dt, f, one, zero, one, vt=zero, curve=curve, t_base=t_base, step=step, **kw)
                assert same_bits(out["r"], b) and same_bits(out["r"], lam * f)
            t = t_base + float(step) * dt
            lam = DR.load_factor(curve, t)
            x = DR.step_kernel(dt, 0.0, lam, f, one, one, zero, zero, zero)[0]
            un = solver.stepperProbeStep(dt, f, one, one, zero, zero, zero, t0=t_base, curve=curve, step=step, run_start=0)[0]
            assert same_bits(un, x)
            if curve is not None and len(curve[0]) > 1:
                ct = np.array(curve[0])
                seen.add("before" if t < ct[0] else "first" if t == ct[0] else "after" if t > ct[-1] else "last" if t == ct[-1] else
                         "knot" if t in ct else "between")
    if curve is not None and len(curve[0]) > 1:
        assert seen == {"before", "first", "between", "last", "after"} | ({"knot"} if len(curve[0]) > 2 else set())


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_probe_arguments(solver):
    z = np.zeros(2 * MAX_GRID)
    p = z.ctypes.data
    lib, h = L.lib(), solver._h
    c = L.CgCtl()
    gv, have, nb = C.c_int(0), C.c_int(0), C.c_int(0)
    cs = (C.c_int64 * 2)(0, 0)
    N, T = L.SCHEME_NEWMARK, L.SCHEME_THETA
    pr = (p,) * 13
    for hh, scheme, n in ((h, N, 0), (h, N, -1), (None, N, 4), (h, 0, 4), (h, 3, 4)):
        if scheme == N:
            assert lib.pfem_imp_probe_predict(hh, n, 1.0, 0.25, 0.5, p, p, p, p, p) == L.ERR_ARG
            assert lib.pfem_dyn_probe_step(hh, n, 1.0, 0.0, 0.0, 0, None, None, 0, 0, 0, 0, None, 0, p, p, p, p, p, p, p, p, C.byref(have), p, C.byref(nb),
                                           cs) == L.ERR_ARG
        assert lib.pfem_imp_probe_rhs(hh, scheme, n, 1.0, 0.25, 0.5, 0.0, 0, None, None, 0.0, 0, 1e-5, 1e-50, 1e5, *pr[:11], C.byref(gv), C.byref(c)) == L.ERR_ARG
        assert lib.pfem_imp_probe_update(hh, scheme, n, 1.0, 0.25, 0.5, 0.0, C.byref(c), 0, 1, p, 1, *pr[:8]) == L.ERR_ARG
        assert lib.pfem_imp_probe_direction(hh, scheme, n, 1.0, 0.25, 0.5, 0.0, C.byref(c), 0, 1, *pr[:7], 10, p) == L.ERR_ARG
        assert lib.pfem_imp_probe_correct(hh, scheme, n, 1.0, 0.25, 0.5, 0.0, p, p, p, p, p, p) == L.ERR_ARG
        assert lib.pfem_imp_probe_energy(hh, scheme, n, p, p, p, p, p, 0, None, 0.0, p, p, C.byref(gv)) == L.ERR_ARG
    # null vectors, a partial count that is not the grid's, parameters the run refuses, a probe row outside the vector
    assert lib.pfem_imp_probe_predict(h, 4, 1.0, 0.25, 0.5, p, None, p, p, p) == L.ERR_ARG
    assert lib.pfem_imp_probe_predict(h, 4, 0.0, 0.25, 0.5, p, p, p, p, p) == L.ERR_ARG
    assert lib.pfem_imp_probe_rhs(h, N, 4, 1.0, 0.25, 0.5, 0.0, 0, None, None, 0.0, 0, 1e-5, 1e-50, 1e5, p, p, None, *pr[:8], C.byref(gv), C.byref(c)) == L.ERR_ARG
    assert lib.pfem_imp_probe_rhs(h, T, 4, 1.0, 0.5, 0.0, 0.1, 0, None, None, 0.0, 0, 1e-5, 1e-50, 1e5, *pr[:11], C.byref(gv), C.byref(c)) == L.ERR_ARG
    assert lib.pfem_imp_probe_rhs(h, N, 4, 1.0, 0.25, 0.5, 0.0, 2, p, None, 0.0, 0, 1e-5, 1e-50, 1e5, *pr[:11], C.byref(gv), C.byref(c)) == L.ERR_ARG
    assert lib.pfem_imp_probe_update(h, N, 4, 1.0, 0.25, 0.5, 0.0, None, 0, 1, p, 1, *pr[:8]) == L.ERR_ARG
    assert lib.pfem_imp_probe_update(h, N, 4, 1.0, 0.25, 0.5, 0.0, C.byref(c), 0, 1, p, 2, *pr[:8]) == L.ERR_ARG
    assert lib.pfem_imp_probe_update(h, N, 4, 1.0, 0.25, 0.5, 0.0, C.byref(c), 0, 0, p, 1, *pr[:8]) == L.ERR_ARG
    assert lib.pfem_imp_probe_update(h, N, 4, 1.0, 0.25, 0.5, 0.0, C.byref(c), -2, 1, p, 1, *pr[:8]) == L.ERR_ARG
    assert lib.pfem_imp_probe_direction(h, N, 2 * B, 1.0, 0.25, 0.5, 0.0, C.byref(c), 0, 1, *pr[:7], 10, p) == L.ERR_ARG
    assert lib.pfem_imp_probe_correct(h, N, 4, 1.0, 0.25, 0.5, 0.0, None, p, p, p, p, p) == L.ERR_ARG
    bad = (C.c_int32 * 1)(4)
    assert lib.pfem_imp_probe_energy(h, N, 4, p, p, p, p, p, 1, bad, 0.0, p, p, C.byref(gv)) == L.ERR_ARG
    assert lib.pfem_imp_probe_energy(h, N, 4, p, p, p, p, p, 1, None, 0.0, p, p, C.byref(gv)) == L.ERR_ARG
    step = lambda *a: lib.pfem_dyn_probe_step(h, 4, *a, p, p, p, p, p, p, p, p, C.byref(have), p, C.byref(nb), cs)
    assert step(1.0, 0.0, 0.0, 0, None, None, 0, 0, 0, 1, bad, 0) == L.ERR_ARG
    assert step(1.0, 0.0, 0.0, 0, None, None, 2, 3, 0, 0, None, 0) == L.ERR_ARG          # run_start behind the step
    assert step(1.0, -1.0, 0.0, 0, None, None, 0, 0, 0, 0, None, 0) == L.ERR_ARG
    assert step(0.0, 0.0, 0.0, 0, None, None, 0, 0, 0, 0, None, 0) == L.ERR_ARG
    assert step(1.0, 0.0, 0.0, 1, None, p, 0, 0, 0, 0, None, 0) == L.ERR_ARG
    assert step(1.0, 0.0, 0.0, 0, None, None, 100, 0, 1, 0, None, 0) == L.ERR_ARG        # more history rows than a probe holds
    assert lib.pfem_dyn_probe_step(h, 4, 1.0, 0.0, 0.0, 0, None, None, 0, 0, 0, 0, None, 0, p, p, p, p, p, None, p, p, C.byref(have), p, C.byref(nb),
                                   cs) == L.ERR_ARG
    with pytest.raises(ValueError):
        solver.stepperProbePredict(1.0, np.zeros(3), np.zeros(4), np.zeros(3))
    with pytest.raises(ValueError):
        solver.stepperProbeCorrect(1.0, np.zeros(3), scheme="euler")
