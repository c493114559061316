"""One launch of each kernel of the modal analysis (pfem_modal_probe_gram / _residual / _update) against a
plain evaluation of the same operation, at row counts on both sides of every point where the kernel takes another path: one
row, a tile less one row, a tile, a tile and a row, the last row count one pass of the capped grid covers, one more, and a
count at which some blocks take three trips and others two with a partial last tile.  The meshes of test_gpu_modal.py end at
2 112 rows -- one trip of every loop --, and LOBPCG converges on a roughly right Gram matrix; here nothing is hidden.

Exact data.  Small integers (blocks in [-4, 4], m in [1, 4], theta and the coefficients in [-2, 2], dinv a power of two): every
product and every partial sum is an integer below 2^53, so the result does not depend on the order of the sums and the device
must equal numpy's int64 evaluation bit for bit.  The first and last row of every tile (and the last row of all) hold no zero,
so that a dropped or doubled row changes the diagonal of G_M, every column norm and its own entries of the update.

Rounding data.  Standard normals times 10**uniform(-3, 3) per row, against numpy longdouble on the same float64 inputs.  The
bounds are those of the operation, with eps = 2^-52:
  Gram entry (a, b)  (n + 2) eps sum_i |s_ia| |k_ib| for G_K, (n + 2) eps sum_i m_i |s_ia| |s_ib| for G_M: an n-term fma sum in
                     any order gives n eps, the rounded m_i s_ib one more;
  W of the residual  the bits of numpy's float64 dinv * (kx - (m * x) * theta): elementwise IEEE operations, no contraction;
  norms              (n + 1) eps x the longdouble sum of the squares of those float64 values;
  update             P': 2 mb eps sum_k |s_k c_k| over the W and P terms; X': (3 mb + 1) eps sum_k |s_k c_k| over all terms.
The largest error / bound per kernel and block size is printed."""
import ctypes as C

import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import _lib as L

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
MBS = [4, 8, 16]
GRAM_TILE, GRAM_BLOCKS, VEC_BLOCKS, BLOCK = 32, 256, 1024, 256       # pfem_modal_kernels.hpp
GRAM_ONE_PASS = GRAM_TILE * GRAM_BLOCKS                              # 8 192 rows
GRAM_N = [1, 31, 32, 33, GRAM_ONE_PASS, GRAM_ONE_PASS + 1, 2 * GRAM_ONE_PASS + 32 + 7]


def residual_n(mb):
    T = VEC_BLOCKS * BLOCK // mb
    return [1, 63, T, T + 1, 2 * T + 77]


def update_n(mb):
    T, TR = VEC_BLOCKS * BLOCK // mb, BLOCK // mb
    return [1, TR - 1, TR, TR + 1, T, T + 1, 2 * T + TR // 2 + 1]


RESIDUAL = [(mb, n) for mb in MBS for n in residual_n(mb)]
UPDATE = [(mb, n) for mb in MBS for n in update_n(mb)]
GRAM = [(mb, n) for mb in MBS for n in GRAM_N]

_WORST = {}


def note(kernel, mb, n, ratio):
    key = (kernel, mb)
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))
    print(f"{kernel}: MB {mb}, n {n}: largest error / bound {ratio:.3f} (so far at this MB {_WORST[key]:.3f})")


def ratio_of(err, bound):
    assert (err <= bound).all()
    return np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0))


@pytest.fixture(scope="module")
def solver():
    s = pf.PetscSolver().initialise(8, 8)        # a handle is all the probes need
    yield s
    s.free()


def int_blocks(rng, count, n, mb, tile):
    """`count` blocks of integers in [-4, 4]; no zero in the first and last row of a tile or in the last row"""
    rows = np.arange(n)
    marked = (rows % tile == 0) | (rows % tile == tile - 1) | (rows == n - 1)
    out = []
    for _ in range(count):
        B = rng.integers(-4, 5, (n, mb))
        fill = rng.integers(1, 5, (n, mb)) * rng.choice([-1, 1], (n, mb))
        out.append(np.where(marked[:, None] & (B == 0), fill, B).astype(np.int64))
    return out


def real_blocks(rng, count, n, mb):
    return [rng.standard_normal((n, mb)) * 10.0 ** rng.uniform(-3, 3, (n, 1)) for _ in range(count)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def computed(mb):
    """the entries of a Gram matrix the kernel computes: the 3 x 3 tiles on and above the diagonal"""
    t = np.arange(3 * mb) // 3
    return t[:, None] <= t[None, :]


# ---- k_modal_gram, k_modal_sum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb,n", GRAM)
def test_gram_exact(solver, mb, n):
    rng = np.random.default_rng(1000 * mb + n)
    X, W, P, KX, KW, KP = int_blocks(rng, 6, n, mb, GRAM_TILE)
    m = rng.integers(1, 5, n).astype(np.int64)
    S, K = np.hstack([X, W, P]), np.hstack([KX, KW, KP])
    up = computed(mb)
    want_k, want_m = np.where(up, S.T @ K, 0), np.where(up, S.T @ (m[:, None] * S), 0)
    assert np.abs(want_k).max() < 2 ** 53 and (np.diag(want_m) > 0).all()
    gk, gm = solver.modalProbeGram(X, W, P, KX, KW, KP, m)
    assert same_bits(gk, want_k) and same_bits(gm, want_m)                  # (the tiles below the diagonal: +0.0)


@pytest.mark.parametrize("mb,n", GRAM)
def test_gram_rounding(solver, mb, n):
    rng = np.random.default_rng(2000 * mb + n)
    B = real_blocks(rng, 6, n, mb)
    m = 10.0 ** rng.uniform(-1, 1, n)
    S, K = np.hstack(B[:3]).astype(LD), np.hstack(B[3:]).astype(LD)
    mS = m.astype(LD)[:, None] * S
    up = computed(mb)
    gk, gm = solver.modalProbeGram(*B, m)
    worst = 0.0
    for got, ref, mag in ((gk, S.T @ K, np.abs(S).T @ np.abs(K)), (gm, S.T @ mS, np.abs(S).T @ np.abs(mS))):
        assert (got[~up] == 0.0).all() and not np.signbit(got[~up]).any()
        worst = max(worst, ratio_of(np.abs(got.astype(LD) - ref)[up], ((n + 2) * EPS * mag)[up]))
    note("k_modal_gram", mb, n, worst)
    again = solver.modalProbeGram(*B, m)
    assert same_bits(again[0], gk) and same_bits(again[1], gm)


# ---- k_modal_residual, k_modal_sum -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dinv", [True, False])
@pytest.mark.parametrize("mb,n", RESIDUAL)
def test_residual_exact(solver, mb, n, with_dinv):
    rng = np.random.default_rng(3000 * mb + n)
    KX, X = int_blocks(rng, 2, n, mb, BLOCK // mb)
    m = rng.integers(1, 5, n).astype(np.int64)
    theta = rng.integers(-2, 3, mb).astype(np.int64)
    dinv = 2.0 ** rng.integers(-2, 3, n) if with_dinv else None
    MX = m[:, None] * X
    R = KX - MX * theta[None, :]
    want_w = R.astype(np.float64) * (dinv[:, None] if with_dinv else 1.0)
    want_norms = np.stack([(R * R).sum(0), (KX * KX).sum(0), (MX * MX).sum(0)])
    assert want_norms.max() < 2 ** 53 and (want_norms[1:] > 0).all()
    Wd, norms = solver.modalProbeResidual(KX, X, m, theta, dinv)
    assert same_bits(Wd, want_w) and same_bits(norms, want_norms)


@pytest.mark.parametrize("with_dinv", [True, False])
@pytest.mark.parametrize("mb,n", RESIDUAL)
def test_residual_rounding(solver, mb, n, with_dinv):
    rng = np.random.default_rng(4000 * mb + n)
    KX, X = real_blocks(rng, 2, n, mb)
    m = 10.0 ** rng.uniform(-1, 1, n)
    theta = rng.standard_normal(mb)
    dinv = 10.0 ** rng.uniform(-2, 2, n) if with_dinv else None
    MX = m[:, None] * X
    R = KX - MX * theta[None, :]
    want_w = dinv[:, None] * R if with_dinv else R
    Wd, norms = solver.modalProbeResidual(KX, X, m, theta, dinv)
    assert same_bits(Wd, want_w)
    ref = np.stack([(v.astype(LD) ** 2).sum(0) for v in (R, KX, MX)])
    note("k_modal_residual", mb, n, ratio_of(np.abs(norms.astype(LD) - ref), (n + 1) * EPS * ref))
    again = solver.modalProbeResidual(KX, X, m, theta, dinv)
    assert same_bits(again[0], Wd) and same_bits(again[1], norms)


# ---- k_modal_update -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb,n", UPDATE)
def test_update_exact(solver, mb, n):
    rng = np.random.default_rng(5000 * mb + n)
    B = int_blocks(rng, 6, n, mb, BLOCK // mb)
    coef = rng.integers(-2, 3, (3 * mb, mb)).astype(np.int64)
    coef[np.arange(3 * mb), np.arange(3 * mb) % mb] = rng.choice([-2, -1, 1, 2], 3 * mb)       # no block of C without a say
    got = solver.modalProbeUpdate(coef, *B)
    for x, w, p, gx, gw, gp in ((0, 1, 2) + got[:3], (3, 4, 5) + got[3:]):
        want_p = B[w] @ coef[mb:2 * mb] + B[p] @ coef[2 * mb:]
        want_x = B[x] @ coef[:mb] + want_p
        assert same_bits(gp, want_p) and same_bits(gx, want_x)
        assert same_bits(gw, B[w])


@pytest.mark.parametrize("mb,n", UPDATE)
def test_update_rounding(solver, mb, n):
    rng = np.random.default_rng(6000 * mb + n)
    B = real_blocks(rng, 6, n, mb)
    coef = rng.standard_normal((3 * mb, mb))
    got = solver.modalProbeUpdate(coef, *B)
    c = coef.astype(LD)
    worst = 0.0
    for x, w, p, gx, gw, gp in ((0, 1, 2) + got[:3], (3, 4, 5) + got[3:]):
        bx, bw, bp = (B[k].astype(LD) for k in (x, w, p))
        ref_p = bw @ c[mb:2 * mb] + bp @ c[2 * mb:]
        mag_p = np.abs(bw) @ np.abs(c[mb:2 * mb]) + np.abs(bp) @ np.abs(c[2 * mb:])
        ref_x = bx @ c[:mb] + ref_p
        mag_x = np.abs(bx) @ np.abs(c[:mb]) + mag_p
        worst = max(worst, ratio_of(np.abs(gp.astype(LD) - ref_p), 2 * mb * EPS * mag_p),
                    ratio_of(np.abs(gx.astype(LD) - ref_x), (3 * mb + 1) * EPS * mag_x))
        assert same_bits(gw, B[w])
    note("k_modal_update", mb, n, worst)
    again = solver.modalProbeUpdate(coef, *B)
    assert all(same_bits(a, b) for a, b in zip(again, got))


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_probe_arguments(solver):
    z = np.zeros((4, 4))
    p = z.ctypes.data
    lib = L.lib()
    for mb, n in ((5, 4), (32, 4), (4, 0), (4, -1)):
        assert lib.pfem_modal_probe_gram(solver._h, mb, n, p, p, p, p, p, p, p, p) == L.ERR_ARG
        assert lib.pfem_modal_probe_residual(solver._h, mb, n, p, p, p, None, p, p, p) == L.ERR_ARG
        assert lib.pfem_modal_probe_update(solver._h, mb, n, p, p, p, p, p, p, p) == L.ERR_ARG
    assert lib.pfem_modal_probe_gram(None, 4, 1, p, p, p, p, p, p, p, p) == L.ERR_ARG
    assert lib.pfem_modal_probe_update(solver._h, 4, 1, None, p, p, p, p, p, p) == L.ERR_ARG
    v = C.c_int(7)
    assert lib.pfem_solver_reordered(solver._h, C.byref(v)) == L.OK and v.value == 0
    assert lib.pfem_solver_reordered(solver._h, None) == L.ERR_ARG
    with pytest.raises(ValueError):
        solver.modalProbeGram(*[np.zeros((3, 5))] * 6, np.ones(3))
    with pytest.raises(ValueError):
        solver.modalProbeUpdate(np.zeros((12, 4)), *[np.zeros((3, 4))] * 5, np.zeros((4, 4)))
