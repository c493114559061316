"""One launch of each block kernel of the buckling solve (pfem_buck_probe_gram / _residual / _update)
against a plain evaluation of the same operation, at MB = 4 / 8 / 16 and at row counts on both sides of every point where the
kernel takes another path: one row, a tile less one row, a tile, a tile and a row, the rows one pass of the capped grid covers
less one, exactly and plus one (8 191 / 8 192 / 8 193 for the Gram kernel: 256 blocks x 32 rows), and a count past 1 024
blocks of the vector kernels at which some blocks take three trips and others two with a partial last tile.  The meshes of
test_gpu_buckling.py end at 2 112 rows -- one trip of every loop.

Exact data: small integers (blocks in [-4, 4], theta and the coefficients in [-2, 2], dinv a power of two), so that every
product and partial sum is an integer below 2^53 and the device must equal numpy's int64 evaluation bit for bit; no zero in the
first and last row of a tile or in the last row.  Rounding data: standard normals times 10**uniform(-3, 3) per row against numpy
longdouble, with the bounds test_gpu_modal_kernels.py uses (eps = 2^-52):
  Gram entry (a, b)  (n + 2) eps sum_i |s_ia| |q_ib|, q the K_g- or the K-product: an n-term fma sum in any order;
  W of the residual  the bits of numpy's float64 dinv * (gx - kx * theta): elementwise IEEE operations, no contraction;
  norms              (n + 1) eps x the longdouble sum of the squares of those float64 values;
  update             P': 2 mb eps sum_k |s_k c_k| over the W and P terms; X': (3 mb + 1) eps sum_k |s_k c_k| over all terms,
                     for each of the three families (S, K S, K_g S)."""
import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import _lib as L

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
MBS = [4, 8, 16]
GRAM_TILE, GRAM_BLOCKS, VEC_BLOCKS, BLOCK = 32, 256, 1024, 256       # pfem_modal_kernels.hpp: the buckling kernels share them
GRAM_ONE_PASS = GRAM_TILE * GRAM_BLOCKS                              # 8 192 rows
GRAM_N = [1, 31, 32, 33, GRAM_ONE_PASS - 1, GRAM_ONE_PASS, GRAM_ONE_PASS + 1, 2 * GRAM_ONE_PASS + 32 + 7]


def residual_n(mb):
    T = VEC_BLOCKS * BLOCK // mb
    return [1, 63, BLOCK // mb, T, T + 1, 2 * T + 77]


def update_n(mb):
    T, TR = VEC_BLOCKS * BLOCK // mb, BLOCK // mb
    return [1, TR - 1, TR, TR + 1, T, T + 1, 2 * T + TR // 2 + 1]


RESIDUAL = [(mb, n) for mb in MBS for n in residual_n(mb)]
UPDATE = [(mb, n) for mb in MBS for n in update_n(mb)]
GRAM = [(mb, n) for mb in MBS for n in GRAM_N]
FAMILIES = ((0, 1, 2), (3, 4, 5), (6, 7, 8))                         # (X, W, P) of S, of K S, of K_g S among the nine blocks

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


# ---- k_buck_gram, k_modal_sum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb,n", GRAM)
def test_gram_exact(solver, mb, n):
    rng = np.random.default_rng(1100 * mb + n)
    B = int_blocks(rng, 9, n, mb, GRAM_TILE)
    S, K, G = (np.hstack(B[3 * f:3 * f + 3]) for f in range(3))
    up = computed(mb)
    want_g, want_k = np.where(up, S.T @ G, 0), np.where(up, S.T @ K, 0)
    assert max(np.abs(want_g).max(), np.abs(want_k).max()) < 2 ** 53 and np.abs(np.diag(want_k)).sum() > 0
    gg, gk = solver.buckProbeGram(*B)
    assert same_bits(gg, want_g) and same_bits(gk, want_k)                  # (the tiles below the diagonal: +0.0)


@pytest.mark.parametrize("mb,n", GRAM)
def test_gram_rounding(solver, mb, n):
    rng = np.random.default_rng(2100 * mb + n)
    B = real_blocks(rng, 9, n, mb)
    S, K, G = (np.hstack(B[3 * f:3 * f + 3]).astype(LD) for f in range(3))
    up = computed(mb)
    gg, gk = solver.buckProbeGram(*B)
    worst = 0.0
    for got, Q in ((gg, G), (gk, K)):
        assert (got[~up] == 0.0).all() and not np.signbit(got[~up]).any()
        worst = max(worst, ratio_of(np.abs(got.astype(LD) - S.T @ Q)[up], ((n + 2) * EPS * (np.abs(S).T @ np.abs(Q)))[up]))
    note("k_buck_gram", mb, n, worst)
    again = solver.buckProbeGram(*B)
    assert same_bits(again[0], gg) and same_bits(again[1], gk)


# ---- k_buck_residual, k_modal_sum --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dinv", [True, False])
@pytest.mark.parametrize("mb,n", RESIDUAL)
def test_residual_exact(solver, mb, n, with_dinv):
    rng = np.random.default_rng(3100 * mb + n)
    GX, KX = int_blocks(rng, 2, n, mb, BLOCK // mb)
    theta = rng.integers(-2, 3, mb).astype(np.int64)
    dinv = 2.0 ** rng.integers(-2, 3, n) if with_dinv else None
    R = GX - KX * theta[None, :]
    want_w = R.astype(np.float64) * (dinv[:, None] if with_dinv else 1.0)
    want_norms = np.stack([(R * R).sum(0), (GX * GX).sum(0), (KX * KX).sum(0)])
    assert want_norms.max() < 2 ** 53 and (want_norms[1:] > 0).all()
    Wd, norms = solver.buckProbeResidual(GX, KX, theta, dinv)
    assert same_bits(Wd, want_w) and same_bits(norms, want_norms)


@pytest.mark.parametrize("with_dinv", [True, False])
@pytest.mark.parametrize("mb,n", RESIDUAL)
def test_residual_rounding(solver, mb, n, with_dinv):
    rng = np.random.default_rng(4100 * mb + n)
    GX, KX = real_blocks(rng, 2, n, mb)
    theta = rng.standard_normal(mb)
    dinv = 10.0 ** rng.uniform(-2, 2, n) if with_dinv else None
    R = GX - KX * theta[None, :]
    want_w = dinv[:, None] * R if with_dinv else R
    Wd, norms = solver.buckProbeResidual(GX, KX, theta, dinv)
    assert same_bits(Wd, want_w)
    ref = np.stack([(v.astype(LD) ** 2).sum(0) for v in (R, GX, KX)])
    note("k_buck_residual", mb, n, ratio_of(np.abs(norms.astype(LD) - ref), (n + 1) * EPS * ref))
    again = solver.buckProbeResidual(GX, KX, theta, dinv)
    assert same_bits(again[0], Wd) and same_bits(again[1], norms)


# ---- k_buck_update -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb,n", UPDATE)
def test_update_exact(solver, mb, n):
    rng = np.random.default_rng(5100 * mb + n)
    B = int_blocks(rng, 9, n, mb, BLOCK // mb)
    coef = rng.integers(-2, 3, (3 * mb, mb)).astype(np.int64)
    coef[np.arange(3 * mb), np.arange(3 * mb) % mb] = rng.choice([-2, -1, 1, 2], 3 * mb)       # no block of C without a say
    got = solver.buckProbeUpdate(coef, *B)
    for x, w, p in FAMILIES:
        want_p = B[w] @ coef[mb:2 * mb] + B[p] @ coef[2 * mb:]
        want_x = B[x] @ coef[:mb] + want_p
        assert same_bits(got[p], want_p) and same_bits(got[x], want_x)
        assert same_bits(got[w], B[w])


@pytest.mark.parametrize("mb,n", UPDATE)
def test_update_rounding(solver, mb, n):
    rng = np.random.default_rng(6100 * mb + n)
    B = real_blocks(rng, 9, n, mb)
    coef = rng.standard_normal((3 * mb, mb))
    got = solver.buckProbeUpdate(coef, *B)
    c = coef.astype(LD)
    worst = 0.0
    for x, w, p in FAMILIES:
        bx, bw, bp = (B[k].astype(LD) for k in (x, w, p))
        ref_p = bw @ c[mb:2 * mb] + bp @ c[2 * mb:]
        mag_p = np.abs(bw) @ np.abs(c[mb:2 * mb]) + np.abs(bp) @ np.abs(c[2 * mb:])
        ref_x = bx @ c[:mb] + ref_p
        mag_x = np.abs(bx) @ np.abs(c[:mb]) + mag_p
        worst = max(worst, ratio_of(np.abs(got[p].astype(LD) - ref_p), 2 * mb * EPS * mag_p),
                    ratio_of(np.abs(got[x].astype(LD) - ref_x), (3 * mb + 1) * EPS * mag_x))
        assert same_bits(got[w], B[w])
    note("k_buck_update", mb, n, worst)
    again = solver.buckProbeUpdate(coef, *B)
    assert all(same_bits(a, b) for a, b in zip(again, got))


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_probe_arguments(solver):
    z = np.zeros((4, 4))
    p = z.ctypes.data
    lib = L.lib()
    for mb, n in ((5, 4), (32, 4), (4, 0), (4, -1)):
        assert lib.pfem_buck_probe_gram(solver._h, mb, n, *([p] * 10)) == L.ERR_ARG
        assert lib.pfem_buck_probe_residual(solver._h, mb, n, p, p, None, p, p, p) == L.ERR_ARG
        assert lib.pfem_buck_probe_update(solver._h, mb, n, *([p] * 10)) == L.ERR_ARG
    assert lib.pfem_buck_probe_gram(None, 4, 1, *([p] * 10)) == L.ERR_ARG
    assert lib.pfem_buck_probe_update(solver._h, 4, 1, None, *([p] * 9)) == L.ERR_ARG
    assert lib.pfem_buck_probe_residual(solver._h, 4, 1, p, p, None, None, p, p) == L.ERR_ARG
    with pytest.raises(ValueError):
        solver.buckProbeGram(*[np.zeros((3, 5))] * 9)
    with pytest.raises(ValueError):
        solver.buckProbeUpdate(np.zeros((12, 4)), *[np.zeros((3, 4))] * 8, np.zeros((4, 4)))
