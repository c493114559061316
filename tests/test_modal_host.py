"""pfem_dense_sym_geneig on the host (no GPU): the Rayleigh-Ritz step of the modal analysis against scipy.linalg.eigh(A, B) on
random symmetric positive definite pairs of the orders the solver uses (8 = 2 x 4, 24 = 3 x 8, 48 = 3 x 16), the "singular"
status, the argument errors, and the stand-alone sanitizer walk (tests/native/modal_sanitize.cpp).

Bound: 64 n eps, relative, for every eigenvalue and for C^T B C - I.  Cholesky, two triangular solves and Jacobi sweeps are
each backward stable with constants of a few n eps; the pairs are well conditioned (B = G^T G / n + I: kappa < 10), so that the
backward error is the forward error up to that factor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

import modal_reference as MO
from pfemfort_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def geneig(A, B, floor=1e-12):
    n = A.shape[0]
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    w, Cm = np.full(n, -7.0), np.full((n, n), -7.0)
    status = C.c_int(-1)
    rc = L.lib().pfem_dense_sym_geneig(n, A.ctypes.data, B.ctypes.data, floor, w.ctypes.data, Cm.ctypes.data, C.byref(status))
    return rc, status.value, w, Cm


def spd_pair(n, seed):
    rng = np.random.default_rng(seed)
    G, Hm = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    return G.T @ G / n + 0.5 * np.eye(n), Hm.T @ Hm / n + np.eye(n)


@pytest.mark.parametrize("n", [8, 24, 48])
def test_random_pairs_against_scipy(n):
    A, B = spd_pair(n, 100 + n)
    rc, status, w, Cm = geneig(A, B)
    assert rc == L.OK and status == 0
    ref = sl.eigh(A, B, eigvals_only=True)
    err = np.abs(w / ref - 1.0).max()
    orth = np.abs(Cm.T @ B @ Cm - np.eye(n)).max()
    res = np.abs(A @ Cm - B @ Cm * w[None, :]).max() / np.abs(w).max()
    print(f"n = {n}: eigenvalues {err:.3e}, C^T B C - I {orth:.3e}, residual {res:.3e}; bound {64 * n * EPS:.3e}")
    assert (np.diff(w) >= 0.0).all()
    assert err <= 64 * n * EPS
    assert orth <= 64 * n * EPS
    assert res <= 64 * n * EPS
    # only the upper triangles are read
    rc, status, w2, C2 = geneig(np.triu(A), np.triu(B) + np.tril(np.full((n, n), np.nan), -1))
    assert rc == L.OK and status == 0 and np.array_equal(w2, w) and np.array_equal(C2, Cm)
    # ... and the mirror's Rayleigh-Ritz, with the mirror's own Jacobi sweeps, is the same step
    th, Cr = MO.rayleigh_ritz(A, B, n, eig=MO.jacobi_eigh if n <= 24 else None)
    assert np.abs(th / w - 1.0).max() <= 64 * n * EPS


@pytest.mark.parametrize("n", [8, 24, 48])
def test_a_duplicated_column_is_singular(n):
    """S with column n - 1 equal to column 0: the last pivot of B = S^T S is rounding -- status 1 and nothing written"""
    rng = np.random.default_rng(n)
    S = rng.standard_normal((4 * n, n))
    S[:, n - 1] = S[:, 0]
    B = S.T @ S
    A = S.T @ (np.arange(1, 4 * n + 1)[:, None] * S)
    rc, status, w, Cm = geneig(A, B)
    assert rc == L.OK and status == 1
    assert (w == -7.0).all() and (Cm == -7.0).all()
    assert MO.rayleigh_ritz(A, B, n) is None
    # the leading block without the copy is regular
    rc, status, w, Cm = geneig(A[:n - 1, :n - 1].copy(), B[:n - 1, :n - 1].copy())
    assert rc == L.OK and status == 0 and (w > 0.0).all()
    # a diagonal entry of B that is not positive
    B2 = B.copy()
    B2[2, 2] = 0.0
    assert geneig(A, B2)[:2] == (L.OK, 1)


def test_argument_errors():
    one, w, c = np.ones(1), np.zeros(1), np.zeros(1)
    status = C.c_int(0)
    f = L.lib().pfem_dense_sym_geneig
    p = lambda a: a.ctypes.data        # noqa: E731
    assert f(1, p(one), p(one), 0.0, p(w), p(c), C.byref(status)) == L.OK and status.value == 0 and w[0] == 1.0 and c[0] == 1.0
    for n in (0, -1, 49):
        assert f(n, p(one), p(one), 0.0, p(w), p(c), C.byref(status)) == L.ERR_ARG
    assert f(1, None, p(one), 0.0, p(w), p(c), C.byref(status)) == L.ERR_ARG
    assert f(1, p(one), None, 0.0, p(w), p(c), C.byref(status)) == L.ERR_ARG
    assert f(1, p(one), p(one), 0.0, None, p(c), C.byref(status)) == L.ERR_ARG
    assert f(1, p(one), p(one), 0.0, p(w), None, C.byref(status)) == L.ERR_ARG
    assert f(1, p(one), p(one), 0.0, p(w), p(c), None) == L.ERR_ARG
    for bad in (-1e-3, float("nan"), float("inf")):
        assert f(1, p(one), p(one), bad, p(w), p(c), C.byref(status)) == L.ERR_ARG


def test_geneig_under_address_and_ub_sanitizers(tmp_path):
    """pfem_host.cpp's pfem_dense_sym_geneig under ASan + UBSan: a stand-alone program that walks n = 1, 47 and 48 on exact-size
    buffers and the argument errors (tests/native/modal_sanitize.cpp)."""
    exe = tmp_path / "modal_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fopenmp",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "modal_sanitize.cpp"),
           os.path.join(ROOT, "pfemfort_amd", "csrc", "pfem_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "modal_sanitize: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
