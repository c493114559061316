"""The bottom of the gamg cycle in one workgroup (k_amg_tail), and the coarse levels' eigenvalue bounds left by the Galerkin
products themselves, against the level-by-level kernels and the stand-alone maxima that PFEM_AMG_FUSED=0 keeps.

The tail has three builds -- vectors, index lists and the first level's matrix in LDS; vectors and lists in LDS with the matrix
read from memory; everything in memory -- and every one does the same operations in the same order as the kernels it replaces:
iterations, residual history and solution are equal bit for bit, as a graph replay and as plain launches, over both value
streams of level 0.  Every case asserts the hierarchy it means to run and that the fused run took the tail (no passing by
falling back), which build of it, and how many bounds the products left (amgBoundsByProducts()).  The bounds (amgInfo()["lambda_max"]) are compared as
well: a maximum does not depend on the order it is taken in.
"""
import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import host as H
from test_gpu_parity import _device_problem, _moved, _shuffled

pytestmark = pytest.mark.gpu


def _solve(kind, mesh, ed, grouped):
    s, _ = _device_problem(kind, mesh, ed)
    if grouped:
        s.setSpmvFormat("grouped")
        s.buildPattern()
        s.assemble(ed, H.TIMEDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=5000)
    its, reason, _ = s.factoriseAndSolve()
    assert reason == 2
    return s, (its, s.getHistory(), s.getSolution())


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _fused_against_reference(monkeypatch, kind, mesh, ed, grouped, rows, tail_from, build, products, rbm_level=None):
    """Every (value stream, fused, graph) combination solves to the bits of (first value stream, fused, graph replay), twice each:
    the first solve of a pattern forms the levels in the symbolic phase and takes the stand-alone maxima, the second one runs the
    numeric set-up, where `products` coarse levels get their bound from the Galerkin product itself (none with PFEM_AMG_FUSED=0;
    products = None: at least level 1).
    `build`: where the fused run's tail keeps its data."""
    out = {}
    for vd in ("0", "1"):
        monkeypatch.setenv("PFEM_SPMV_VALDICT", vd)
        for fused, graph in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
            monkeypatch.setenv("PFEM_AMG_FUSED", fused)
            monkeypatch.setenv("PFEM_CG_GRAPH", graph)
            s, res = _solve(kind, mesh, ed, grouped)
            info, cyc = s.amgInfo(), s.amgCycle()
            assert info["rows"] == rows
            assert (cyc["tail_from"], cyc["tail_build"]) == ((tail_from, build) if fused == "1" else (-1, None))          # (no passing by falling back)
            assert s.amgBoundsByProducts() == 0
            assert rbm_level is None or s.amgTransfer(rbm_level)["rbm"]
            its, reason, _ = s.factoriseAndSolve()
            assert reason == 2 and _same(res, (its, s.getHistory(), s.getSolution())) and s.amgInfo()["lambda_max"] == info["lambda_max"]
            got = s.amgBoundsByProducts()
            assert got == (products if fused == "1" else 0) if products is not None else (1 <= got < len(rows)) == (fused == "1"), got
            out[vd, fused, graph] = res + (info["lambda_max"],)
            s.free()
    a = out["0", "1", "1"]
    for key, b in out.items():
        assert _same(a, b) and a[3] == b[3], key


def _cube(cells):
    return H.gen_box_tets(-1, 1, cells[0], -1, 1, cells[1], -1, 1, cells[2])


def test_flagship_tail_matrix_in_lds(monkeypatch):
    """28 cells a side: 27^3 free rows, levels 19 683 -> 2 744 -> 343 -> 64.  The tail is the flagship's own: the 343- and 64-row
    levels, the 343-row level's 10 368 matrix slots staged in LDS beside the vectors and the index lists, and a dense inverse of
    64 rows."""
    _fused_against_reference(monkeypatch, pf.POISSON_TET, _cube((28, 28, 28)), H.POISSON_ELEMDATA, True,
                             [19683, 2744, 343, 64], 2, "lds+matrix", 3)


def test_tail_vectors_in_lds_matrix_from_memory(monkeypatch):
    """40 cells a side: 39^3 free rows, levels 59 319 -> 8 000 -> 1 000 -> 125; the tail is the 1 000- and 125-row levels.  Their
    vectors and lists are in LDS; the 1 000-row level's 27 648 slots (324 KB + offsets) do not fit, so its matrix is read from
    memory; the dense inverse has 125 rows."""
    _fused_against_reference(monkeypatch, pf.POISSON_TET, _cube((40, 40, 40)), H.POISSON_ELEMDATA, True,
                             [59319, 8000, 1000, 125], 2, "lds", 3)


def test_tail_of_ragged_levels(monkeypatch):
    """40 x 38 x 36 cells: 39 * 37 * 35 = 50 505 free rows, bricks of unequal sides all the way down: 20 * 19 * 18 = 6 840, then
    10 * 10 * 9 = 900 rows where the tail begins, then 5 * 5 * 5 = 125.  Level 0 -> 1 is always a product in the lattice form and
    leaves level 1's bound; a product further down that is not in that form (unequal bricks) ends the chain of zeroed words, and the
    levels after it keep the stand-alone maxima -- how many do is not part of what this case states."""
    _fused_against_reference(monkeypatch, pf.POISSON_TET, _cube((40, 38, 36)), H.POISSON_ELEMDATA, True,
                             [50505, 6840, 900, 125], 2, "lds", None)


def _no_lattice(cells):
    """nodes moved at random, numbering shuffled: coarsened by matching"""
    return _shuffled(_moved(_cube(cells), 2.0 / cells[0]))


def test_tail_of_matched_aggregates(monkeypatch):
    """A mesh without a lattice is coarsened by matching: 1 872 -> 275 -> 42 rows, the tail begins at level 1 and its index lists
    are those of irregular aggregates.  No lattice, so no product leaves a bound."""
    _fused_against_reference(monkeypatch, pf.POISSON_TET, _no_lattice((14, 13, 13)), H.POISSON_ELEMDATA, False, [1872, 275, 42], 1, "lds+matrix", 0)


def test_tail_with_more_than_64_kb_of_lds_and_no_matrix(monkeypatch):
    """20 cells a side without a lattice: 6 859 -> 1 013 -> 152 -> 25.  The tail's 1 190 rows take 57 120 B of vectors and, with
    10 040 B of index lists, 67 160 B of LDS: more than the 64 KB a kernel gets unasked, in the build without the matrix.

    Whether the tail works out of LDS is decided by its vectors alone (6 x 8 B a row: up to 1 365 rows in its levels together);
    the lists ride along.  The build that keeps everything in memory (more than 1 365 rows) is not reached by any small mesh
    through the public API: a tail level has at most 1 024 rows, the lattice hierarchies coarsen by 8 to 64 a level and matching
    by about 7, so this case's 1 190 rows are about the most a tail gets, and there is no setting for pair aggregates.  That build
    is compiled from the same source through the same template; it is not run by this file."""
    _fused_against_reference(monkeypatch, pf.POISSON_TET, _no_lattice((20, 20, 20)), H.POISSON_ELEMDATA, False, [6859, 1013, 152, 25], 1, "lds", 0)


def test_tail_with_the_rigid_body_transfer(monkeypatch):
    """The 6 x 36 x 6 beam of test_gpu_parity.py (node-wise aggregates): 5 292 -> 216 -> 24 rows.  Both tail levels carry six dofs
    a node and the rigid-body transfer between them, which reads its own lists from memory and the vectors from LDS.  Hierarchies
    with rigid-body modes keep the stand-alone bound kernels."""
    mesh = H.gen_box_tets(-0.5, 0.5, 6, 0.0, 6.0, 36, -0.5, 0.5, 6, bc_mode=1, ndof=3)
    _fused_against_reference(monkeypatch, pf.ELAST_TET, mesh, H.ELAST_ELEMDATA, True, [5292, 216, 24], 1, "lds", 0, rbm_level=1)


def test_second_solve_on_the_same_solver(monkeypatch):
    """Nothing of the first solve is left in what the second one reads -- the bound words the products' blocks meet in are zeroed
    inside every set-up --: the same bounds, history and iterate again, after a new assembly too, and the same as the reference
    path's.  (The first solve of a pattern forms the levels in the symbolic phase and takes the stand-alone maxima; the later ones
    take the products' own.)"""
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("PFEM_AMG_FUSED", fused)
        s, first = _solve(pf.POISSON_TET, _cube((28, 28, 28)), H.POISSON_ELEMDATA, True)
        assert s.amgInfo()["rows"] == [19683, 2744, 343, 64] and s.amgCycle()["tail_from"] == (2 if fused == "1" else -1)
        lam = s.amgInfo()["lambda_max"]
        its, reason, _ = s.factoriseAndSolve()
        second = (its, s.getHistory(), s.getSolution())
        assert reason == 2 and _same(first, second) and s.amgInfo()["lambda_max"] == lam
        assert s.amgBoundsByProducts() == (3 if fused == "1" else 0)
        # ... and after a new assembly (the numeric set-up runs again on the kept hierarchy)
        s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
        its, reason, _ = s.factoriseAndSolve()
        assert reason == 2 and _same(first, (its, s.getHistory(), s.getSolution())) and s.amgInfo()["lambda_max"] == lam
        assert s.amgBoundsByProducts() == (3 if fused == "1" else 0)
        out[fused] = first + (lam,)
        s.free()
    assert _same(out["1"], out["0"]) and out["1"][3] == out["0"][3]
