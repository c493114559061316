"""gamg on one rank with level 0 in the 4-row relative-group SpMV form: the cycle's last fine product carries the final smoothing
step and the CG's (r,z), (z,z) as its epilogue (Level0Ep, pfem_kernels.hpp), and x += alpha p is done by the direction kernel.

* The epilogue against its stand-alone twin (PFEM_AMG_FUSED=0: k_amg_cheb_first + k_pc_dots_rows4), as a graph replay and as
  plain launches, over both value streams of the form: the same bits.  The small cubes of the fused-vs-unfused test in
  test_gpu_parity.py stay in the one-row form and never reach this path.
* The ends of a solve with the moved x update against the oracle's restatement of the same loop.
"""
import numpy as np
import pytest

import pfemfort_amd as pf
from oracle import pfem_oracle as O
from pfemfort_amd import host as H
from test_gpu_parity import _device_problem, _transfers

pytestmark = pytest.mark.gpu


def _grouped_poisson(cells):
    s, dm = _device_problem(pf.POISSON_TET, H.gen_box_tets(-1, 1, cells[0], -1, 1, cells[1], -1, 1, cells[2]), H.POISSON_ELEMDATA)
    s.setSpmvFormat("grouped")
    s.buildPattern()
    s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    s.setPreconditioner("gamg")
    return s, dm


@pytest.mark.parametrize("cells", [(40, 40, 40), (40, 38, 36)])
def test_level0_epilogue_equals_standalone_kernels_bit_for_bit(cells, monkeypatch):
    """39^3 = 59 319 and 39 * 37 * 35 = 50 505 free rows: neither a multiple of 4 nor of 1024, so the last lane and the last
    block of the product are ragged."""
    n_free = (cells[0] - 1) * (cells[1] - 1) * (cells[2] - 1)
    assert n_free % 4 and n_free % 1024
    out = {}
    for vd in ("0", "1"):
        monkeypatch.setenv("PFEM_SPMV_VALDICT", vd)
        for fused, graph in (("1", "1"), ("0", "1"), ("1", "0")):
            monkeypatch.setenv("PFEM_AMG_FUSED", fused)
            monkeypatch.setenv("PFEM_CG_GRAPH", graph)
            s, dm = _grouped_poisson(cells)
            assert dm.size_global == n_free
            s.setTolerances(rtol=1e-10, maxits=5000)
            its, reason, _ = s.factoriseAndSolve()
            assert reason == 2 and s.spmvRowGroup() == 4 and (s.spmvValueDictionary() > 0) == (vd == "1")
            assert s.amgCycle()["level0_epilogue"] == (fused == "1")          # (no passing by falling back)
            out[vd, fused, graph] = (its, s.getHistory(), s.getSolution())
            s.free()
    a = out["0", "1", "1"]
    for key, b in out.items():
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), key


def test_one_row_form_keeps_the_standalone_kernels():
    s, _ = _device_problem(pf.POISSON_TET, H.gen_box_tets(-1, 1, 40, -1, 1, 40, -1, 1, 40), H.POISSON_ELEMDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=5000)
    assert s.factoriseAndSolve()[1] == 2 and s.spmvRowGroup() == 1 and not s.amgCycle()["level0_epilogue"]
    s.free()


def _oracle(s, rtol, maxits):
    info, cyc = s.amgInfo(), s.amgCycle()
    rowptr, cols, vals = s.getCSR()
    return O.pcg_amg(rowptr, cols, vals, s.getRHS(), _transfers(s, info), cheb_degree=info["cheb_degree"], fine_degree=info["fine_degree"],
                     eig_ratio=info["eig_ratio"], coarse_scale=info["coarse_scale"], rtol=rtol, maxits=maxits,
                     gamma=2 if cyc["cycle"] == "w" else 1, gamma_to=cyc["last_level_visited_twice"])


def test_ends_of_a_solve_with_the_x_update_in_the_direction_kernel():
    """x is advanced by the kernel that also judges the iterate: in the launch that finds convergence, in the one that stops at
    maxits, never when b = 0, and from zero again in a second solve.  Tolerances: those of the gamg cases of test_gpu_parity.py /
    test_gpu_reuse.py (history 1e-6 of its first entry, iterate 1e-9 where the two loops stop at the same step)."""
    s, _ = _grouped_poisson((40, 40, 40))
    # converged at the default tolerance
    s.setTolerances(rtol=1e-5, maxits=10000)
    its, reason, _ = s.factoriseAndSolve()
    assert s.amgCycle()["level0_epilogue"]
    x, h = s.getSolution(), s.getHistory()
    xo, ito, ro, _, hist = _oracle(s, 1e-5, 10000)
    assert (reason, ro) == (2, 2) and abs(its - ito) <= max(1, ito // 50), (its, ito)
    m = min(len(h), len(hist), 30)
    assert np.abs(h[:m] - hist[:m]).max() <= 1e-6 * hist[0]
    scale = max(1.0, np.abs(xo).max())
    assert np.abs(x - xo).max() <= (1e-9 if its == ito else 1e-3) * scale
    # a second solve on the same solver starts from zero again: the same iterate, not twice the first
    its2, reason2, _ = s.factoriseAndSolve()
    assert (its2, reason2) == (its, reason) and np.array_equal(s.getSolution(), x) and np.array_equal(s.getHistory(), h)
    # stopped by maxits: the oracle's iterate after that many steps
    s.setTolerances(rtol=1e-14, maxits=3)
    its3, reason3, _ = s.factoriseAndSolve()
    x3, ito3, ro3, _, _ = _oracle(s, 1e-14, 3)
    assert (its3, reason3) == (3, -3) and (ito3, ro3) == (3, -3)
    assert np.abs(s.getSolution() - x3).max() <= 1e-9 * max(1.0, np.abs(x3).max())
    s.free()
    # b = 0 (the beam without its body force): 0 iterations, KSP_CONVERGED_ATOL, x all zero
    ed0 = H.ELAST_ELEMDATA.copy()
    ed0[3:] = 0.0
    z, _ = _device_problem(pf.ELAST_TET, H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3), ed0)
    z.setPreconditioner("gamg")
    assert z.factoriseAndSolve()[:2] == (0, 3) and not z.getSolution().any()
    z.free()
