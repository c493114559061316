"""The SpMV form in effect (spmv_form, pfem_device.hip): what the getters say about it is what the launcher runs.

* Every reachable form -- int32 columns, 16-bit gaps (literal, with the gap table, with escapes), the 3-row groups, the 4-row
  relative groups (literal 16-bit gaps, gap table, 32-bit gaps), fp64 values or dictionary codes -- reports one tuple of getter
  values and one byte count, and its product equals the int32 form's bit for bit.  The tuples are not derived here: they are what
  the library returned before the form had a description of its own (commit 2f288c8, profiles/LAB_NOTES.md), so a change of
  any getter, of AUTO's thresholds or of the value-code state shows up as a changed row.
* Level 0's epilogue of gamg on the gap-table form of the relative groups (k_spmvr / k_spmvr_vd <false, true, true>): the cubes
  of test_gpu_level0_epilogue.py have planes that fit 16 bits and never launch it.
"""
import functools
import os

import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import host as H
from test_gpu_parity import _device_problem

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name == "box":        # 11 x 9 x 10 free nodes
        return pf.POISSON_TET, H.POISSON_ELEMDATA, H.gen_box_tets(-1, 1, 12, -1, 1, 10, -1, 1, 11)
    if name == "beam":       # three dofs per node, clamped at y = 0
        return pf.ELAST_TET, H.ELAST_ELEMDATA, H.gen_box_tets(-0.5, 0.5, 4, 0.0, 6.0, 12, -0.5, 0.5, 4, bc_mode=1, ndof=3)
    if name == "tria20":     # unstructured numbering: no group form
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        return pf.POISSON_TRIA, np.array([1.0, 1.0]), H.read_mesh(f"{golden}/input/tria20x20")
    if name == "slab":       # 257 x 257 x 3 free nodes: a z-plane of 66 049 rows, just beyond a 16-bit gap
        return pf.POISSON_TET, H.POISSON_ELEMDATA, H.gen_box_tets(-1, 1, 258, -1, 1, 258, -1, 1, 4)
    if name == "plate":      # 151 x 151 nodes of three dofs to the numbering plane: 68 403 dofs to the next one
        return pf.ELAST_TET, H.ELAST_ELEMDATA, H.gen_box_tets(-0.5, 0.5, 150, 0.0, 1.0, 150, -0.01, 0.01, 1, bc_mode=1, ndof=3)
    if name == "plate256":   # the same with a spacing of 2^-8, exact in binary: 257 x 257 nodes to the plane, element matrices that repeat
        return pf.ELAST_TET, H.ELAST_ELEMDATA, H.gen_box_tets(-0.5, 0.5, 256, 0.0, 1.0, 256, -0.01, 0.01, 1, bc_mode=1, ndof=3)
    raise KeyError(name)


# case -> ((rows per lane, column bits, gap table in use, escapes in use, value codes in use), bytes of one product)
EXPECTED = {
    "box-auto-vd0": ((1, 16, False, False, False), 164064),
    "box-auto-vd1": ((1, 16, False, False, False), 164064),
    "box-int32-vd0": ((1, 32, False, False, False), 195032),
    "box-int32-vd1": ((1, 32, False, False, False), 195032),
    "box-gaps16-vd0": ((1, 16, False, False, False), 164064),
    "box-gaps16-vd1": ((1, 16, False, False, False), 164064),
    "box-grouped-vd0": ((4, 16, False, False, False), 146976),
    "box-grouped-vd1": ((4, 16, False, False, True), 54816),
    "beam-auto-vd0": ((1, 16, False, False, False), 387120),
    "beam-auto-vd1": ((1, 16, False, False, False), 387120),
    "beam-int32-vd0": ((1, 32, False, False, False), 462792),
    "beam-int32-vd1": ((1, 32, False, False, False), 462792),
    "beam-gaps16-vd0": ((1, 16, False, False, False), 387120),
    "beam-gaps16-vd1": ((1, 16, False, False, False), 387120),
    "beam-grouped-vd0": ((3, 16, False, False, False), 350788),
    "beam-grouped-vd1": ((3, 16, False, False, True), 144964),
    "tria20-auto-vd0": ((1, 16, False, False, False), 33520),
    "tria20-auto-vd1": ((1, 16, False, False, False), 33520),
    "tria20-int32-vd0": ((1, 32, False, False, False), 39524),
    "tria20-int32-vd1": ((1, 32, False, False, False), 39524),
    "tria20-gaps16-vd0": ((1, 16, False, False, False), 33520),
    "tria20-gaps16-vd1": ((1, 16, False, False, False), 33520),
    "tria20-grouped-vd0": ((1, 16, False, False, False), 33520),
    "tria20-grouped-vd1": ((1, 16, False, False, False), 33520),
    "slab-grouped-vd0": ((4, 16, True, False, False), 24060832),
    "slab-grouped-vd1": ((4, 16, True, False, True), 9393568),
    "slab-grouped-vd1-PFEM_DEBUG_REL_GAP32": ((4, 32, False, False, False), 25183648),
    "plate-grouped-vd0": ((3, 16, True, False, False), 41215444),
    "plate-grouped-vd1": ((3, 16, True, False, False), 41215444),
    "plate-gaps16-vd1": ((1, 16, True, False, False), 47181696),
    "plate-grouped-vd1-PFEM_DEBUG_NO_ROW_GAP_TABLE": ((1, 16, False, True, False), 47181696),
    "plate-gaps16-vd1-PFEM_DEBUG_NO_ROW_GAP_TABLE": ((1, 16, False, True, False), 47181696),
    "plate256-grouped-vd1": ((3, 16, True, False, True), 50468996),
}

_small = [(m, f, vd, None) for m in ("box", "beam", "tria20") for f in ("auto", "int32", "gaps16", "grouped") for vd in ("0", "1")]
_large = [("slab", "grouped", "0", None), ("slab", "grouped", "1", None), ("slab", "grouped", "1", "PFEM_DEBUG_REL_GAP32"),
          ("plate", "grouped", "0", None), ("plate", "grouped", "1", None), ("plate", "gaps16", "1", None),
          ("plate", "grouped", "1", "PFEM_DEBUG_NO_ROW_GAP_TABLE"), ("plate", "gaps16", "1", "PFEM_DEBUG_NO_ROW_GAP_TABLE"),
          ("plate256", "grouped", "1", None)]


def _case_id(case):
    mesh, fmt, vd, debug = case
    return f"{mesh}-{fmt}-vd{vd}" + (f"-{debug}" if debug else "")


def _observe(case):
    """What the getters say after one product in the case's form, and whether that product equals the int32 form's."""
    mesh, fmt, _, _ = case
    kind, ed, m = _problem(mesh)
    s, dm = _device_problem(kind, m, ed)
    x = np.random.default_rng(7).standard_normal(dm.size_global)
    s.setSpmvFormat(fmt)
    y = s.spmv(x)
    got = ((s.spmvRowGroup(), s.spmvColumnBits(), s.spmvGapTable() > 0, s.spmvGapEscapes(), s.spmvValueDictionary() > 0), s.spmvFormatBytes())
    s.setSpmvFormat("int32")
    same = np.array_equal(y, s.spmv(x))
    int32_says = (s.spmvRowGroup(), s.spmvColumnBits(), s.spmvGapTable(), s.spmvGapEscapes(), s.spmvValueDictionary())
    s.free()
    return got, same, int32_says


@pytest.mark.parametrize("case", _small + _large, ids=_case_id)
def test_getters_agree_with_the_kernel_that_runs(case, monkeypatch):
    monkeypatch.setenv("PFEM_SPMV_VALDICT", case[2])
    if case[3]:
        monkeypatch.setenv(case[3], "1")
    got, same, int32_says = _observe(case)
    assert same and int32_says == (1, 32, 0, False, 0)
    assert got == EXPECTED[_case_id(case)]


def test_level0_epilogue_on_the_gap_table_form(monkeypatch):
    """gamg on the slab whose relative groups need the gap table: with the epilogue and with its stand-alone twin, as a graph
    replay and as plain launches, over both value streams -- the same iteration count, history and iterate, bit for bit."""
    kind, ed, m = _problem("slab")
    out = {}
    for vd in ("0", "1"):
        monkeypatch.setenv("PFEM_SPMV_VALDICT", vd)
        for fused, graph in (("1", "1"), ("0", "1"), ("1", "0")):
            monkeypatch.setenv("PFEM_AMG_FUSED", fused)
            monkeypatch.setenv("PFEM_CG_GRAPH", graph)
            s, dm = _device_problem(kind, m, ed)
            s.setSpmvFormat("grouped")
            s.buildPattern()
            s.assemble(ed, H.TIMEDATA)
            s.setPreconditioner("gamg")
            s.setTolerances(rtol=1e-10, maxits=5000)
            its, reason, _ = s.factoriseAndSolve()
            assert reason == 2 and (s.spmvRowGroup(), s.spmvColumnBits()) == (4, 16) and s.spmvGapTable() > 0
            assert (s.spmvValueDictionary() > 0) == (vd == "1")
            assert s.amgCycle()["level0_epilogue"] == (fused == "1")          # (no passing by falling back)
            out[vd, fused, graph] = (its, s.getHistory(), s.getSolution())
            s.free()
    a = out["0", "1", "1"]
    for key, b in out.items():
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), key
