"""gamg's numeric phase on one rank with level 0 in the 4-row relative-group SpMV form: on a warm step level 1 is summed from the
SpMV's 16-bit value codes (k_lat_galerkin_codes, pfem_amg_kernels.hpp) instead of the fp64 row form (k_lat_galerkin).  The same
additions in the same order, so everything downstream keeps its bits.

Every case assembles and solves twice and looks at the second step: only the second assembly of a pattern writes the codes itself
(the first forms the coarse operators in the symbolic phase).  The small cubes reach the group form through setSpmvFormat("grouped"),
as in test_gpu_level0_epilogue.py.
"""
import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import host as H
from test_gpu_parity import _device_problem

pytestmark = pytest.mark.gpu


def _problem(cells, grouped=True, elemdata=H.POISSON_ELEMDATA):
    s, dm = _device_problem(pf.POISSON_TET, H.gen_box_tets(-1, 1, cells[0], -1, 1, cells[1], -1, 1, cells[2]), elemdata)
    if grouped:
        s.setSpmvFormat("grouped")
        s.buildPattern()
        s.assemble(elemdata, H.TIMEDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=5000)
    return s, dm


def _step(s, elemdata=None):
    """One step (with `elemdata`: assembled anew first) and everything the numeric phase feeds."""
    if elemdata is not None:
        s.assemble(elemdata, H.TIMEDATA)
    its, reason, _ = s.factoriseAndSolve()
    assert reason == 2
    info = s.amgInfo()
    assert info["levels"] >= 3
    return {"from_codes": info["galerkin_from_codes"], "its": its, "lam": np.array(info["lambda_max"]), "l1": s.amgLevelValues(1),
            "l2": s.amgLevelValues(2), "hist": s.getHistory(), "x": s.getSolution()}


def _same_bits(a, b):
    assert a["its"] == b["its"]
    for key in ("lam", "l1", "l2", "hist", "x"):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("cells", [(40, 40, 40), (40, 38, 36), (41, 37, 33)])
def test_level1_from_codes_equals_the_fp64_kernel_bit_for_bit(cells, monkeypatch):
    """(40, 40, 40): 39 free nodes per axis -- a one-node brick at every far edge, x-pairs that drift across the 4-row groups from
    line to line; (40, 38, 36): ragged, n % 4 != 0; (41, 37, 33): an even free count on every axis, whole bricks only."""
    out = {}
    for leg in ("1", "0"):
        monkeypatch.setenv("PFEM_AMG_GALERKIN_CODES", leg)
        s, dm = _problem(cells)
        assert dm.size_global == (cells[0] - 1) * (cells[1] - 1) * (cells[2] - 1)
        first = _step(s)
        assert not first["from_codes"]                       # (the symbolic phase formed the levels)
        out[leg] = _step(s, H.POISSON_ELEMDATA)
        assert s.spmvRowGroup() == 4 and s.spmvValueDictionary() > 0
        assert out[leg]["from_codes"] == (leg == "1")        # (no passing by falling back)
        assert out[leg]["l1"].size > 0 and out[leg]["l2"].size > 0 and np.abs(out[leg]["l1"]).max() > 0.0
        _same_bits(first, out[leg])                          # (the same matrix: the same step)
        s.free()
    _same_bits(out["1"], out["0"])


def test_a_dictionary_miss_takes_the_fp64_kernel_and_the_next_step_the_codes_again():
    cells = (40, 38, 36)
    scaled = H.POISSON_ELEMDATA * 1.7
    f, _ = _problem(cells, elemdata=scaled)
    fresh = _step(f)
    f.free()
    s, _ = _problem(cells)
    _step(s)
    assert _step(s, H.POISSON_ELEMDATA)["from_codes"]
    third = _step(s, scaled)                                 # values the dictionary lacks
    assert not third["from_codes"]
    _same_bits(fresh, third)
    fourth = _step(s, scaled)                                # the new dictionary holds them
    assert fourth["from_codes"]
    _same_bits(fresh, fourth)
    s.free()


@pytest.mark.parametrize("form", ["no-dictionary", "one-row"])
def test_fallbacks_keep_the_fp64_kernel(form, monkeypatch):
    """PFEM_SPMV_VALDICT=0 (the group form streams doubles) and the one-row form (no group form at all): the fp64 kernel, and the
    step solves as it does with the new kernel switched off."""
    if form == "no-dictionary":
        monkeypatch.setenv("PFEM_SPMV_VALDICT", "0")
    out = {}
    for leg in ("1", "0"):
        monkeypatch.setenv("PFEM_AMG_GALERKIN_CODES", leg)
        s, _ = _problem((40, 40, 40), grouped=form != "one-row")
        _step(s)
        out[leg] = _step(s, H.POISSON_ELEMDATA)
        assert s.spmvRowGroup() == (1 if form == "one-row" else 4) and s.spmvValueDictionary() == 0
        assert not out[leg]["from_codes"]
        s.free()
    _same_bits(out["1"], out["0"])
