"""gamg on one rank: the fused products of a coarse level that takes the value dictionary read one-byte column codes (the index of
col - row among the level's distinct offsets, k_amg_spmv_ep_vd<., true> in pfem_amg_kernels.hpp) instead of int32 columns.  The
same products in the same order, so every solve keeps its bits; the codes are compared with the columns on the device before
they are used, and a level with too many distinct offsets keeps its int32 kernel.

A level takes the dictionary from 2^20 stored slots, and level 1 of a box of tetrahedra stores 16.7 slots a row (a 15-point stencil
in slices of 64 rows: 715 200 slots at 70^3 cells, measured, so that box does not reach the form).  82^3 cells: 81^3 free rows,
level 1 = 41^3 = 68 921 rows and about 1.15 M slots, the only level large enough.  84 x 82 x 80 cells: level 1 = 42 * 41 * 40 =
68 880 rows = 1076 slices + 16 rows, a partly filled last slice, and boundary slices narrower than the rest.  Every configuration
is solved once per module and shared.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_parity import _moved

pytestmark = pytest.mark.gpu

CELLS = {"cube": (82, 82, 82), "ragged": (84, 82, 80)}
MOVED = {"cube_moved": "cube"}          # the same cells, the nodes off their sites (test_gpu_parity._moved)
SWITCHES = ("PFEM_AMG_COL_CODES", "PFEM_AMG_COL_CODES_MAX", "PFEM_AMG_FUSED", "PFEM_CG_GRAPH", "PFEM_SPMV_VALDICT")
LEGS = {"codes": {}, "int32": {"PFEM_AMG_COL_CODES": "0"}, "unfused": {"PFEM_AMG_FUSED": "0"}}


@contextlib.contextmanager
def _env(**kw):
    """The switches of this file as given, every other one of them unset; restored afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _setup(name):
    c = CELLS[MOVED.get(name, name)]
    mesh = H.gen_box_tets(-1, 1, c[0], -1, 1, c[1], -1, 1, c[2])
    return D._setup(pf.POISSON_TET, _moved(mesh, 2.0 / max(c)) if name in MOVED else mesh)


def _rows(name):
    """Free rows of the box and of its first brick level (bricks of two nodes per axis)."""
    free = [c - 1 for c in CELLS[MOVED.get(name, name)]]
    return int(np.prod(free)), int(np.prod([(f + 1) // 2 for f in free]))


def _load(s, name):
    dm, conn, xyz, edof = _setup(name)
    if not s._h or s.size_global != dm.size_global:
        s.initialise(dm.size_global, dm.size_global)
    s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=5000)


def _step(s, name, assemble=False):
    if assemble:
        s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
    its, reason, _ = s.factoriseAndSolve()
    assert reason == 2
    info, cyc = s.amgInfo(), s.amgCycle()
    print(name, "rows", info["rows"], "column_codes", cyc["column_codes"], "builds", cyc["column_code_builds"], "its", its)
    assert tuple(info["rows"][:2]) == _rows(name) and info["levels"] >= 4
    return {"its": its, "lam": np.array(info["lambda_max"]), "hist": s.getHistory(), "x": s.getSolution(), "cc": cyc["column_codes"],
            "builds": cyc["column_code_builds"]}


def _same_bits(a, b, where):
    assert a["its"] == b["its"], where
    for key in ("lam", "hist", "x"):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (where, key)


@functools.lru_cache(maxsize=None)
def _two_solves(name, leg, graph):
    """A fresh solver under the switches of `leg`: the pattern's first solve and a warm step."""
    with _env(PFEM_CG_GRAPH=graph, **LEGS[leg]):
        s = pf.PetscSolver()
        try:
            _load(s, name)
            return _step(s, name), _step(s, name, assemble=True)
        finally:
            s.free()


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("name", sorted(CELLS))
def test_column_codes_keep_every_bit(name, graph):
    ref = _two_solves(name, "int32", "1")
    for leg in LEGS:
        first, warm = _two_solves(name, leg, graph)
        for what, step in (("first", first), ("warm", warm)):
            assert step["cc"] == ([1] if leg == "codes" else []), (leg, what)          # (no passing by falling back)
            assert step["builds"] == (1 if leg == "codes" else 0), (leg, what)         # (built once per hierarchy)
            _same_bits(step, ref[0], (name, leg, graph, what))
    _same_bits(ref[1], ref[0], (name, "reference, warm"))


@pytest.mark.parametrize("name", sorted(CELLS))
def test_decoded_columns_equal_the_int32_columns(name):
    with _env():
        s = pf.PetscSolver()
        try:
            _load(s, name)
            assert _step(s, name)["cc"] == [1]
            n = _rows(name)[1]
            cols, dec = s.amgLevelColumns(1, False), s.amgLevelColumns(1, True)
        finally:
            s.free()
    # (slot order, padding included; the lanes past n of the last slice hold 0 in both: every slot is compared)
    assert cols.size >= 2 ** 20 and cols.size % 64 == 0 and cols.shape == dec.shape
    assert cols.min() == 0 and cols.max() == n - 1
    assert np.array_equal(cols, dec)


def test_too_many_offsets_keep_the_int32_kernel():
    name = "ragged"
    ref = _two_solves(name, "int32", "1")[0]
    with _env(PFEM_AMG_COL_CODES_MAX="8"):
        s = pf.PetscSolver()
        try:
            _load(s, name)
            for what, assemble in (("first", False), ("second", True)):
                step = _step(s, name, assemble)
                assert step["cc"] == [] and step["builds"] == 1, what          # (refused for the hierarchy: not tried again)
                _same_bits(step, ref, what)
            with pytest.raises(Exception):
                s.amgLevelColumns(1, True)
        finally:
            s.free()


def test_a_level_whose_values_do_not_repeat_refuses_its_dictionary():
    """The 82^3 box with its nodes moved inside balls of 0.2 cell edges (test_gpu_parity._moved): the numbering is still a box's, so
    the hierarchy keeps its bricks and level 1 its 41^3 rows and 1.15 M slots -- a candidate for the dictionary --, but its 68 921 rows
    are sums over cells that differ: more than 4096 distinct values, the verdict refuses the level for this hierarchy.  The pattern's
    first solve and two warm steps stream fp64 values and int32 columns on level 1 (the column codes ride on the value codes), and
    each is, bit for bit, the same solve with the dictionaries switched off."""
    name = "cube_moved"

    def three_solves(**env):
        with _env(**env):
            s = pf.PetscSolver()
            try:
                _load(s, name)
                steps = []
                for assemble in (False, True, True):
                    step = _step(s, name, assemble)
                    lat, step["vd"] = s.amgLayout()["lattice_levels"], s.amgValueDictionaries()
                    print(name, env, "lattice_levels", lat, "value dictionaries", step["vd"])
                    assert tuple(s.amgInfo()["rows"][:2]) == _rows(name) and lat >= 1          # (bricks, through the numbering)
                    steps.append(step)
                return steps
            finally:
                s.free()

    ref = three_solves(PFEM_SPMV_VALDICT="0")
    for what, step, off in zip(("first", "warm", "second warm"), three_solves(), ref):
        assert step["vd"][1] == 0 and off["vd"][1] == 0, (what, step["vd"])
        assert step["cc"] == [] and off["cc"] == [], what
        _same_bits(step, off, what)


def test_reused_solver_follows_the_mesh_and_the_switch():
    """82^3 -> the ragged box in the same object, then the switch off and on again: each solve is a fresh solver's, bit for bit,
    with the level list of its own configuration (flags and buffers die with the hierarchy; the cycle's graph follows the switch)."""
    ref = {name: _two_solves(name, "int32", "1")[0] for name in CELLS}
    s = pf.PetscSolver()
    try:
        with _env():
            _load(s, "cube")
            step = _step(s, "cube")
            assert step["cc"] == [1] and step["builds"] == 1
            _same_bits(step, ref["cube"], "cube")
            _load(s, "ragged")
            step = _step(s, "ragged")
            assert step["cc"] == [1] and step["builds"] == 1          # (the new hierarchy's own codes)
            _same_bits(step, ref["ragged"], "ragged after cube")
            assert np.array_equal(s.amgLevelColumns(1, False), s.amgLevelColumns(1, True))
        with _env(PFEM_AMG_COL_CODES="0"):
            step = _step(s, "ragged", assemble=True)
            assert step["cc"] == [] and step["builds"] == 1
            _same_bits(step, ref["ragged"], "switched off")
        with _env():
            step = _step(s, "ragged", assemble=True)
            assert step["cc"] == [1] and step["builds"] == 1          # (still the codes built before: nothing is built twice)
            _same_bits(step, ref["ragged"], "switched on again")
    finally:
        s.free()
