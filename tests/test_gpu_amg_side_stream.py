"""The numeric set-up's side chain (amg_numeric: the products that form the small levels and the dense inverse on a stream of their
own beside the first cycle's upper levels) against the same solver with PFEM_AMG_SIDE_STREAM=0, where everything runs on the
solver's stream in program order.  The side chain changes where kernels are enqueued and nothing they compute: iterations, reason,
residual history, solution, every coarse level's stored values and every level's bound are compared bit for bit after every step.

Each shape runs five steps on one solver with element data A, A, B, B, A (B = other conductivities), so that a cycle that read a
coarse level before the chain had written it would meet the operator of the step before and give another answer: the first B step
must differ from the A step before it.  The first step of a solver forms its levels in the symbolic phase and never forks; the
first A -> B step meets values the dictionaries lack (the rebuild path), the second B step is the steady state.

Shapes (free rows a side; cells = rows + 1):
  * 39^3: no coarse level reaches 2^20 stored slots, no verdict levels; the fork sits behind 0 -> 1, the join at the restriction 1 -> 2;
  * 82^3 and 84 x 82 x 80: level 1 stores more than 2^20 slots and is a verdict level -- the value dictionary and, on the cube, the
    column codes (asserted there; on the box of unequal bricks the run is held to what the one-stream run does) --: the fork
    behind a verdict level, the verdicts read on the solver's stream while the chain runs;
  * the 20-cell cube without a lattice (test_gpu_amg_tail.py): matched aggregates, the map-driven products with stand-alone bound
    kernels on the side stream, the tail from level 1 on with more than 64 KB of LDS: the join in front of k_amg_tail.
Every run asserts that the chain was forked, and from which level (no passing by falling back), and that it was not with the switch
off, with rigid-body modes and with PFEM_AMG_FUSED=0.
"""
import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import host as H
from test_gpu_parity import _moved, _shuffled

pytestmark = pytest.mark.gpu

ED_A = H.POISSON_ELEMDATA
ED_B = np.array([2.0, 0.5, 1.5])
SEQUENCE = (ED_A, ED_A, ED_B, ED_B, ED_A)


def _cube(cells):
    return H.gen_box_tets(-1, 1, cells[0], -1, 1, cells[1], -1, 1, cells[2])


SHAPES = {
    # name: (mesh, levels on column codes -- None: whatever the one-stream run has --, first level of the side chain)
    "cube39": (lambda: _cube((40, 40, 40)), [], 2),
    "cube82": (lambda: _cube((83, 83, 83)), [1], 2),
    "box84x82x80": (lambda: _cube((85, 83, 81)), None, 2),          # (bricks of unequal sides: whether level 1 gets column codes is not this file's business)
    "cube20_no_lattice": (lambda: _shuffled(_moved(_cube((20, 20, 20)), 2.0 / 20)), [], 2),
}
_setups = {}


def _setup(kind, name, make):
    """(dm, conn, xyz, edof) of a mesh, numbered once for all the solvers of this file"""
    if name not in _setups:
        from pfemfort_amd import drivers as D
        _setups[name] = D._setup(kind, make())
    return _setups[name]


def _solver(kind, setup, ed):
    dm, conn, xyz, edof = setup
    s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    s.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    s.assemble(ed, H.TIMEDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-8, maxits=500)
    return s


def _step(s):
    its, reason, _ = s.factoriseAndSolve()
    info = s.amgInfo()
    return {"its": its, "reason": reason, "history": s.getHistory(), "solution": s.getSolution(), "lambda_max": info["lambda_max"],
            "values": [s.amgLevelValues(l) for l in range(1, info["levels"])], "side": s.amgSideStream(), "cycle": s.amgCycle(),
            "numeric_ms": info["numeric_ms"]}


def _sequence(setup, side, monkeypatch):
    monkeypatch.setenv("PFEM_AMG_SIDE_STREAM", side)
    s = _solver(pf.POISSON_TET, setup, SEQUENCE[0])
    try:
        steps = [_step(s)]
        for ed in SEQUENCE[1:]:
            s.assemble(ed, H.TIMEDATA)
            steps.append(_step(s))
        return steps
    finally:
        s.free()


def _same_step(a, b, where):
    assert (a["its"], a["reason"]) == (b["its"], b["reason"]), where
    assert np.array_equal(a["history"], b["history"]), where
    assert np.array_equal(a["solution"], b["solution"]), where
    assert a["lambda_max"] == b["lambda_max"], where
    assert len(a["values"]) == len(b["values"]) and all(np.array_equal(x, y) for x, y in zip(a["values"], b["values"])), where


@pytest.mark.parametrize("shape", list(SHAPES))
def test_same_bits_as_one_stream(shape, monkeypatch):
    make, on_codes, first_level = SHAPES[shape]
    setup = _setup(pf.POISSON_TET, shape, make)
    ref = _sequence(setup, "0", monkeypatch)
    got = _sequence(setup, "1", monkeypatch)
    for i, (a, b) in enumerate(zip(got, ref)):
        print(shape, "step", i, "its", a["its"], "side", a["side"], "numeric_ms", a["numeric_ms"], "one stream", b["numeric_ms"], "codes", a["cycle"]["column_codes"])
        assert a["reason"] == 2
        _same_step(a, b, (shape, i))
        assert b["side"] == {"used": False, "first_level": 0, "ms": 0.0}, (shape, i)
        if i == 0:                          # (the levels were formed in the symbolic phase)
            assert not a["side"]["used"], shape
        else:                               # no passing by falling back
            assert a["side"]["used"] and a["side"]["first_level"] == first_level and a["side"]["ms"] > 0.0, (shape, i, a["side"])
            assert a["cycle"] == b["cycle"] and (on_codes is None or a["cycle"]["column_codes"] == on_codes), (shape, i, a["cycle"])
    # the sequence can see a stale operator: B's answer is not A's, and A's comes back
    assert not np.array_equal(ref[2]["solution"], ref[1]["solution"]) and not np.array_equal(ref[2]["values"][-1], ref[1]["values"][-1])
    _same_step(ref[3], ref[2], shape)
    _same_step(ref[4], ref[1], shape)


def test_not_used_without_its_conditions(monkeypatch):
    """Rigid-body transfers (the 6 x 36 x 6 beam) and PFEM_AMG_FUSED=0 keep one stream, warm steps included."""
    beam = H.gen_box_tets(-0.5, 0.5, 6, 0.0, 6.0, 36, -0.5, 0.5, 6, bc_mode=1, ndof=3)
    s = _solver(pf.ELAST_TET, _setup(pf.ELAST_TET, "beam", lambda: beam), H.ELAST_ELEMDATA)
    try:
        for _ in range(2):
            assert s.factoriseAndSolve()[1] == 2 and s.amgTransfer(1)["rbm"] and not s.amgSideStream()["used"]
    finally:
        s.free()
    monkeypatch.setenv("PFEM_AMG_FUSED", "0")
    s = _solver(pf.POISSON_TET, _setup(pf.POISSON_TET, "cube39", SHAPES["cube39"][0]), ED_A)
    try:
        for _ in range(2):
            assert s.factoriseAndSolve()[1] == 2 and s.amgSideStream() == {"used": False, "first_level": 0, "ms": 0.0}
    finally:
        s.free()


def test_a_solve_that_ends_at_once_leaves_the_solver_usable(monkeypatch):
    """maxits = 0 on a warm step: the chain is forked, the solve ends behind its first cycle, and the next solve on the same solver
    gives the bits of a solver that never did this.

    This solve still passes the first cycle's own wait.  The returns between the fork and that wait are error returns of the
    runtime (a failed launch or event call); none of them is reachable from Python without provoking a device fault, so the scope
    guard in run_pcg_amg (SideJoin: the solver's stream follows the side stream on every way out) is covered by reading it."""
    setup = _setup(pf.POISSON_TET, "cube39", SHAPES["cube39"][0])
    monkeypatch.setenv("PFEM_AMG_SIDE_STREAM", "1")
    out = {}
    for cut in (False, True):
        s = _solver(pf.POISSON_TET, setup, ED_A)
        try:
            first = _step(s)
            if cut:
                s.assemble(ED_B, H.TIMEDATA)
                s.setTolerances(rtol=1e-8, maxits=0)
                its, reason, _ = s.factoriseAndSolve()
                assert its == 0 and reason != 2 and s.amgSideStream()["used"]
                s.setTolerances(rtol=1e-8, maxits=500)
            s.assemble(ED_B, H.TIMEDATA)
            second = _step(s)
            assert second["side"]["used"] and second["reason"] == 2
            out[cut] = (first, second)
        finally:
            s.free()
    for k in (0, 1):
        _same_step(out[True][k], out[False][k], k)
