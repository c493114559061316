"""A reused solver solves like a fresh one after every setter.

A ``PetscSolver`` is built once and reused from step to step (the drivers, bench.py).  Between two solves it keeps the CG
graph execs, the SpMV forms and the flags that say they hold the current values, the value dictionary, the assembly
kernel's level-0 bound, the gamg hierarchy with its automatic knobs, and device blocks the pool hands out again.  gamg is
only a preconditioner: a stale smoother interval, bound or operator still converges, a few iterations later.  So every
case changes one thing on an object that has solved already and checks every solve twice:

1. against a FRESH object built for the same end configuration -- computed first, before the reused object allocated
   anything, so that the two see the device pool in different states -- bit for bit: (its, reason, rnorm), residual
   history, solution and, with gamg, the hierarchy (rows, nonzeros, bounds), the knobs in effect and the cycle;
2. against the oracle's restatement of the same loop on the device's own CSR and right-hand side (O.pcg_jacobi and its
   kin; gamg: O.pcg_amg given the device's aggregates and the degrees, interval, scale and cycle the device reports).

A handle's row count is fixed when it is created: a mesh of another size (``test_another_mesh_in_the_same_object``) comes
through ``initialise`` on the same Python object -- a new handle that draws its blocks from the same process-wide pool.

Not reachable on one rank: a level-0 bound left by the assembly kernel (``asm_bound_fresh``) that outlives the hierarchy it
was written for.  The sites of one rank that drop the hierarchy (a mesh upload, a pattern build) also drop the assembled
values, and the assembly a solve needs after them writes the flag afresh (the fourth site is the neighbour plan of several
ranks).  The flag is cleared at those sites all the same; ``test_assembly_mode_between_assemblies`` turns the shortcut off
and on.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import pfemfort_amd as pf
from oracle import pfem_oracle as O
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
from test_gpu_parity import U_ATOL, _moved, _transfers

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOBS = ("cheb_degree", "fine_degree", "eig_ratio", "coarse_scale")
AMG_KEYS = KNOBS + ("levels", "rows", "nnz", "lambda_max")


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(kind, mesh, elemData, other elemData on the same pattern)."""
    if name == "tet10":           # 729 rows: no multiple of 4, its last 256-row slice partial
        return pf.POISSON_TET, H.read_mesh(f"{GOLDEN}/input/tet10"), H.POISSON_ELEMDATA, np.array([2.0, 2.0, 2.0])
    if name in ("box", "box_moved", "box_aniso"):      # 13 x 11 x 9 free nodes: a lattice, bricks, a value dictionary
        m = H.gen_box_tets(-1, 1, 14, -1, 1, 12, -1, 1, 10)
        # (box: K doubles -- the same aggregates, every value new; box_aniso: other conductivities per axis, for the loops
        # that form no aggregates)
        other = np.array([1.3, 0.7, 2.1]) if name == "box_aniso" else np.array([2.0, 2.0, 2.0])
        return pf.POISSON_TET, (_moved(m, 2.0 / 14) if name == "box_moved" else m), H.POISSON_ELEMDATA, other
    if name == "cube30":
        return pf.POISSON_TET, H.gen_box_tets(-1, 1, 30, -1, 1, 30, -1, 1, 30), H.POISSON_ELEMDATA, None
    if name == "beam":            # 3-row groups, rigid-body modes, node-block Jacobi
        other = np.array(H.ELAST_ELEMDATA, dtype=np.float64).copy()
        other[0] *= 1.7           # another Young's modulus: every entry scaled
        return (pf.ELAST_TET, H.gen_box_tets(-0.5, 0.5, 6, 0.0, 6.0, 36, -0.5, 0.5, 6, bc_mode=1, ndof=3),
                H.ELAST_ELEMDATA, other)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _setup(name):
    kind, mesh, _, _ = _mesh(name)
    return D._setup(kind, mesh)


def _forces(name):
    """A few nodal forces on free dofs (VecSetValue ADD_VALUES after the element loop)."""
    n = _setup(name)[0].size_global
    g = np.arange(7, n, max(1, n // 6))[:6]
    return g, np.linspace(0.05, 0.3, len(g))


def _cfg(mesh, **kw):
    """A configuration as plain data."""
    c = dict(mesh=mesh, values="first", forces=False, pc="jacobi", single=False, fmt="grouped" if mesh == "beam" else "auto",
             mode="gather", amg=None, cycle=None, rtol=1e-10, maxits=20000, stream=None)
    c.update(kw)
    return c


def _assemble(s, c):
    _, _, ed, other = _mesh(c["mesh"])
    s.assemble(ed if c["values"] == "first" else other, H.TIMEDATA)
    if c["forces"]:
        s.addNodalForces(*_forces(c["mesh"]))


def _load(s, c):
    """uploadMesh -> buildPattern -> assemble (a mesh of another row count: a new handle of that size first)."""
    kind = _mesh(c["mesh"])[0]
    dm, conn, xyz, edof = _setup(c["mesh"])
    if not s._h or s.size_global != dm.size_global:
        s.initialise(dm.size_global, dm.size_global)
    if c["stream"] is not None:
        s.setStream(c["stream"])
    s.setSpmvFormat(c["fmt"])
    s.setAssemblyMode(c["mode"])
    s.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    s.buildPattern()
    _assemble(s, c)


def _settings(s, c):
    s.setSpmvFormat(c["fmt"])
    s.setAssemblyMode(c["mode"])
    s.setPreconditioner(c["pc"])
    s.setSingleReduction(c["single"])
    if c["amg"] is not None:
        s.setAmgOptions(*c["amg"])
    if c["cycle"] is not None:
        s.setAmgCycle(c["cycle"])
    s.setTolerances(rtol=c["rtol"], maxits=c["maxits"])
    if c["stream"] is not None:
        s.setStream(c["stream"])


def _fingerprint(s):
    fp = {}
    if s.preconditioner() == "gamg":             # (first: a stale knob is named before the iterations it costs)
        info = s.amgInfo()
        fp.update({k: info[k] for k in AMG_KEYS})
        fp["cycle"] = s.amgCycle()
    fp.update({"its": s.its, "reason": s.reason, "rnorm": s.norm, "history": s.getHistory(), "solution": s.getSolution()})
    return fp


def _fresh(c):
    """A new object for configuration ``c``, solved once and freed: its fingerprint."""
    s = pf.PetscSolver()
    try:
        _load(s, c)
        _settings(s, c)
        s.factoriseAndSolve()
        return _fingerprint(s)
    finally:
        s.free()


def _same(a, b, where):
    assert a.keys() == b.keys(), where
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (where, k)
        else:
            assert a[k] == b[k], (where, k, "reused", a[k], "fresh", b[k])


def _close(a, b, where):
    """The same solve up to the order of floating-point atomics: knobs, hierarchy sizes and cycle equal, the rest close."""
    for k in KNOBS + ("levels", "rows", "nnz", "cycle"):
        assert a.get(k) == b.get(k), (where, k, "reused", a.get(k), "fresh", b.get(k))
    assert a["reason"] == b["reason"] and abs(a["its"] - b["its"]) <= 1, (where, a["its"], b["its"])
    scale = max(1.0, np.abs(b["solution"]).max())
    assert np.abs(a["solution"] - b["solution"]).max() <= 1e-9 * scale, where


def _oracle_check(s, c, where):
    """The solve that just ran against the oracle's restatement of the same loop on the device's own system."""
    rowptr, cols, vals = s.getCSR()
    b = s.getRHS()
    x, h = s.getSolution(), s.getHistory()
    its, reason = s.its, s.reason
    rtol, maxits = c["rtol"], c["maxits"]
    elast = _mesh(c["mesh"])[0] == pf.ELAST_TET
    pc = s.preconditioner()
    if pc == "gamg":
        info, cyc = s.amgInfo(), s.amgCycle()
        xo, ito, ro, _, hist = O.pcg_amg(rowptr, cols, vals, b, _transfers(s, info), cheb_degree=info["cheb_degree"],
                                         fine_degree=info["fine_degree"], eig_ratio=info["eig_ratio"], coarse_scale=info["coarse_scale"],
                                         rtol=rtol, maxits=maxits, gamma=2 if cyc["cycle"] == "w" else 1,
                                         gamma_to=cyc["last_level_visited_twice"])
        slack = max(1, ito // 50)
        m = min(len(h), len(hist), 30)
        assert np.abs(h[:m] - hist[:m]).max() <= 1e-6 * hist[0], where
    else:
        if pc == "pbjacobi":
            xo, ito, ro, _ = O.pcg_block_jacobi(rowptr, cols, vals, b, O.row_groups(rowptr, cols), rtol=rtol, maxits=maxits)
        else:
            f = O.pcg_jacobi_single_reduction if c["single"] else O.pcg_jacobi
            xo, ito, ro, _, hist = f(rowptr, cols, vals, b, rtol=rtol, maxits=maxits, hist_len=len(h) + 64)
            m = min(len(h), len(hist), 30 if elast else 200)      # (the slender beam amplifies rounding along the history)
            assert m >= min(its, ito, 30) and np.allclose(h[:m], hist[:m], rtol=1e-6), where
        slack = max(3, ito // 25) if elast else 1      # (the beam's 600-iteration runs: rounding moves the end by up to 3 %)
    assert reason == ro and abs(its - ito) <= (0 if reason < 0 else slack), (where, its, reason, ito, ro)
    scale = max(1.0, np.abs(xo).max())
    if reason < 0 or (pc == "gamg" and (rtol <= 1e-10 or its == ito)):
        assert np.abs(x - xo).max() <= 1e-9 * scale, where
    elif pc != "gamg":
        xc, *_ = O.pcg_jacobi(rowptr, cols, vals, b, rtol=1e-12, maxits=100000)
        assert np.abs(x - xc).max() <= (U_ATOL if rtol <= 1e-10 else 1e-3) * scale, where
    else:
        assert np.abs(x - xo).max() <= 1e-3 * scale, where


def _run(steps, compare=None, after=None):
    """``steps``: (what, configuration) -- what = "load" (mesh, pattern, assembly), "assemble", "forces" (addNodalForces) or
    "set" (setters only).  ``compare[i]``: "bits" (default), "close" (the last assembly summed with atomics) or "knobs" (only
    the gamg knobs and the cycle against the fresh object's; the oracle check still holds)."""
    compare = compare or ["bits"] * len(steps)
    ref = [_fresh(c) for _, c in steps]            # first: the reused object has allocated nothing yet
    s = pf.PetscSolver()
    try:
        for i, ((what, c), how) in enumerate(zip(steps, compare)):
            where = f"step {i}: {what} -> " + ", ".join(f"{k}={v}" for k, v in c.items() if k == "mesh" or v != _cfg(c["mesh"])[k])
            if what == "load":
                _load(s, c)
            _settings(s, c)
            if what == "assemble":
                _assemble(s, c)
            elif what == "forces":
                s.addNodalForces(*_forces(c["mesh"]))
            s.factoriseAndSolve()
            fp = _fingerprint(s)
            if how == "bits":
                _same(fp, ref[i], where)
            elif how == "close":
                _close(fp, ref[i], where)
            else:
                for k in KNOBS + ("cycle",):
                    assert fp[k] == ref[i][k], (where, k, "reused", fp[k], "fresh", ref[i][k])
            _oracle_check(s, c, where)
            if after:
                after(s, c, where)
    finally:
        s.free()


# ---- 1. new element data on the same pattern ----------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,pc,single,fmt", [("box_aniso", "jacobi", False, "grouped"),     # level 0's dictionary re-encoded
                                                ("box_aniso", "jacobi", True, "auto"),
                                                ("beam", "pbjacobi", False, "grouped"),
                                                ("box", "gamg", False, "grouped"),
                                                ("beam", "gamg", False, "grouped")])
def test_new_element_data_same_pattern(mesh, pc, single, fmt):
    cfg = functools.partial(_cfg, mesh, pc=pc, single=single, fmt=fmt)
    _run([("load", cfg()), ("assemble", cfg(values="other")), ("assemble", cfg())])


# ---- 2. nodal forces after a solve, then a new assembly -----------------------------------------------------------------
@pytest.mark.parametrize("mesh,pc", [("beam", "jacobi"), ("box", "gamg")])
def test_nodal_forces_after_a_solve(mesh, pc):
    cfg = functools.partial(_cfg, mesh, pc=pc)
    _run([("load", cfg()), ("forces", cfg(forces=True)), ("assemble", cfg())])


# ---- 3. preconditioner switches on one object --------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [None, "1"])
def test_preconditioner_switches(graph, monkeypatch):
    if graph is None:
        monkeypatch.delenv("PFEM_CG_GRAPH", raising=False)
    else:
        monkeypatch.setenv("PFEM_CG_GRAPH", graph)
    _run([("load", _cfg("beam", pc="jacobi"))] + [("set", _cfg("beam", pc=pc)) for pc in ("gamg", "jacobi", "pbjacobi", "gamg")])


# ---- 4. single reduction on -> off -> on --------------------------------------------------------------------------------
def test_single_reduction_toggled():
    _run([("load", _cfg("box", single=True)), ("set", _cfg("box", single=False)), ("set", _cfg("box", single=True))])


# ---- 5. setStream ------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime the library is linked against (loaded in this process with the library)."""
    L.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    assert paths
    hip = C.CDLL(paths[0])
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamCreate.restype = C.c_int
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.restype = C.c_int
    return hip


@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
def test_set_stream_between_solves(pc, monkeypatch):
    """A created stream -> 0 (the legacy default stream) -> a second created stream -> 0.  Below kGraphMaxRows with
    PFEM_CG_GRAPH=1 the Jacobi loop captures its graph again on every created stream; on the null stream capture may be
    refused and the loop enqueue on the stream: only the bits are asserted there (and for gamg's graph)."""
    monkeypatch.setenv("PFEM_CG_GRAPH", "1")
    hip = _hip_runtime()
    streams = []
    try:
        for _ in range(2):
            h = C.c_void_p()
            assert hip.hipStreamCreate(C.byref(h)) == 0 and h.value
            streams.append(h.value)
        a, b = streams

        def graph_replayed(s, c, where):
            if c["pc"] == "jacobi" and c["stream"]:
                assert s.timings()["graph_iterations"] > 0, where

        _run([("load", _cfg("box", pc=pc, stream=a))] + [("set", _cfg("box", pc=pc, stream=st)) for st in (0, b, 0)], after=graph_replayed)
    finally:
        for h in streams:                   # (every solver is back on 0 -- or freed -- by now)
            hip.hipStreamDestroy(h)


# ---- 6. setAmgOptions between gamg solves on one hierarchy --------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["box", "beam"])
def test_amg_options_between_solves(mesh):
    """defaults -> (cheb 3, fine 2, eig_ratio 30, coarse_scale 1.2) -> (1, 0, automatic, automatic) -> defaults: a knob returned
    to automatic takes the automatic value of the hierarchy's symbolic phase, not the value it was given before."""
    cfg = functools.partial(_cfg, mesh, pc="gamg")
    _run([("load", cfg()), ("set", cfg(amg=(3, 2, 30.0, 1.2))), ("set", cfg(amg=(1, 0, None, None))), ("set", cfg(amg=(2, 1, None, None)))])


# ---- 7. setAmgCycle between gamg solves on one hierarchy ----------------------------------------------------------------
def test_amg_cycle_between_solves(monkeypatch):
    """v -> w -> v -> auto on matched aggregates (the moved box: the W has a coarse problem to visit twice)."""
    monkeypatch.setenv("PFEM_AMG_LATTICE_BY_NUMBERING", "0")
    cfg = functools.partial(_cfg, "box_moved", pc="gamg")
    _run([("load", cfg(cycle="v"))] + [("set", cfg(cycle=cy)) for cy in ("w", "v", "auto")])


# ---- 8. setSpmvFormat between solves without buildPattern ----------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
def test_spmv_format_between_solves(pc):
    """auto -> int32 -> gaps16 -> grouped without a new pattern.  Jacobi: the fresh object's bits.  gamg: whether the hierarchy
    is kept is not pinned, only that its solve is the oracle's given the device's current aggregates (no dropped form read)."""
    cfg = functools.partial(_cfg, "box", pc=pc)
    how = ["bits"] + (["bits"] * 3 if pc == "jacobi" else ["knobs"] * 3)
    _run([("load", cfg(fmt="auto"))] + [("set", cfg(fmt=f)) for f in ("int32", "gaps16", "grouped")], compare=how)


# ---- 9. setAssemblyMode between assemblies ------------------------------------------------------------------------------
def test_assembly_mode_between_assemblies():
    """gather -> scatter -> gather with gamg: the scatter step has no level-0 bound from the assembly kernel, the gather step
    after it has one again.  (The scatter step's sums come in the order of the atomics: close to the fresh object, not equal.)"""
    cfg = functools.partial(_cfg, "box", pc="gamg")
    _run([("load", cfg(mode="gather")), ("assemble", cfg(mode="scatter")), ("assemble", cfg(mode="gather"))],
         compare=["bits", "close", "bits"])


# ---- 10. another mesh in the same object ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("change", ["size", "moved"])
def test_another_mesh_in_the_same_object(change, pc, monkeypatch):
    """uploadMesh -> buildPattern -> assemble -> solve each time.  "size": the 30^3 box -> tet10 -> the 30^3 box (blocks a
    larger problem used come back holding its data: SpMV guard bands, padded slices, partial sums).  "moved": the box -> its
    nodes moved -> the box, in one handle: lattice <-> matching, value dictionary <-> fp64 copy."""
    if change == "size":
        meshes, fmt = ("cube30", "tet10", "cube30"), "auto"
    else:
        monkeypatch.setenv("PFEM_AMG_LATTICE_BY_NUMBERING", "0")
        meshes, fmt = ("box", "box_moved", "box"), "grouped"
    _run([("load", _cfg(m, pc=pc, fmt=fmt)) for m in meshes])


# ---- 11. tolerances on one assembled system ------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
def test_tolerances_between_solves(pc):
    """maxits 2 (KSP_DIVERGED_ITS) -> rtol 1e-10 -> rtol 1e-5."""
    cfg = functools.partial(_cfg, "box", pc=pc)
    _run([("load", cfg(maxits=2)), ("set", cfg()), ("set", cfg(rtol=1e-5))])
