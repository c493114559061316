"""``PetscSolver`` -- Python mirror of ``TYPE PetscSolver`` (MODULE Module_SolverPetsc,
solverpetsc.F:72-105) over the C ABI.  Same procedure names, argument meaning and status
machine as the reference; the linear algebra runs in hand-written HIP kernels on the GPU.
There is no CPU fallback: constructing the device object without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as L
from ._lib import (ADD_VALUES, ASSEMBLY_OK, FACTORISE_OK, INIT_OK, INSERT_VALUES,  # noqa: F401
                   PATTERN_OK, SOLVER_EMPTY)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


ModalResult = namedtuple("ModalResult", "omega omega2 modes residuals iterations restarts reason block pc")
SolveManyResult = namedtuple("SolveManyResult", "x iterations reasons rnorm pc")
BucklingResult = namedtuple("BucklingResult", "theta factors modes residuals iterations restarts reason block pc")


class PetscSolver:
    """Drop-in for ``solverpetsc`` in the drivers (``call solverpetsc%initialise(...)`` ...)."""

    def __init__(self):
        self._h = C.c_void_p(None)
        self.nRow = self.nCol = 0
        self.its = 0
        self.reason = 0
        self.norm = 0.0
        self._keep = []          # ctypes callbacks / tensors that must outlive the handle

    # ---- solverpetsc.F:116-214 -------------------------------------------------------
    def initialise(self, size_local, size_global, diag_nnz=None, offdiag_nnz=None, row_start=0, device=-1):
        if self._h:
            self.free()
        dn = None if diag_nnz is None else _i32(diag_nnz)
        on = None if offdiag_nnz is None else _i32(offdiag_nnz)
        h = C.c_void_p(None)
        L.check(L.lib().pfem_solver_create(C.byref(h), size_local, size_global, row_start, _p(dn), _p(on), device),
                "PetscSolver%initialise")
        self._h = h
        self.nRow = self.nCol = size_global
        self.size_local, self.size_global, self.row_start = size_local, size_global, row_start
        return self

    @property
    def currentStatus(self):
        st = C.c_int(0)
        L.check(L.lib().pfem_solver_status(self._h, C.byref(st)), "PetscSolver%currentStatus")
        return st.value

    def setTolerances(self, rtol=1e-5, abstol=1e-50, dtol=1e5, maxits=10000):
        """KSPSetFromOptions stand-in (petsc_options.dat is not part of the reference tree)."""
        L.check(L.lib().pfem_solver_set_tolerances(self._h, rtol, abstol, dtol, maxits), "PetscSolver%setTolerances")

    def setStream(self, hip_stream):
        L.check(L.lib().pfem_solver_set_stream(self._h, C.c_void_p(hip_stream)), "PetscSolver%setStream")

    # ---- solverpetsc.F:222-246 -------------------------------------------------------
    def setZero(self):
        L.check(L.lib().pfem_solver_set_zero(self._h), "PetscSolver%setZero")

    # ---- solverpetsc.F:254-278 -------------------------------------------------------
    def free(self, collective=True):
        """``collective``: the explicit call of a multi-rank run, made by every rank while the process group lives -- the
        communication backend's teardown step (pfem_solver_comm_shutdown: a barrier of the peer-memory transport) runs first.
        The garbage collector's call is not collective."""
        if self._h:
            if collective and self._keep:            # (hooks are kept alive here: a backend was attached)
                L.lib().pfem_solver_comm_shutdown(self._h)
            L.lib().pfem_solver_destroy(self._h)
            self._h = C.c_void_p(None)
        self._keep.clear()

    def __del__(self):
        try:
            self.free(collective=False)
        except Exception:
            pass

    # ---- solverpetsc.F:286-320 -------------------------------------------------------
    def printInfo(self):
        L.check(L.lib().pfem_solver_print_info(self._h), "PetscSolver%printInfo")

    # ---- the PETSc calls the drivers make on solverpetsc%mtx / %rhsVec ---------------
    def MatSetValues(self, idxm, idxn, v, mode):
        """``MatSetValues(mtx,m,idxm,n,idxn,v,mode)``; ``v`` is read row-major like PETSc does
        (pass the Fortran-ordered Klocal's memory, i.e. ``np.asfortranarray(K).ravel(order='K')``)."""
        idxm = _i32(idxm); idxn = _i32(idxn)
        vv = None if v is None else _f64(v).ravel()
        L.check(L.lib().pfem_mat_set_values(self._h, len(idxm), _p(idxm), len(idxn), _p(idxn), _p(vv), mode),
                "MatSetValues")

    def VecSetValues(self, idx, v, mode):
        idx = _i32(idx)
        L.check(L.lib().pfem_vec_set_values(self._h, len(idx), _p(idx), _p(_f64(v)), mode), "VecSetValues")

    # ---- solverpetsc.F:328-401 -------------------------------------------------------
    def assembleMatrixAndVector(self, R, Cc, Klocal, Flocal):
        K = None if Klocal is None else np.asfortranarray(Klocal, dtype=np.float64)
        F = None if Flocal is None else _f64(Flocal)
        R = _i32(R); Cc = _i32(Cc)
        L.check(L.lib().pfem_solver_assemble_matrix_and_vector(self._h, len(R), _p(R), _p(Cc), _p(K), _p(F)),
                "PetscSolver%assembleMatrixAndVector")

    def assembleMatrix(self, R, Cc, Klocal):
        self.assembleMatrixAndVector(R, Cc, Klocal, None)

    def assembleVector(self, R, Flocal):
        self.assembleMatrixAndVector(R, R, None, Flocal)

    # ---- solverpetsc.F:409-509 -------------------------------------------------------
    def factorise(self):
        L.check(L.lib().pfem_solver_factorise(self._h), "PetscSolver%factorise")

    def _solve(self, fn, where):
        its = C.c_int(0); reason = C.c_int(0); rn = C.c_double(0)
        L.check(fn(self._h, C.byref(its), C.byref(reason), C.byref(rn)), where)
        self.its, self.reason, self.norm = its.value, reason.value, rn.value
        return self.its, self.reason, self.norm

    def solve(self):
        return self._solve(L.lib().pfem_solver_solve, "PetscSolver%solve")

    def factoriseAndSolve(self):
        return self._solve(L.lib().pfem_solver_factorise_and_solve, "PetscSolver%factoriseAndSolve")

    def getSolution(self):
        """VecGetArray(solnVec): the owned block of the solution."""
        x = np.empty(self.size_local)
        L.check(L.lib().pfem_solver_get_solution(self._h, _p(x)), "VecGetArray")
        return x

    def getHistory(self):
        h = np.empty(self.its + 1)
        n = C.c_int(0)
        L.check(L.lib().pfem_solver_get_history(self._h, _p(h), len(h), C.byref(n)), "pfem_solver_get_history")
        return h[:n.value]

    # ---- batched device path (the element loop as one call) --------------------------
    def uploadMesh(self, kind, conn, xyz, edof, solnApplied):
        conn = _i32(conn); xyz = _f64(xyz); edof = _i32(edof); sa = _f64(solnApplied)
        assert conn.shape[0] == L.NPELEM[kind] and xyz.shape[0] == L.NDIM[kind]
        assert edof.shape == (L.NPELEM[kind] * L.NDOF[kind], conn.shape[1])
        assert sa.size == xyz.shape[1] * L.NDOF[kind]
        L.check(L.lib().pfem_mesh_upload(self._h, kind, conn.shape[1], _p(conn), xyz.shape[1], _p(xyz), _p(edof), _p(sa)),
                "pfem_mesh_upload")
        self.kind = kind
        self.nElem = conn.shape[1]
        self.nNode = xyz.shape[1]

    def generateBoxMesh(self, kind, x0, x1, nEx, y0, y1, nEy, z0, z1, nEz, bc_mode=0, nparts=1, part=0, axis=2):
        """The structured box of genTetra.cpp + the driver's numbering for slab ``part`` of ``nparts`` along ``axis``
        (0 x, 1 y, 2 z, -1 the longest), generated on the device (the solver must have been initialised with
        ``host.box_slab_sizes`` for the same axis)."""
        L.check(L.lib().pfem_mesh_generate_box_axis(self._h, kind, x0, x1, nEx, y0, y1, nEy, z0, z1, nEz, bc_mode, axis, nparts, part),
                "pfem_mesh_generate_box_axis")
        self.kind = kind
        sz = L.lib().pfem_box_slab_sizes_axis
        n = C.c_int64(0); ne = C.c_int64(0)
        L.check(sz(nEx, nEy, nEz, bc_mode, L.NDOF[kind], axis, nparts, part, None, None, None, C.byref(n), C.byref(ne), None, None, None),
                "pfem_box_slab_sizes_axis")
        self.nElem, self.nNode = ne.value, n.value

    def downloadMesh(self):
        """(conn, xyz, edof_local, solnApplied) as the device holds them."""
        npe, ndof, ndim = L.NPELEM[self.kind], L.NDOF[self.kind], L.NDIM[self.kind]
        conn = np.empty((npe, self.nElem), np.int32); xyz = np.empty((ndim, self.nNode))
        edof = np.empty((npe * ndof, self.nElem), np.int32); sa = np.empty(self.nNode * ndof)
        L.check(L.lib().pfem_mesh_download(self._h, _p(conn), _p(xyz), _p(edof), _p(sa)), "pfem_mesh_download")
        return conn, xyz, edof, sa

    # ---- several materials -------------------------------------------------------------
    def setMaterials(self, elem_mat, n_mat=None, stride=None):
        """Material id of every element (``elem_mat[e]`` in ``0 .. n_mat-1``, at most 256 materials; the element order of
        ``uploadMesh``'s ``conn`` / of ``host.gen_box_tets`` for a generated box).  From here on ``assemble``, ``evalElems``,
        ``elementFields``, ``nodalForces``, ``nodalRecovery`` and ``errorIndicator`` take a 2-D ``(n_mat, stride)`` table as
        ``elemData`` and element ``e`` uses row ``elem_mat[e]``.  The stride is fixed HERE, not at first use: ``stride`` (default:
        the kind's count of elemData entries -- Poisson tet 3, Poisson triangle 2, elastic tet 6, elastic triangle 5), and every
        later table must have that many columns.  ``n_mat`` defaults to ``max(elem_mat) + 1``.  Legal between the mesh and
        ``buildPattern``; ``elem_mat=None`` clears the map, and so does a new mesh.  One rank only."""
        if elem_mat is None:
            L.check(L.lib().pfem_mesh_set_materials(self._h, 0, None, 0, 0), "pfem_mesh_set_materials")
            return
        em = _i32(elem_mat).ravel()
        if n_mat is None:
            n_mat = int(em.max()) + 1 if em.size else 1
        if stride is None:
            stride = L.NELEMDATA.get(getattr(self, "kind", None), 0)
        L.check(L.lib().pfem_mesh_set_materials(self._h, em.size, _p(em), int(n_mat), int(stride)), "pfem_mesh_set_materials")

    def materials(self):
        """``(elem_mat, n_mat, stride)`` of the map in effect, or ``None`` without one."""
        n = C.c_int(0); st = C.c_int(0)
        L.check(L.lib().pfem_mesh_get_materials(self._h, C.byref(n), C.byref(st), None), "pfem_mesh_get_materials")
        if n.value == 0:
            return None
        em = np.empty(self.nElem, np.int32)
        L.check(L.lib().pfem_mesh_get_materials(self._h, C.byref(n), C.byref(st), _p(em)), "pfem_mesh_get_materials")
        return em, n.value, st.value

    def _elem_data(self, elemData):
        """``elemData`` as the library reads it: one vector, or -- while a material map is set -- the ``(n_mat, stride)`` table."""
        if elemData is None:
            return None
        ed = _f64(elemData)
        n = C.c_int(0); st = C.c_int(0)
        if self._h and getattr(self, "kind", None) is not None:
            L.check(L.lib().pfem_mesh_get_materials(self._h, C.byref(n), C.byref(st), None), "pfem_mesh_get_materials")
        if n.value:
            if ed.shape != (n.value, st.value):
                raise ValueError(f"elemData of shape {ed.shape}: the material map wants a ({n.value}, {st.value}) table")
        elif ed.ndim != 1:
            raise ValueError("a 2-D elemData table needs a material map (setMaterials)")
        return ed

    def buildPattern(self):
        L.check(L.lib().pfem_pattern_build(self._h), "pfem_pattern_build")

    def setAssemblyMode(self, mode):
        """"gather" (default: no atomics, bit-reproducible) or "scatter" (f64 atomics)."""
        L.check(L.lib().pfem_solver_set_assembly_mode(self._h, {"gather": 0, "scatter": 1}[mode]),
                "pfem_solver_set_assembly_mode")

    def assemblyInfo(self):
        """{"gather": bool, "hub_nodes": n, "block_threads": T, "lds_bytes": b} for the current pattern."""
        g = C.c_int(0); h = C.c_int(0); t = C.c_int(0); b = C.c_int64(0)
        L.check(L.lib().pfem_solver_assembly_info(self._h, C.byref(g), C.byref(h), C.byref(t), C.byref(b)), "pfem_solver_assembly_info")
        return {"gather": bool(g.value), "hub_nodes": h.value, "block_threads": t.value, "lds_bytes": b.value}

    def setSpmvFormat(self, fmt):
        """"auto" (16-bit column gaps when they fit; row groups when the pattern has them and the system is large),
        "grouped" (row groups at any size), "gaps16" (16-bit gaps, one row per lane) or "int32"."""
        L.check(L.lib().pfem_solver_set_spmv_format(self._h, {"auto": 0, "int32": 1, "gaps16": 2, "grouped": 3}[fmt]), "pfem_solver_set_spmv_format")

    def spmvColumnBits(self):
        b = C.c_int(0)
        L.check(L.lib().pfem_solver_get_spmv_format(self._h, C.byref(b)), "pfem_solver_get_spmv_format")
        return b.value

    def spmvGapTable(self):
        """Entries of the table of distinct large gaps (dictionary form of the relative row groups), 0 otherwise."""
        b = C.c_int(0)
        L.check(L.lib().pfem_solver_get_spmv_gap_table(self._h, C.byref(b)), "pfem_solver_get_spmv_gap_table")
        return b.value

    def spmvValueDictionary(self):
        """Distinct matrix values in the SpMV's dictionary when it streams 16-bit value codes (structured meshes), else 0."""
        b = C.c_int(0)
        L.check(L.lib().pfem_solver_get_spmv_value_dictionary(self._h, C.byref(b)), "pfem_solver_get_spmv_value_dictionary")
        return b.value

    def amgValueDictionaries(self):
        """Per level of the last gamg hierarchy: distinct values in the level's dictionary when its SpMVs stream 16-bit value codes
        (0: fp64 values)."""
        n = C.c_int(0)
        e = (C.c_int * 32)()
        L.check(L.lib().pfem_solver_amg_value_dictionaries(self._h, 32, C.byref(n), e), "pfem_solver_amg_value_dictionaries")
        return list(e[:n.value])

    def spmvGapEscapes(self):
        """True when the row form streams 16-bit gaps with escapes to the int32 column array (k_spmv16e)."""
        b = C.c_int(0)
        L.check(L.lib().pfem_solver_get_spmv_gap_escapes(self._h, C.byref(b)), "pfem_solver_get_spmv_gap_escapes")
        return bool(b.value)

    def setPreconditioner(self, pc):
        """"jacobi" (default; PCJACOBI), "pbjacobi" (node-block Jacobi, PETSc's -pc_type pbjacobi) or "gamg" (plain-aggregation
        multigrid V-cycle, PETSc's -pc_type gamg; one rank)."""
        L.check(L.lib().pfem_solver_set_preconditioner(self._h, {"jacobi": 0, "pbjacobi": 1, "gamg": 2}[pc]), "pfem_solver_set_preconditioner")

    def setSingleReduction(self, on=True):
        """KSPCGUseSingleReduction (-ksp_cg_single_reduction): one all-reduce per CG iteration instead of two
        (``None``: leave it to PFEM_CG_SINGLE_REDUCTION)."""
        L.check(L.lib().pfem_solver_set_cg_single_reduction(self._h, -1 if on is None else int(bool(on))),
                "pfem_solver_set_cg_single_reduction")

    def preconditioner(self):
        """The preconditioner the next solve uses ("pbjacobi" needs 3-dof row groups and one rank)."""
        b = C.c_int(0)
        L.check(L.lib().pfem_solver_get_preconditioner(self._h, C.byref(b)), "pfem_solver_get_preconditioner")
        return ("jacobi", "pbjacobi", "gamg")[b.value]

    def setAmgOptions(self, cheb_degree=2, fine_degree=1, eig_ratio=None, coarse_scale=None):
        """-pc_gamg knobs: Chebyshev degree on the coarse levels / on the assembled matrix (0: the same), lmax/lmin of the
        smoothing interval, scaling of the coarse-grid correction (``None``: that knob is automatic -- 16 / 1.5 for scalar
        problems and for displacement problems with rigid-body modes, 8 / 1.8 for 3-dof nodes without them: what
        amg_symbolic picks for the hierarchy, pfem_amg.inc -- also when it was given a value before)."""
        L.check(L.lib().pfem_solver_set_amg_options(self._h, cheb_degree, fine_degree, -1.0 if eig_ratio is None else eig_ratio,
                                                    -1.0 if coarse_scale is None else coarse_scale), "pfem_solver_set_amg_options")

    def setAmgCycle(self, cycle=None):
        """-pc_mg_cycle_type: "v" (the default, also ``None``) or "w" (every coarse problem above the cycle's tail visited twice)."""
        code = {None: 0, "auto": 0, "v": 1, "w": 2}[cycle.lower() if isinstance(cycle, str) else cycle]
        L.check(L.lib().pfem_solver_set_amg_cycle(self._h, code), "pfem_solver_set_amg_cycle")

    def amgCycle(self):
        """What the last gamg solve ran: {"cycle": "v" | "w", "last_level_visited_twice": l (0 with the V-cycle),
        "level0_epilogue": the cycle's last fine product carried the final smoothing step and the CG's sums,
        "tail_from": first level of the one-workgroup tail launch (-1: the cycle went level by level to the bottom),
        "tail_build": None | "memory" | "lds" | "lds+matrix" (where that launch kept the levels' vectors and the first level's matrix),
        "column_codes": the levels whose fused products read one-byte column codes, "column_code_builds": how many times this
        hierarchy has built a level's column codes}."""
        c, w, e, t, tb, bp = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(-1), C.c_int(0), C.c_int(0)
        L.check(L.lib().pfem_solver_amg_cycle(self._h, C.byref(c), C.byref(w)), "pfem_solver_amg_cycle")
        L.check(L.lib().pfem_solver_amg_level0_epilogue(self._h, C.byref(e)), "pfem_solver_amg_level0_epilogue")
        L.check(L.lib().pfem_solver_amg_tail_from(self._h, C.byref(t), C.byref(tb), C.byref(bp)), "pfem_solver_amg_tail_from")
        ncc, nb = C.c_int(0), C.c_int(0)
        cc = (C.c_int * 32)()
        L.check(L.lib().pfem_solver_amg_column_codes(self._h, 32, C.byref(ncc), cc, C.byref(nb)), "pfem_solver_amg_column_codes")
        return {"cycle": "w" if c.value == 2 else "v", "last_level_visited_twice": w.value, "level0_epilogue": bool(e.value),
                "tail_from": t.value, "tail_build": [None, "memory", "lds", "lds+matrix"][tb.value],
                "column_codes": list(cc[:ncc.value]), "column_code_builds": nb.value}

    def amgBoundsByProducts(self):
        """Coarse levels whose eigenvalue bound the last numeric set-up took from the Galerkin product that formed them, instead of
        the stand-alone maximum kernels (0 in a pattern's first solve, whose products run in the symbolic phase: a property of the
        solver's history, unlike amgCycle())."""
        t, tb, bp = C.c_int(-1), C.c_int(0), C.c_int(0)
        L.check(L.lib().pfem_solver_amg_tail_from(self._h, C.byref(t), C.byref(tb), C.byref(bp)), "pfem_solver_amg_tail_from")
        return bp.value

    def amgSideStream(self):
        """The side chain of the last gamg solve's numeric set-up: {"used": the products that form the levels from "first_level" on
        and the dense inverse ran on a stream of their own beside the first cycle's upper levels, "first_level": that level (0: none),
        "ms": the chain's span on its stream -- amgInfo()["numeric_ms"] then covers the solver's own stream only}.  Never used in a
        pattern's first solve, whose products run in the symbolic phase: a property of the solver's history, unlike amgCycle()."""
        u, k, ms = C.c_int(0), C.c_int(0), C.c_double(0)
        L.check(L.lib().pfem_solver_amg_side_stream(self._h, C.byref(u), C.byref(k), C.byref(ms)), "pfem_solver_amg_side_stream")
        return {"used": bool(u.value), "first_level": k.value, "ms": ms.value}

    def amgTransfer(self, level, xyz=False):
        """The transfer from ``level`` to the next: {"rbm": carries rotations?, "fine_bs", "coarse_bs", "dim", "n_nodes"} and, with
        ``xyz``, the level's node coordinates [3, n_nodes]."""
        rbm, fb, cb, dim = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        nn = C.c_int64(0)
        L.check(L.lib().pfem_solver_amg_transfer(self._h, level, C.byref(rbm), C.byref(fb), C.byref(cb), C.byref(dim), C.byref(nn), None), "pfem_solver_amg_transfer")
        out = {"rbm": bool(rbm.value), "fine_bs": fb.value, "coarse_bs": cb.value, "dim": dim.value, "n_nodes": nn.value}
        if xyz:
            a = np.empty((3, nn.value), np.float64)
            L.check(L.lib().pfem_solver_amg_transfer(self._h, level, C.byref(rbm), C.byref(fb), C.byref(cb), C.byref(dim), C.byref(nn), _p(a)), "pfem_solver_amg_transfer")
            out["xyz"] = a
        return out

    def incidencePatterns(self):
        """(patterns, longest list) of the gather form's incidence lists stored as translated copies; (0, 0): own records."""
        n = C.c_int(0); m = C.c_int(0)
        L.check(L.lib().pfem_solver_incidence_patterns(self._h, C.byref(n), C.byref(m)), "pfem_solver_incidence_patterns")
        return n.value, m.value

    def amgAggregation(self):
        """How every level's aggregates were formed: a list of "bricks" / "node-bricks" / "split-bricks" / "lattice-passes" /
        "matching" per transfer (one fewer than levels)."""
        mx = 32
        nl = C.c_int(0)
        kind = (C.c_int * mx)()
        L.check(L.lib().pfem_solver_amg_aggregation(self._h, mx, C.byref(nl), kind), "pfem_solver_amg_aggregation")
        names = {0: "none", 1: "bricks", 2: "node-bricks", 3: "split-bricks", 4: "lattice-passes", 5: "matching"}
        return [names.get(kind[l], str(kind[l])) for l in range(max(nl.value - 1, 0))]

    def amgInfo(self):
        """The multigrid hierarchy of the last ``gamg`` solve: rows / nonzeros / eigenvalue bound per level, phase times."""
        mx = 32
        nl = C.c_int(0); rows = (C.c_int64 * mx)(); nnz = (C.c_int64 * mx)(); lam = (C.c_double * mx)()
        sym = C.c_double(0); num = C.c_double(0); deg = C.c_int(0); fdeg = C.c_int(0); ratio = C.c_double(0); scale = C.c_double(0)
        L.check(L.lib().pfem_solver_amg_info(self._h, mx, C.byref(nl), rows, nnz, lam, C.byref(sym), C.byref(num), C.byref(deg),
                                             C.byref(fdeg), C.byref(ratio), C.byref(scale)), "pfem_solver_amg_info")
        n = nl.value
        gc = C.c_int(0)
        L.check(L.lib().pfem_solver_amg_galerkin_from_codes(self._h, C.byref(gc)), "pfem_solver_amg_galerkin_from_codes")
        return {"levels": n, "rows": list(rows[:n]), "nnz": list(nnz[:n]), "lambda_max": list(lam[:n]), "symbolic_ms": sym.value,
                "numeric_ms": num.value, "cheb_degree": deg.value, "fine_degree": fdeg.value, "eig_ratio": ratio.value, "coarse_scale": scale.value,
                "galerkin_from_codes": bool(gc.value)}

    def amgLevelValues(self, level):
        """The stored values of coarse ``level`` (>= 1) of the last hierarchy, in slot order (padding included)."""
        n = C.c_int64(0)
        L.check(L.lib().pfem_solver_amg_level_values(self._h, level, 0, None, C.byref(n)), "pfem_solver_amg_level_values")
        a = np.empty(n.value, np.float64)
        L.check(L.lib().pfem_solver_amg_level_values(self._h, level, n.value, _p(a), C.byref(n)), "pfem_solver_amg_level_values")
        return a

    def amgLevelColumns(self, level, decoded=False):
        """The columns of coarse ``level`` (>= 1) of the last hierarchy, in slot order (padding included): the level's int32 array,
        or -- ``decoded`` -- what the device decodes from the level's one-byte column codes and offset table."""
        n = C.c_int64(0)
        L.check(L.lib().pfem_solver_amg_level_columns(self._h, level, int(bool(decoded)), 0, None, C.byref(n)), "pfem_solver_amg_level_columns")
        a = np.empty(n.value, np.int32)
        L.check(L.lib().pfem_solver_amg_level_columns(self._h, level, int(bool(decoded)), n.value, _p(a), C.byref(n)), "pfem_solver_amg_level_columns")
        return a

    def amgLevelCSR(self, level):
        """Coarse ``level`` (>= 1) of the last hierarchy as ``(rowptr, cols, vals)``: plain CSR without the storage's padding, the
        columns of a row ascending (one rank)."""
        n, nnz = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().pfem_solver_amg_level_csr(self._h, level, None, None, None, C.byref(n), C.byref(nnz)), "pfem_solver_amg_level_csr")
        rowptr = np.empty(n.value + 1, np.int64)
        cols = np.empty(nnz.value, np.int32)
        vals = np.empty(nnz.value, np.float64)
        L.check(L.lib().pfem_solver_amg_level_csr(self._h, level, _p(rowptr), _p(cols), _p(vals), C.byref(n), C.byref(nnz)), "pfem_solver_amg_level_csr")
        return rowptr, cols, vals

    def amgApply(self, r):
        """``z = M^-1 r``: one application of the last gamg solve's cycle with the set-up that solve left (one rank; ``r`` and ``z`` in
        the caller's dof order).  Changes nothing the next solve reads."""
        r = _f64(r)
        assert r.ndim == 1 and r.size == self.matrixInfo()["n_local"]
        z = np.empty_like(r)
        L.check(L.lib().pfem_solver_amg_apply(self._h, _p(r), _p(z)), "pfem_solver_amg_apply")
        return z

    def amgAggregates(self, level, n_rows):
        """Coarse dof of every dof of ``level`` (``n_rows`` = amgInfo()["rows"][level])."""
        a = np.empty(n_rows, np.int32)
        L.check(L.lib().pfem_solver_amg_aggregates(self._h, level, _p(a)), "pfem_solver_amg_aggregates")
        return a

    def amgLayout(self):
        """Several ranks: {"coupled": one hierarchy across the ranks?, "distributed_levels": how many of its levels are spread
        over the ranks (the rest is held whole by every rank), "first_dof": [...], "local_rows": [...]} per level."""
        mx = 32
        cp, nd = C.c_int(0), C.c_int(0)
        first = np.zeros(mx, np.int64)
        loc = np.zeros(mx, np.int64)
        L.check(L.lib().pfem_solver_amg_layout(self._h, mx, C.byref(cp), C.byref(nd), _p(first), _p(loc)), "pfem_solver_amg_layout")
        nl = self.amgInfo()["levels"]
        ex, ar = C.c_int(0), C.c_int(0)
        L.check(L.lib().pfem_solver_amg_comm_counts(self._h, C.byref(ex), C.byref(ar)), "pfem_solver_amg_comm_counts")
        lat = C.c_int(0)
        L.check(L.lib().pfem_solver_amg_pairing(self._h, C.byref(lat)), "pfem_solver_amg_pairing")
        return {"coupled": bool(cp.value), "distributed_levels": nd.value, "first_dof": first[:nl].tolist(), "local_rows": loc[:nl].tolist(),
                "exchanges_per_cycle": ex.value, "allreduces_per_cycle": ar.value, "lattice_levels": lat.value}

    def amgCycleProfile(self):
        """One instrumented V-cycle of the hierarchy across the ranks (collective): per level the exchanges, their time and bytes;
        the cycle's all-reduces; the cycle's time."""
        mx = 32
        nl, na = C.c_int(0), C.c_int(0)
        ex = np.zeros(mx, np.int32); ms = np.zeros(mx, np.float64); dbl = np.zeros(mx, np.int64)
        ams, adbl, cyc = C.c_double(0), C.c_int64(0), C.c_double(0)
        L.check(L.lib().pfem_solver_amg_cycle_profile(self._h, mx, C.byref(nl), _p(ex), _p(ms), _p(dbl), C.byref(na), C.byref(ams), C.byref(adbl),
                                                      C.byref(cyc)), "pfem_solver_amg_cycle_profile")
        n = nl.value
        return {"cycle_ms": cyc.value, "exchanges_per_level": ex[:n].tolist(), "exchange_ms_per_level": ms[:n].tolist(),
                "exchange_bytes_per_level": (8 * dbl[:n]).tolist(), "allreduces": na.value, "allreduce_ms": ams.value, "allreduce_bytes": 8 * adbl.value}

    def spmvRowGroup(self):
        """Rows served by one lane of the current SpMV (3: row-grouped form)."""
        b = C.c_int(0)
        L.check(L.lib().pfem_solver_get_spmv_row_group(self._h, C.byref(b)), "pfem_solver_get_spmv_row_group")
        return b.value

    def spmvFormatBytes(self):
        """Bytes one launch of the selected SpMV form moves at best (its storage + x + y)."""
        b = C.c_int64(0)
        L.check(L.lib().pfem_solver_spmv_bytes(self._h, C.byref(b)), "pfem_solver_spmv_bytes")
        return b.value

    def assemble(self, elemData, timeData):
        ed = self._elem_data(elemData)
        L.check(L.lib().pfem_assemble(self._h, _p(ed), _p(_f64(timeData))), "pfem_assemble")

    def addNodalForces(self, global_dof, values):
        """VecSetValue(rhsVec, row, fact, ADD_VALUES) loop of the elasticity drivers (:971-982)."""
        g = np.ascontiguousarray(global_dof, dtype=np.int64); v = _f64(values)
        L.check(L.lib().pfem_rhs_add_values(self._h, len(g), _p(g), _p(v)), "pfem_rhs_add_values")

    # ---- surface loads (one rank, batched path) ----------------------------------------
    def boundaryFaces(self):
        """``(elem, side)`` of the sides that belong to exactly one element, sorted by (element, side): side ``f`` of an element
        is the face / edge opposite its local node ``f``, elements in the order of ``uploadMesh``'s ``conn`` (of
        ``host.gen_box_tets`` for a generated box).  Found on the device from the mesh alone, kept until the next mesh."""
        n = C.c_int64(0)
        L.check(L.lib().pfem_mesh_boundary_faces(self._h, C.byref(n), None, None), "pfem_mesh_boundary_faces")
        fe = np.empty(n.value, np.int32); fs = np.empty(n.value, np.int32)
        L.check(L.lib().pfem_mesh_boundary_faces(self._h, C.byref(n), _p(fe), _p(fs)), "pfem_mesh_boundary_faces")
        return fe, fs

    def surfaceGeometry(self, elem, side):
        """``(measure (nFace,), normal (ndim, nFace), nodes (npe-1, nFace))`` of any sides: area / length, the named element's
        outward unit normal, the side's nodes in ascending local order (caller's node numbering).  ``host.FaceLoad`` is the
        per-side mirror, bit for bit."""
        fe = _i32(elem).ravel(); fs = _i32(side).ravel()
        assert fe.size == fs.size
        kind = getattr(self, "kind", None)
        if kind is None:                       # no mesh on this handle: the library says so
            L.check(L.lib().pfem_surface_geometry(self._h, fe.size, _p(fe), _p(fs), None, None, None), "pfem_surface_geometry")
        n = fe.size
        meas = np.empty(n); nrm = np.empty((L.NDIM[kind], n)); nodes = np.empty((L.NPELEM[kind] - 1, n), np.int32)
        L.check(L.lib().pfem_surface_geometry(self._h, n, _p(fe), _p(fs), _p(meas), _p(nrm), _p(nodes)), "pfem_surface_geometry")
        return meas, nrm, nodes

    def addSurfaceLoad(self, elem, side, load, values, layout=None, elemData=None):
        """rhs += the consistent nodal loads of ``values`` on the sides ``(elem, side)``; after ``assemble`` (which zeroes the
        rhs), before the solve.  ``load``: "flux" (Poisson kinds; the normal flux into the body), "traction" (elasticity kinds,
        ndof components) or "pressure" (elasticity kinds; the traction ``-p n``), or the ``LOAD_*`` code.  ``layout``: "uniform"
        (``values (ncomp,)``), "face" (``(nFace, ncomp)``) or "face_node" (``(nFace, npe-1, ncomp)``, linear on each side);
        ``None`` infers it from ``values.shape`` (a trailing axis of one component may be left out).  ``elemData`` is read for
        the plane-stress triangle only (its thickness): the vector, or the table while a material map is set."""
        fe = _i32(elem).ravel(); fs = _i32(side).ravel()
        assert fe.size == fs.size
        code = {"flux": L.LOAD_FLUX, "traction": L.LOAD_TRACTION, "pressure": L.LOAD_PRESSURE}.get(load, load)
        kind = getattr(self, "kind", None)
        v = _f64(values)
        if kind is None:
            L.check(L.lib().pfem_rhs_add_surface_load(self._h, fe.size, _p(fe), _p(fs), int(code), 0, _p(v.ravel()), None),
                    "pfem_rhs_add_surface_load")
        ncomp = L.NDOF[kind] if code == L.LOAD_TRACTION else 1
        ns = L.NPELEM[kind] - 1
        sizes = {L.LOAD_UNIFORM: ncomp, L.LOAD_PER_FACE: fe.size * ncomp, L.LOAD_PER_FACE_NODE: fe.size * ns * ncomp}
        if layout is None:
            shapes = {L.LOAD_UNIFORM: [(ncomp,)] + ([()] if ncomp == 1 else []),
                      L.LOAD_PER_FACE: [(fe.size, ncomp)] + ([(fe.size,)] if ncomp == 1 else []),
                      L.LOAD_PER_FACE_NODE: [(fe.size, ns, ncomp)] + ([(fe.size, ns)] if ncomp == 1 else [])}
            fits = [k for k in (L.LOAD_UNIFORM, L.LOAD_PER_FACE, L.LOAD_PER_FACE_NODE) if v.shape in shapes[k]]
            if not fits:
                raise ValueError(f"values of shape {v.shape} fit no layout of {fe.size} sides with {ncomp} component(s)")
            lay = fits[0]
        else:
            lay = {"uniform": L.LOAD_UNIFORM, "face": L.LOAD_PER_FACE, "face_node": L.LOAD_PER_FACE_NODE}.get(layout, layout)
            if lay in sizes and v.size != sizes[lay]:
                raise ValueError(f"values of size {v.size}: layout {layout!r} wants {sizes[lay]}")
        ed = self._elem_data(elemData) if kind == L.ELAST_TRIA else None
        L.check(L.lib().pfem_rhs_add_surface_load(self._h, fe.size, _p(fe), _p(fs), int(code), int(lay), _p(v.ravel()), _p(ed)),
                "pfem_rhs_add_surface_load")

    def evalElems(self, elemData, timeData):
        ns = L.NPELEM[self.kind] * L.NDOF[self.kind]
        K = np.empty((self.nElem, ns, ns)); F = np.empty((self.nElem, ns))
        ed = self._elem_data(elemData)
        L.check(L.lib().pfem_eval_elems(self._h, _p(ed), _p(_f64(timeData)), _p(K), _p(F)), "pfem_eval_elems")
        return K.transpose(0, 2, 1).copy(), F     # column-major blocks -> K[e][i,j] = Klocal(i,j)

    # ---- post-processing of a solution (one rank, batched path) -----------------------
    def elementFields(self, elemData, u=None):
        """``(grad, flux, scalar)`` of every element for the nodal field ``u`` ((nNode, ndof) or flat, the caller's node numbering;
        ``None``: the last solve's): gradient / engineering Voigt strain and flux / stress as ``(ng, nElem)``, ``|q|`` / von Mises
        as ``(nElem,)`` (``host.ElementPost`` is the per-element mirror)."""
        kind = getattr(self, "kind", None)
        ed = self._elem_data(elemData)
        uu = None if u is None else _f64(u).ravel()
        if kind is None:                       # no mesh on this handle: the library says so
            L.check(L.lib().pfem_post_elements(self._h, _p(ed), _p(uu), None, None, None), "pfem_post_elements")
        assert uu is None or uu.size == self.nNode * L.NDOF[kind]
        ng = L.NG[kind]
        grad = np.empty((ng, self.nElem)); flux = np.empty((ng, self.nElem)); scalar = np.empty(self.nElem)
        L.check(L.lib().pfem_post_elements(self._h, _p(ed), _p(uu), _p(grad), _p(flux), _p(scalar)), "pfem_post_elements")
        return grad, flux, scalar

    def nodalForces(self, elemData, timeData, u=None):
        """``R (nNode, ndof)`` = sum over the elements of ``K_e u_e - F_e`` at every node dof: the applied nodal force at a free dof
        of a converged solution, the reaction at a constrained one (``u`` as in ``elementFields``)."""
        kind = getattr(self, "kind", None)
        ed = self._elem_data(elemData)
        td = None if timeData is None else _f64(timeData)
        uu = None if u is None else _f64(u).ravel()
        if kind is None:
            L.check(L.lib().pfem_post_nodal_forces(self._h, _p(ed), _p(td), _p(uu), _p(np.empty(1))), "pfem_post_nodal_forces")
        assert uu is None or uu.size == self.nNode * L.NDOF[kind]
        R = np.empty((self.nNode, L.NDOF[kind]))
        L.check(L.lib().pfem_post_nodal_forces(self._h, _p(ed), _p(td), _p(uu), _p(R)), "pfem_post_nodal_forces")
        return R

    def nodalRecovery(self, elemData, u=None, field="flux"):
        """``(nodal (nNode, ng), nodal_scalar (nNode,) or None, weight (nNode,))``: the volume-weighted average of the element
        flux / stress (``field="flux"``) or gradient / strain (``"grad"``) at every node, the scalar of the recovered flux
        (``None`` for ``"grad"``) and the sum of the weights (``u`` as in ``elementFields``; ``host.PostScalar`` mirrors the
        scalar)."""
        kind = getattr(self, "kind", None)
        ed = self._elem_data(elemData)
        uu = None if u is None else _f64(u).ravel()
        fld = {"flux": 0, "grad": 1}[field]
        if kind is None:
            L.check(L.lib().pfem_post_nodal_recovery(self._h, _p(ed), _p(uu), fld, None, None, None), "pfem_post_nodal_recovery")
        assert uu is None or uu.size == self.nNode * L.NDOF[kind]
        nodal = np.empty((self.nNode, L.NG[kind])); weight = np.empty(self.nNode)
        scalar = np.empty(self.nNode) if fld == 0 else None
        L.check(L.lib().pfem_post_nodal_recovery(self._h, _p(ed), _p(uu), fld, _p(nodal), _p(scalar), _p(weight)),
                "pfem_post_nodal_recovery")
        return nodal, scalar, weight

    def errorIndicator(self, elemData, u=None):
        """Zienkiewicz-Zhu indicator ``(eta2 (nElem,), eta2_total, flux_norm2_total)``: per element the integral of
        ``|recovered nodal flux - element flux|^2`` (``host.ElementRecoveryError``), and the sums over the mesh."""
        kind = getattr(self, "kind", None)
        ed = self._elem_data(elemData)
        uu = None if u is None else _f64(u).ravel()
        tot = C.c_double(0); fn = C.c_double(0)
        if kind is None:
            L.check(L.lib().pfem_post_error_indicator(self._h, _p(ed), _p(uu), None, C.byref(tot), C.byref(fn)), "pfem_post_error_indicator")
        assert uu is None or uu.size == self.nNode * L.NDOF[kind]
        eta2 = np.empty(self.nElem)
        L.check(L.lib().pfem_post_error_indicator(self._h, _p(ed), _p(uu), _p(eta2), C.byref(tot), C.byref(fn)), "pfem_post_error_indicator")
        return eta2, tot.value, fn.value

    def recoveryTimings(self):
        """Kernel milliseconds of the last ``nodalRecovery`` / ``errorIndicator`` call (the indicator's includes its recovery)."""
        a = C.c_double(0); b = C.c_double(0)
        L.check(L.lib().pfem_post_recovery_timings(self._h, C.byref(a), C.byref(b)), "pfem_post_recovery_timings")
        return {"recovery_ms": a.value, "indicator_ms": b.value}

    def trueResidual(self):
        """``(|b - K x|_2, |b|_2)`` over the owned rows for the x of the last solve (-ksp_monitor_true_residual)."""
        r = C.c_double(0); b = C.c_double(0)
        L.check(L.lib().pfem_solver_true_residual(self._h, C.byref(r), C.byref(b)), "pfem_solver_true_residual")
        return r.value, b.value

    # ---- thermal strains (elasticity kinds, one rank, batched path; include/pfem_amd.h "thermal strains") ------------
    def setThermal(self, alpha, theta):
        """Thermal state of an elastic body: ``theta (nNode,)`` = T - T_ref in the caller's node numbering and the expansion
        coefficient ``alpha`` (a number, or one per material row while a map is set).  Needs the pattern; lives until
        ``clearThermal``, a new mesh or a new pattern.  While it is set ``elementFields``, ``nodalForces``, ``nodalRecovery``
        and ``errorIndicator`` work on the stress ``D (strain - alpha thetabar)``; ``addThermalLoad`` puts the load on the rhs."""
        a = _f64(np.atleast_1d(alpha)).ravel()
        th = _f64(theta).ravel()
        if getattr(self, "kind", None) is not None and th.size != self.nNode:
            raise ValueError(f"theta of {th.size} entries: one per node ({self.nNode}) wanted")
        L.check(L.lib().pfem_thermal_set(self._h, a.size, _p(a), _p(th)), "pfem_thermal_set")

    def setThermalFrom(self, poisson_solver, alpha, T_ref=0.0):
        """The same with ``theta`` = the nodal field of ``poisson_solver``'s last solve minus ``T_ref``, handed over on the device
        (a handle of a one-dof kind with the same nodes IN THE SAME NUMBERING as this one's -- only their count is checked)."""
        a = _f64(np.atleast_1d(alpha)).ravel()
        L.check(L.lib().pfem_thermal_set_from_solver(self._h, a.size, _p(a), poisson_solver._h, float(T_ref)),
                "pfem_thermal_set_from_solver")

    def getThermal(self):
        """``(alpha (n_alpha,), theta (nNode,))`` of the state in effect, theta in the caller's node numbering."""
        n = C.c_int(0)
        L.check(L.lib().pfem_thermal_get(self._h, C.byref(n), None, None), "pfem_thermal_get")
        a = np.empty(n.value); th = np.empty(self.nNode)
        L.check(L.lib().pfem_thermal_get(self._h, C.byref(n), _p(a), _p(th)), "pfem_thermal_get")
        return a, th

    def clearThermal(self):
        L.check(L.lib().pfem_thermal_clear(self._h), "pfem_thermal_clear")

    def addThermalLoad(self, elemData):
        """rhs += the thermal load ``sum_e dvol B^T D eps_th`` of the state in effect at the free dofs; after ``assemble`` (which
        zeroes the rhs), before the solve.  ``elemData`` as ``assemble`` takes it (``host.ThermalLoad`` is the per-element
        mirror)."""
        ed = self._elem_data(elemData)
        L.check(L.lib().pfem_rhs_add_thermal_load(self._h, _p(ed)), "pfem_rhs_add_thermal_load")

    # ---- explicit dynamics (one rank, batched path; include/pfem_amd.h "explicit dynamics") ------------
    def dynamicsSetup(self, elemData, density):
        """Lumped mass on the device from ``density`` (a number, or one per material row while a map is set) and the mesh;
        ``elemData`` as ``assemble`` takes it (the thickness of ``ELAST_TRIA``).  Needs an assembled matrix.  Returns the total
        mass.  The state is at rest at ``t = 0`` afterwards."""
        ed = self._elem_data(elemData)
        dens = _f64(np.atleast_1d(density)).ravel()
        mats = self.materials() if self._h and getattr(self, "kind", None) is not None else None
        want = mats[1] if mats else 1
        if dens.size != want:
            raise ValueError(f"density of {dens.size} entries: {want} wanted (one per material row, or one without a map)")
        tot = C.c_double(0)
        L.check(L.lib().pfem_dynamics_setup(self._h, _p(ed), _p(dens), C.byref(tot)), "pfem_dynamics_setup")
        self._n_probe = 0
        return tot.value

    def dynamicsMass(self):
        """Lumped mass per free dof, in ``getSolution``'s order."""
        m = np.empty(self.size_local)
        L.check(L.lib().pfem_dynamics_get_mass(self._h, _p(m)), "pfem_dynamics_get_mass")
        return m

    def stableDt(self):
        """``2 / sqrt(max_i sum_j |K_ij| / m_i)``: never above the critical step of the central-difference scheme."""
        dt = C.c_double(0)
        L.check(L.lib().pfem_dynamics_stable_dt(self._h, C.byref(dt)), "pfem_dynamics_stable_dt")
        return dt.value

    def setDynamicsState(self, t0=0.0, u0=None, v0=None):
        """``u(t0)``, ``u'(t0)`` per free dof in ``getSolution``'s order (``None``: zeros)."""
        u = None if u0 is None else _f64(u0).ravel()
        v = None if v0 is None else _f64(v0).ravel()
        for a in (u, v):
            if a is not None and a.size != self.size_local:
                raise ValueError("state vectors have one entry per free dof")
        L.check(L.lib().pfem_dynamics_set_state(self._h, float(t0), _p(u), _p(v)), "pfem_dynamics_set_state")

    def setLoadCurve(self, t=None, lam=None):
        """``lambda(t)`` piecewise linear through ``(t[k], lam[k])``, constant outside; no arguments: ``lambda = 1``.  It scales
        the assembled right-hand side as a whole, the Dirichlet lift included."""
        if t is None:
            L.check(L.lib().pfem_dynamics_set_load_curve(self._h, 0, None, None), "pfem_dynamics_set_load_curve")
            return
        tt, ll = _f64(t).ravel(), _f64(lam).ravel()
        if tt.size != ll.size:
            raise ValueError("t and lam differ in length")
        L.check(L.lib().pfem_dynamics_set_load_curve(self._h, tt.size, _p(tt), _p(ll)), "pfem_dynamics_set_load_curve")

    def setProbes(self, global_dof=()):
        """Free dofs (global ids, as ``addNodalForces`` takes them) whose ``u`` and ``v`` go into the history rows."""
        g = np.ascontiguousarray(global_dof, dtype=np.int64).ravel()
        L.check(L.lib().pfem_dynamics_set_probes(self._h, g.size, _p(g)), "pfem_dynamics_set_probes")
        self._n_probe = g.size

    def dynamicsRun(self, dt, n_steps, alpha=0.0, sample_every=0):
        """``n_steps`` central-difference steps with damping ``alpha M``.  Returns the history, ``(n_steps // sample_every,
        4 + 2 n_probe)``: ``[t, T, S, W, u at the probes, v at the probes]`` after every ``sample_every``-th step of this run."""
        rows = C.c_int64(0)
        n_rows = n_steps // sample_every if sample_every > 0 else 0
        hist = np.empty((n_rows, 4 + 2 * getattr(self, "_n_probe", 0)))
        L.check(L.lib().pfem_dynamics_run(self._h, float(dt), int(n_steps), float(alpha), int(sample_every), _p(hist) if n_rows else None,
                                          C.byref(rows)), "pfem_dynamics_run")
        assert rows.value == n_rows
        return hist

    def dynamicsState(self):
        """``(t_n, u_n, v_{n-1/2})`` per free dof in ``getSolution``'s order (before the first run: ``u0``, ``v0`` as set)."""
        t = C.c_double(0); st = C.c_int64(0)
        u = np.empty(self.size_local); v = np.empty(self.size_local)
        L.check(L.lib().pfem_dynamics_get_state(self._h, C.byref(t), C.byref(st), _p(u), _p(v)), "pfem_dynamics_get_state")
        return t.value, u, v

    def benchDynamics(self, dt, graphs=64):
        """Microseconds per explicit step inside ``graphs`` replays of the captured step graph (``pfem_dynamics_bench``)."""
        us = C.c_double(0); per = C.c_int(0)
        L.check(L.lib().pfem_dynamics_bench(self._h, float(dt), int(graphs), C.byref(us), C.byref(per)), "pfem_dynamics_bench")
        return us.value

    def implicitRun(self, dt, n_steps, scheme="newmark", beta=0.25, gamma=0.5, theta=None, alpha=0.0, sample_every=0):
        """``n_steps`` implicit steps on the lumped mass (``pfem_dynamics_run_implicit``): ``scheme="newmark"`` with ``beta``,
        ``gamma`` and damping ``alpha M``, or ``scheme="theta"`` (first order in time; ``theta`` in (0, 1], default 1: backward
        Euler; ``alpha`` must be 0).  Every step is one Jacobi-PCG solve of ``(K + sigma diag(m)) d = b`` from ``d = 0`` with the
        tolerances of ``setTolerances``; the preconditioner is always the point Jacobi of the shifted operator, also when the
        solver's is gamg or node-block Jacobi, which are neither used nor touched.  Returns ``(history, iterations)``: the rows
        ``[t, T, S, W, u at the probes, v at the probes]`` of every ``sample_every``-th step and the CG iterations of every
        step.  ``dynamicsState`` afterwards gives ``(t_n, u_n, v_n)``, v at the integer step.  A step whose solve diverges
        raises ``PfemError`` (``ERR_DIVERGED``) with ``steps_done``, ``history`` and ``iterations`` of the completed steps
        as attributes; the state is that of the last completed step."""
        if scheme == "newmark":
            code, p0, p1 = L.SCHEME_NEWMARK, float(beta), float(gamma)
        elif scheme == "theta":
            code, p0, p1 = L.SCHEME_THETA, 1.0 if theta is None else float(theta), 0.0
        else:
            raise ValueError(f"scheme {scheme!r}: 'newmark' or 'theta'")
        n_steps = int(n_steps)
        rows = C.c_int64(0); done = C.c_int64(0)
        n_rows = n_steps // sample_every if sample_every > 0 and n_steps > 0 else 0
        hist = np.empty((n_rows, 4 + 2 * getattr(self, "_n_probe", 0)))
        its = np.zeros(max(n_steps, 0), np.int32)
        rc = L.lib().pfem_dynamics_run_implicit(self._h, code, float(dt), n_steps, p0, p1, float(alpha), int(sample_every),
                                                _p(hist) if n_rows else None, C.byref(rows), _p(its) if n_steps > 0 else None, C.byref(done))
        if rc == L.ERR_DIVERGED:
            e = L.PfemError(rc, "pfem_dynamics_run_implicit", L.lib().pfem_last_error_string().decode())
            e.steps_done, e.history, e.iterations = done.value, hist[:rows.value], its[:done.value]
            raise e
        L.check(rc, "pfem_dynamics_run_implicit")
        assert rows.value == n_rows and done.value == n_steps
        return hist, its

    def benchImplicit(self, dt, iterations=200, scheme="newmark", beta=0.25, gamma=0.5, theta=1.0):
        """Microseconds per iteration of the shifted CG loop of ``implicitRun``, ``iterations`` of them between two events with
        no convergence exit (``pfem_dynamics_bench_implicit``).  The state does not advance."""
        code, p0, p1 = (L.SCHEME_NEWMARK, beta, gamma) if scheme == "newmark" else (L.SCHEME_THETA, theta, 0.0)
        us = C.c_double(0)
        L.check(L.lib().pfem_dynamics_bench_implicit(self._h, code, float(dt), float(p0), float(p1), int(iterations), C.byref(us)),
                "pfem_dynamics_bench_implicit")
        return us.value

    def modalSolve(self, n_modes, tol=1e-6, max_iterations=1000, block=0, pc=None, x0=None, modes=True):
        """The lowest ``n_modes`` (1..12) modes of ``K phi = omega^2 M phi`` with the lumped mass of ``dynamicsSetup``
        (``pfem_modal_solve``): LOBPCG on a block of 4, 8 or 16 vectors (``block=0``: chosen from ``n_modes``), started from
        ``x0`` (``N x block``, row-major) or from a fixed hash of the dof numbers, so that two runs give the same bits.  The
        preconditioner ``pc``: None takes the solver's -- the cycle of the last gamg solve when ``setPreconditioner("gamg")`` is
        in effect and a solve has run since the last assemble, else the point Jacobi ``1 / K_ii``; ``"jacobi"`` forces the
        point Jacobi, ``"gamg"`` raises ``ERR_STATE`` where the cycle is not current.  The result's ``pc`` names what ran.
        Returns a ``ModalResult``: ``omega`` (rad per time unit, ascending), ``omega2``,
        ``modes`` (``N x n_modes``, ``phi^T M phi = 1``, the largest entry positive; None with ``modes=False``),
        ``residuals`` (``||K phi - omega^2 M phi||`` relative to ``||K phi|| + omega^2 ||M phi||``), ``iterations``,
        ``restarts``, ``reason`` (1 converged, -1 ``max_iterations``, -2 breakdown) and ``block``.  The solve, its
        preconditioner and the steppers' state are left as they are."""
        n_modes = int(n_modes)
        mb = max(int(block), 4 if n_modes <= 2 else 8 if n_modes <= 6 else 16)
        N = self.matrixInfo()["n_owned"]
        k = max(n_modes, 1)
        om2 = np.zeros(k); res = np.zeros(k)
        phi = np.zeros((k, N)) if modes else None
        if x0 is not None:
            x0 = _f64(x0)
            if x0.shape != (N, mb):
                raise ValueError(f"x0 must be {N} x {mb}")
        its = C.c_int(0); restarts = C.c_int(0); reason = C.c_int(0)
        L.check(L.lib().pfem_modal_solve(self._h, n_modes, int(block), float(tol), int(max_iterations), {None: -1, "jacobi": 0, "pbjacobi": 1, "gamg": 2}.get(pc, pc),
                                         _p(x0) if x0 is not None else None, _p(om2), _p(phi) if modes else None, _p(res),
                                         C.byref(its), C.byref(restarts), C.byref(reason)), "pfem_modal_solve")
        used = C.c_int(0)
        L.check(L.lib().pfem_modal_last_pc(self._h, C.byref(used)), "pfem_modal_last_pc")
        return ModalResult(omega=np.sqrt(np.maximum(om2, 0.0)), omega2=om2, modes=np.ascontiguousarray(phi.T) if modes else None,
                           residuals=res, iterations=its.value, restarts=restarts.value, reason=reason.value, block=mb,
                           pc={0: "jacobi", 2: "gamg"}[used.value])

    # ---- linear buckling (pfem_buckling_*; one rank, batched path, the elasticity kinds) ----------------------------------------
    def bucklingSetup(self, elemData, u=None, stress=None):
        """The geometric stiffness ``K_g(sigma_0)`` on the device, on K's pattern (``pfem_buckling_setup``).  ``stress``
        (``(ng, nElem)``, as ``elementFields`` returns ``flux``) prescribes the reference stress; else it is the stress of ``u``
        (``None``: the last solve's field), thermal state included, formed on the device.  ``elemData`` as ``assemble`` takes
        it.  Lives until the next set-up, mesh or ``buildPattern``; a re-assemble of K keeps it."""
        kind = getattr(self, "kind", None)
        ed = self._elem_data(elemData)
        uu = None if u is None else _f64(u).ravel()
        st = None if stress is None else _f64(stress)
        if kind is not None and st is not None and st.shape != (L.NG[kind], self.nElem):
            raise ValueError(f"stress must be {L.NG[kind]} x {self.nElem}")
        assert kind is None or uu is None or uu.size == self.nNode * L.NDOF[kind]
        L.check(L.lib().pfem_buckling_setup(self._h, _p(ed), _p(uu), _p(st)), "pfem_buckling_setup")

    def geometricStiffness(self):
        """``K_g``'s values in ``getCSR``'s layout and order, with its ``rowptr`` and ``cols`` (``pfem_buckling_get_geometric``)."""
        vals = np.empty(self.matrixInfo()["nnz"])
        L.check(L.lib().pfem_buckling_get_geometric(self._h, _p(vals)), "pfem_buckling_get_geometric")
        return vals

    def bucklingSolve(self, n_modes, tol=1e-6, max_iterations=1000, block=0, pc=None, x0=None, modes=True):
        """The lowest ``n_modes`` (1..12) pairs of ``K_g phi = theta K phi`` after ``bucklingSetup`` (``pfem_buckling_solve``):
        the critical load factors of ``(K + lambda K_g) phi = 0`` are ``lambda = -1 / theta`` for ``theta < 0``, ``inf`` for a
        pair that does not buckle in the load's direction.  LOBPCG as ``modalSolve`` runs it, with the same choice of block, start
        and preconditioner ``pc`` (the cycle of the last gamg solve where current, else the point Jacobi of K).  Returns a
        ``BucklingResult``: ``theta`` (ascending), ``factors``, ``modes`` (``N x n_modes``, ``phi^T K phi = 1``, the largest
        entry positive; None with ``modes=False``), ``residuals`` (``||K_g phi - theta K phi||`` relative to
        ``||K_g phi|| + |theta| ||K phi||``), ``iterations``, ``restarts``, ``reason`` (1 converged, -1 ``max_iterations``,
        -2 breakdown), ``block`` and ``pc``.  The solve, the steppers, the modal and the thermal state are left as they are."""
        n_modes = int(n_modes)
        mb = max(int(block), 4 if n_modes <= 2 else 8 if n_modes <= 6 else 16)
        N = self.matrixInfo()["n_owned"]
        k = max(n_modes, 1)
        th = np.zeros(k); fac = np.zeros(k); res = np.zeros(k)
        phi = np.zeros((k, N)) if modes else None
        if x0 is not None:
            x0 = _f64(x0)
            if x0.shape != (N, mb):
                raise ValueError(f"x0 must be {N} x {mb}")
        its = C.c_int(0); restarts = C.c_int(0); reason = C.c_int(0)
        L.check(L.lib().pfem_buckling_solve(self._h, n_modes, int(block), float(tol), int(max_iterations),
                                            {None: -1, "jacobi": 0, "pbjacobi": 1, "gamg": 2}.get(pc, pc), _p(x0) if x0 is not None else None, _p(th), _p(fac),
                                            _p(phi) if modes else None, _p(res), C.byref(its), C.byref(restarts), C.byref(reason)), "pfem_buckling_solve")
        used = C.c_int(0)
        L.check(L.lib().pfem_buckling_last_pc(self._h, C.byref(used)), "pfem_buckling_last_pc")
        return BucklingResult(theta=th, factors=fac, modes=np.ascontiguousarray(phi.T) if modes else None, residuals=res, iterations=its.value,
                              restarts=restarts.value, reason=reason.value, block=mb, pc={0: "jacobi", 2: "gamg"}[used.value])

    def buckProbeGram(self, X, W, P, KX, KW, KP, GX, GW, GP):
        """One launch of ``bucklingSolve``'s Gram kernel and of the sum of its partials on nine ``n x mb`` blocks
        (``pfem_buck_probe_gram``): ``(S^T K_g S, S^T K S)`` from the product blocks, ``3 mb x 3 mb`` each -- the upper block
        triangles, zeros below them."""
        B, n, mb = self._blocks((X, W, P, KX, KW, KP, GX, GW, GP))
        ns = 3 * mb
        out = np.empty((2, ns, ns))
        L.check(L.lib().pfem_buck_probe_gram(self._h, mb, n, *[_p(b) for b in B], _p(out)), "pfem_buck_probe_gram")
        return out[0], out[1]

    def buckProbeResidual(self, GX, KX, theta, dinv=None):
        """One launch of ``bucklingSolve``'s residual kernel and of the sum of its partials (``pfem_buck_probe_residual``):
        ``(W, norms)`` with ``W = dinv o (GX - KX diag(theta))`` (without ``dinv``: the residual itself) and ``norms``
        (``3 x mb``) the squared column norms of the residual, of ``GX`` and of ``KX``."""
        (GX, KX), n, mb = self._blocks((GX, KX))
        theta = _f64(theta)
        dinv = None if dinv is None else _f64(dinv)
        if theta.shape != (mb,) or (dinv is not None and dinv.shape != (n,)):
            raise ValueError(f"dinv must hold {n} doubles, theta {mb}")
        W, norms = np.empty((n, mb)), np.empty((3, mb))
        L.check(L.lib().pfem_buck_probe_residual(self._h, mb, n, _p(GX), _p(KX), _p(dinv), _p(theta), _p(W), _p(norms)), "pfem_buck_probe_residual")
        return W, norms

    def buckProbeUpdate(self, coef, X, W, P, KX, KW, KP, GX, GW, GP):
        """One launch of ``bucklingSolve``'s update kernel with the coefficients ``coef`` (``3 mb x mb``) on copies of the nine
        blocks (``pfem_buck_probe_update``): the nine as the launch left them."""
        B, n, mb = self._blocks((X, W, P, KX, KW, KP, GX, GW, GP))
        coef = _f64(coef)
        if coef.shape != (3 * mb, mb):
            raise ValueError(f"coef must be {3 * mb} x {mb}")
        L.check(L.lib().pfem_buck_probe_update(self._h, mb, n, _p(coef), *[_p(b) for b in B]), "pfem_buck_probe_update")
        return tuple(B)

    def benchBucklingKernels(self, mb, n, reps=20):
        """Microseconds of one launch of ``k_buck_gram`` (with the sum), ``k_buck_update``, ``k_modal_gram`` (with the sum) and
        ``k_modal_update`` on blocks of ``n`` rows (``pfem_buckling_bench_kernels``)."""
        us = np.zeros(4)
        L.check(L.lib().pfem_buckling_bench_kernels(self._h, int(mb), int(n), int(reps), _p(us)), "pfem_buckling_bench_kernels")
        return dict(zip(("buck_gram", "buck_update", "modal_gram", "modal_update"), us))

    def bucklingSetupMs(self):
        ms = C.c_double(0)
        L.check(L.lib().pfem_buckling_setup_ms(self._h, C.byref(ms)), "pfem_buckling_setup_ms")
        return ms.value

    def modalSpmm(self, X):
        """``K X`` for a block ``X`` (``n_local x 4 / 8 / 16``) by the block product of ``modalSolve`` (``pfem_modal_spmm``)."""
        X = _f64(X)
        Y = np.empty_like(X)
        L.check(L.lib().pfem_modal_spmm(self._h, X.shape[1], _p(X), _p(Y)), "pfem_modal_spmm")
        return Y

    @staticmethod
    def _blocks(blocks):
        """contiguous float64 copies of blocks of one shape ``n x mb``, ``mb`` 4, 8 or 16"""
        out = [np.array(b, dtype=np.float64, order="C", ndmin=2) for b in blocks]
        n, mb = out[0].shape
        if mb not in (4, 8, 16) or n < 1 or any(b.shape != (n, mb) for b in out):
            raise ValueError(f"blocks of one shape n x 4 / 8 / 16 with n >= 1, not {[b.shape for b in out]}")
        return out, n, mb

    def modalProbeGram(self, X, W, P, KX, KW, KP, m):
        """One launch of ``modalSolve``'s Gram kernel and of the sum of its partials on the six ``n x mb`` blocks and the ``n``
        masses (``pfem_modal_probe_gram``): ``(G_K, G_M)``, ``3 mb x 3 mb`` each, ``S^T K S`` and ``S^T (m o S)`` for
        ``S = [X W P]`` -- the upper block triangles, zeros below them."""
        B, n, mb = self._blocks((X, W, P, KX, KW, KP))
        m = _f64(m)
        if m.shape != (n,):
            raise ValueError(f"m must hold {n} doubles")
        ns = 3 * mb
        out = np.empty((2, ns, ns))
        L.check(L.lib().pfem_modal_probe_gram(self._h, mb, n, *[_p(b) for b in B], _p(m), _p(out)), "pfem_modal_probe_gram")
        return out[0], out[1]

    def modalProbeResidual(self, KX, X, m, theta, dinv=None):
        """One launch of ``modalSolve``'s residual kernel and of the sum of its partials (``pfem_modal_probe_residual``):
        ``(W, norms)`` with ``W = dinv o (KX - (m o X) diag(theta))`` (without ``dinv``: the residual itself) and ``norms``
        (``3 x mb``) the squared column norms of the residual, of ``KX`` and of ``m o X``."""
        (KX, X), n, mb = self._blocks((KX, X))
        m, theta = _f64(m), _f64(theta)
        dinv = None if dinv is None else _f64(dinv)
        if m.shape != (n,) or theta.shape != (mb,) or (dinv is not None and dinv.shape != (n,)):
            raise ValueError(f"m and dinv must hold {n} doubles, theta {mb}")
        W, norms = np.empty((n, mb)), np.empty((3, mb))
        L.check(L.lib().pfem_modal_probe_residual(self._h, mb, n, _p(KX), _p(X), _p(m), _p(dinv), _p(theta), _p(W), _p(norms)),
                "pfem_modal_probe_residual")
        return W, norms

    def modalProbeUpdate(self, coef, X, W, P, KX, KW, KP):
        """One launch of ``modalSolve``'s update kernel with the coefficients ``coef`` (``3 mb x mb``: rows of X, of W, of P) on
        copies of the six blocks (``pfem_modal_probe_update``): the six as the launch left them -- ``X, P, KX, KP`` updated,
        ``W, KW`` as they stood on the device."""
        B, n, mb = self._blocks((X, W, P, KX, KW, KP))
        coef = _f64(coef)
        if coef.shape != (3 * mb, mb):
            raise ValueError(f"coef must be {3 * mb} x {mb}")
        L.check(L.lib().pfem_modal_probe_update(self._h, mb, n, _p(coef), *[_p(b) for b in B]), "pfem_modal_probe_update")
        return tuple(B)

    # ---- several right-hand sides in one solve (pfem_solver_solve_multi; one rank) ----------------------------------------------
    _PC_CODES = {None: -1, "jacobi": 0, "pbjacobi": 1, "gamg": 2}

    def solveMany(self, B, pc=None):
        """``K x_j = B_j`` for up to 64 right-hand sides on the assembled matrix (``pfem_solver_solve_multi``): every column is
        the CG iteration ``solve`` would run with ``B_j`` as right-hand side -- from ``x = 0``, with the solver's tolerances
        and reasons --, and the columns share one pass over the matrix per iteration, in panels of 4 or 8.  ``B``: ``nrhs x
        N`` (one case per row, ``getRHS()``'s order) or a single vector.  ``pc`` as ``modalSolve``: None takes the solver's
        (the cycle of the last gamg solve where that is current, else the point Jacobi), ``"jacobi"`` forces the point
        Jacobi, ``"gamg"`` raises ``ERR_STATE`` where the cycle is not current.  Returns a ``SolveManyResult``: ``x`` (``nrhs x
        N``), ``iterations``, ``reasons``, ``rnorm`` (arrays of ``nrhs``) and ``pc``, what ran.  A negative reason in some
        column is not an error.  The solve's own solution, right-hand side, history and counters are left as they are."""
        B = np.array(B, dtype=np.float64, order="C", ndmin=2)
        N = self.matrixInfo()["n_owned"]
        if B.ndim != 2 or B.shape[1] != N:
            raise ValueError(f"B must be nrhs x {N} (or one vector of {N}), not {B.shape}")
        nrhs = B.shape[0]
        X = np.zeros((max(nrhs, 1), N))
        its = np.zeros(max(nrhs, 1), dtype=np.int32); why = np.zeros(max(nrhs, 1), dtype=np.int32); rn = np.zeros(max(nrhs, 1))
        L.check(L.lib().pfem_solver_solve_multi(self._h, nrhs, _p(B), self._PC_CODES.get(pc, pc), _p(X), _p(its), _p(why), _p(rn)),
                "pfem_solver_solve_multi")
        used = C.c_int(0)
        L.check(L.lib().pfem_multi_last_pc(self._h, C.byref(used)), "pfem_multi_last_pc")
        return SolveManyResult(x=X, iterations=its, reasons=why, rnorm=rn, pc={0: "jacobi", 2: "gamg"}[used.value])

    def benchSolveMany(self, nrhs, reps=1, pc=None):
        """Device milliseconds of ``reps`` ``solveMany`` runs on the assembled right-hand side scaled by ``j + 1`` and the
        iteration counts of the last (``pfem_multi_bench``): ``(ms[reps], iterations[nrhs])``."""
        ms = np.zeros(reps); its = np.zeros(nrhs, dtype=np.int32)
        L.check(L.lib().pfem_multi_bench(self._h, int(nrhs), int(reps), self._PC_CODES.get(pc, pc), _p(ms), _p(its)), "pfem_multi_bench")
        return ms, its

    # one launch of a kernel of solveMany on panels of the caller's (pfem_multi_probe_*).  The control block travels as a dict
    # of arrays over the mb columns (MCG_FIELDS) with the scalars "running" and "step".
    MCG_BLOCKS = 1024                # blocks of a vector kernel of solveMany at most = rows of partials
    MCG_FOLD = 32                    # rows of folded product partials
    MCG_FIELDS = ("beta", "rn0", "ttol", "rn", "alpha", "bb", "flag", "its", "verdict")

    @staticmethod
    def _mcg_ctl(ctl, mb):
        c = L.McgCtl()
        if ctl is not None:
            for f in PetscSolver.MCG_FIELDS:
                if f in ctl:
                    for j in range(mb):
                        if f == "beta":
                            c.beta[j][0], c.beta[j][1] = float(ctl[f][j][0]), float(ctl[f][j][1])
                        elif f in ("flag", "its", "verdict"):
                            getattr(c, f)[j] = int(ctl[f][j])
                        else:
                            getattr(c, f)[j] = float(ctl[f][j])
            c.running = int(ctl.get("running", 0))
            c.step = int(ctl.get("step", 0))
        return c

    @staticmethod
    def _mcg_dict(c, mb):
        d = {f: np.array([getattr(c, f)[j] for j in range(mb)]) for f in PetscSolver.MCG_FIELDS if f != "beta"}
        d["beta"] = np.array([[c.beta[j][0], c.beta[j][1]] for j in range(mb)])
        d["running"], d["step"] = c.running, c.step
        return d

    @staticmethod
    def _panels(panels):
        out = [np.array(b, dtype=np.float64, order="C", ndmin=2) for b in panels]
        n, mb = out[0].shape
        if mb not in (4, 8) or n < 1 or any(b.shape != (n, mb) for b in out):
            raise ValueError(f"panels of one shape n x 4 / 8 with n >= 1, not {[b.shape for b in out]}")
        return out, n, mb

    def multiProbeInit(self, B, dinv=None):
        """One launch of ``k_mcg_init`` (``pfem_multi_probe_init``): ``(X, R, P, part)``, ``part`` the ``gv x 2 x mb``
        partials of (r,z) and (z,z); without ``dinv`` (the gamg form) ``P`` and ``part`` come back NaN."""
        (B,), n, mb = self._panels((B,))
        dinv = None if dinv is None else _f64(dinv)
        X, R, P = np.empty((n, mb)), np.empty((n, mb)), np.empty((n, mb))
        part = np.empty((self.MCG_BLOCKS, 2, mb)); gv = C.c_int(0)
        L.check(L.lib().pfem_multi_probe_init(self._h, mb, n, _p(B), _p(dinv), _p(X), _p(R), _p(P), _p(part), C.byref(gv)), "pfem_multi_probe_init")
        return X, R, P, part[:gv.value].copy()

    def multiProbeStart(self, part, rtol, abstol):
        """One launch of ``k_mcg_start`` on ``part`` (``nparts x 2 x mb``) (``pfem_multi_probe_start``): the control block."""
        part = _f64(part)
        nparts, _, mb = part.shape
        c = L.McgCtl()
        L.check(L.lib().pfem_multi_probe_start(self._h, mb, nparts, _p(part), float(rtol), float(abstol), C.byref(c)), "pfem_multi_probe_start")
        return self._mcg_dict(c, mb)

    def multiProbeFold(self, part_pw):
        """One launch of ``k_mcg_fold`` on ``part_pw`` (``nb x mb``) (``pfem_multi_probe_fold``): the ``32 x mb`` folded sums."""
        part_pw = _f64(part_pw)
        nb, mb = part_pw.shape
        out = np.empty((self.MCG_FOLD, mb))
        L.check(L.lib().pfem_multi_probe_fold(self._h, mb, nb, _p(part_pw), _p(out)), "pfem_multi_probe_fold")
        return out

    def multiProbeUpdate(self, ctl, fold_pw, W, R, dinv=None):
        """One launch of ``k_mcg_update`` (``pfem_multi_probe_update``): ``(ctl, R, part)``."""
        (W, R), n, mb = self._panels((W, R))
        fold_pw = _f64(fold_pw); dinv = None if dinv is None else _f64(dinv)
        if fold_pw.shape != (self.MCG_FOLD, mb):
            raise ValueError(f"fold_pw must be {self.MCG_FOLD} x {mb}")
        c = self._mcg_ctl(ctl, mb)
        part = np.empty((self.MCG_BLOCKS, 2, mb)); gv = C.c_int(0)
        L.check(L.lib().pfem_multi_probe_update(self._h, mb, n, C.byref(c), _p(fold_pw), _p(W), _p(dinv), _p(R), _p(part), C.byref(gv)),
                "pfem_multi_probe_update")
        return self._mcg_dict(c, mb), R, part[:gv.value].copy()

    def multiProbeDots(self, R, Z, ctl=None, fold_pw=None):
        """One launch of ``k_mcg_dots`` (``pfem_multi_probe_dots``): the ``gv x 2 x mb`` partials."""
        (R, Z), n, mb = self._panels((R, Z))
        fold_pw = None if fold_pw is None else _f64(fold_pw)
        c = None if ctl is None else self._mcg_ctl(ctl, mb)
        part = np.empty((self.MCG_BLOCKS, 2, mb)); gv = C.c_int(0)
        L.check(L.lib().pfem_multi_probe_dots(self._h, mb, n, None if c is None else C.byref(c), _p(fold_pw), _p(R), _p(Z), _p(part), C.byref(gv)),
                "pfem_multi_probe_dots")
        return part[:gv.value].copy()

    def multiProbeVerdict(self, ctl, part, dtol, maxits):
        """One launch of ``k_mcg_verdict`` on ``part`` (``nparts x 2 x mb``) (``pfem_multi_probe_verdict``): the control block."""
        part = _f64(part)
        nparts, _, mb = part.shape
        c = self._mcg_ctl(ctl, mb)
        L.check(L.lib().pfem_multi_probe_verdict(self._h, mb, C.byref(c), nparts, _p(part), float(dtol), int(maxits)), "pfem_multi_probe_verdict")
        return self._mcg_dict(c, mb)

    def multiProbeDirection(self, ctl, R, P, X, dinv=None, Z=None):
        """One launch of ``k_mcg_direction`` (``pfem_multi_probe_direction``): ``(P, X)``; ``Z`` instead of ``dinv``: the gamg form."""
        (R, P, X), n, mb = self._panels((R, P, X))
        dinv = None if dinv is None else _f64(dinv)
        Z = None if Z is None else self._panels((Z,))[0][0]
        c = self._mcg_ctl(ctl, mb)
        L.check(L.lib().pfem_multi_probe_direction(self._h, mb, n, C.byref(c), _p(R), _p(dinv), _p(Z), _p(P), _p(X)), "pfem_multi_probe_direction")
        return P, X

    def multiSpmmDot(self, P):
        """``(K P, pw)`` for a panel ``P`` (``n_local x 4 / 8``) by the product kernel of ``solveMany`` and the fold of its
        partials (``pfem_multi_spmm_dot``): ``pw[j]`` is ``(p_j, K p_j)`` as the update kernel reads it."""
        (P,), n, mb = self._panels((P,))
        W, pw = np.empty_like(P), np.empty(mb)
        L.check(L.lib().pfem_multi_spmm_dot(self._h, mb, _p(P), _p(W), _p(pw)), "pfem_multi_spmm_dot")
        return W, pw

    # ---- one launch of a stepper kernel on vectors of the caller's (pfem_imp_probe_*, pfem_dyn_probe_step) ----------------------
    MAX_GRID = 2048                  # blocks of a stepper's vector kernel at most = partials per sum
    CTL_FIELDS = ("rn0", "ttol", "rn", "dtol", "alpha", "flag", "its", "its_dir")

    @staticmethod
    def _scheme(scheme, beta, gamma, theta):
        if scheme == "newmark":
            return L.SCHEME_NEWMARK, float(beta), float(gamma)
        if scheme == "theta":
            return L.SCHEME_THETA, 1.0 if theta is None else float(theta), 0.0
        raise ValueError(f"scheme {scheme!r}: 'newmark' or 'theta'")

    @staticmethod
    def _vectors(vectors, n=None):
        """contiguous float64 copies of vectors of one length ``n >= 1``"""
        out = [np.array(v, dtype=np.float64, order="C").ravel() for v in vectors]
        n = out[0].size if n is None else n
        if n < 1 or any(v.size != n for v in out):
            raise ValueError(f"vectors of one length n >= 1, not {[v.size for v in out]}")
        return out, n

    @classmethod
    def _ctl_in(cls, ctl):
        c = L.CgCtl()
        c.beta[0], c.beta[1] = (float(b) for b in ctl.get("beta", (0.0, 0.0)))
        for k in cls.CTL_FIELDS:
            setattr(c, k, ctl.get(k, 0))
        return c

    @classmethod
    def _ctl_out(cls, c):
        return {"beta": (c.beta[0], c.beta[1]), **{k: getattr(c, k) for k in cls.CTL_FIELDS}}

    @staticmethod
    def _curve(curve):
        if curve is None:
            return 0, None, None
        ct, cl = (_f64(a).ravel() for a in curve)
        if ct.size != cl.size:
            raise ValueError("t and lam differ in length")
        return ct.size, ct, cl

    def stepperProbePredict(self, dt, u, v, a, beta=0.25, gamma=0.5):
        """One launch of Newmark's predictor (``pfem_imp_probe_predict``): ``(ut, vt)``."""
        (u, v, a), n = self._vectors((u, v, a))
        ut, vt = np.empty(n), np.empty(n)
        L.check(L.lib().pfem_imp_probe_predict(self._h, n, float(dt), float(beta), float(gamma), _p(u), _p(v), _p(a), _p(ut), _p(vt)),
                "pfem_imp_probe_predict")
        return ut, vt

    def stepperProbeRhs(self, dt, f, m, w, dinv, vt=None, scheme="newmark", beta=0.25, gamma=0.5, theta=None, alpha=0.0, curve=None, t_base=0.0,
                        step=0, rtol=1e-5, abstol=1e-50, dtol=1e5):
        """The right-hand side of step ``step`` and the start of its CG (``pfem_imp_probe_rhs``): a dict with ``d, r, p``, the
        partials ``part_rz, part_zz, part_mp`` (2 048 each, NaN behind the first ``gv``), ``gv`` and the control block ``ctl``."""
        code, p0, p1 = self._scheme(scheme, beta, gamma, theta)
        (f, m, w, dinv), n = self._vectors((f, m, w, dinv))
        if vt is not None:
            (vt,), _ = self._vectors((vt,), n)
        nc, ct, cl = self._curve(curve)
        out = {k: np.empty(n) for k in ("d", "r", "p")}
        out.update({k: np.empty(self.MAX_GRID) for k in ("part_rz", "part_zz", "part_mp")})
        gv = C.c_int(0); c = L.CgCtl()
        L.check(L.lib().pfem_imp_probe_rhs(self._h, code, n, float(dt), p0, p1, float(alpha), nc, _p(ct), _p(cl), float(t_base), int(step), float(rtol),
                                           float(abstol), float(dtol), _p(f), _p(m), _p(vt), _p(w), _p(dinv), _p(out["d"]), _p(out["r"]), _p(out["p"]),
                                           _p(out["part_rz"]), _p(out["part_zz"]), _p(out["part_mp"]), C.byref(gv), C.byref(c)), "pfem_imp_probe_rhs")
        out["gv"], out["ctl"] = gv.value, self._ctl_out(c)
        return out

    def stepperProbeUpdate(self, dt, ctl, it_arg, part_pw, part_mp, p, w, m, dinv, r, scheme="newmark", beta=0.25, gamma=0.5, theta=None, alpha=0.0):
        """One launch of the implicit CG's update kernel (``pfem_imp_probe_update``): ``(r, part_rz, part_zz, ctl)``; ``it_arg``
        -1 is the captured graph's form."""
        code, p0, p1 = self._scheme(scheme, beta, gamma, theta)
        (p, w, m, dinv, r), n = self._vectors((p, w, m, dinv, r))
        part_pw, part_mp = _f64(part_pw).ravel(), _f64(part_mp).ravel()
        prz, pzz = np.empty(self.MAX_GRID), np.empty(self.MAX_GRID)
        c = self._ctl_in(ctl)
        L.check(L.lib().pfem_imp_probe_update(self._h, code, n, float(dt), p0, p1, float(alpha), C.byref(c), int(it_arg), part_pw.size, _p(part_pw),
                                              part_mp.size, _p(part_mp), _p(p), _p(w), _p(m), _p(dinv), _p(r), _p(prz), _p(pzz)), "pfem_imp_probe_update")
        return r, prz, pzz, self._ctl_out(c)

    def stepperProbeDirection(self, dt, ctl, it_arg, part_rz, part_zz, r, dinv, m, p, d, maxits, scheme="newmark", beta=0.25, gamma=0.5, theta=None,
                              alpha=0.0):
        """One launch of the implicit CG's direction kernel (``pfem_imp_probe_direction``): ``(p, d, part_mp, ctl)``."""
        code, p0, p1 = self._scheme(scheme, beta, gamma, theta)
        (r, dinv, m, p, d), n = self._vectors((r, dinv, m, p, d))
        part_rz, part_zz = _f64(part_rz).ravel(), _f64(part_zz).ravel()
        if part_rz.size != part_zz.size:
            raise ValueError("part_rz and part_zz differ in length")
        pmp = np.empty(self.MAX_GRID)
        c = self._ctl_in(ctl)
        L.check(L.lib().pfem_imp_probe_direction(self._h, code, n, float(dt), p0, p1, float(alpha), C.byref(c), int(it_arg), part_rz.size, _p(part_rz),
                                                 _p(part_zz), _p(r), _p(dinv), _p(m), _p(p), _p(d), int(maxits), _p(pmp)), "pfem_imp_probe_direction")
        return p, d, pmp, self._ctl_out(c)

    def stepperProbeCorrect(self, dt, d, u=None, ut=None, vt=None, scheme="newmark", beta=0.25, gamma=0.5, theta=None, alpha=0.0):
        """One launch of the corrector (``pfem_imp_probe_correct``): ``(u, v, a)`` -- Newmark from ``ut, vt, d``, the
        theta-method from ``u, d`` (``a`` comes back NaN: the kernel does not write it)."""
        code, p0, p1 = self._scheme(scheme, beta, gamma, theta)
        (d,), n = self._vectors((d,))
        if scheme == "newmark":
            (ut, vt), _ = self._vectors((ut, vt), n)
            u = np.empty(n)
        else:
            (u,), _ = self._vectors((u,), n)
            ut = vt = None
        v, a = np.empty(n), np.empty(n)
        L.check(L.lib().pfem_imp_probe_correct(self._h, code, n, float(dt), p0, p1, float(alpha), _p(ut), _p(vt), _p(d), _p(u), _p(v), _p(a)),
                "pfem_imp_probe_correct")
        return u, v, a

    def stepperProbeEnergy(self, f, m, u, v, w, scheme="newmark", probes=(), t=0.0):
        """The partials of a sampled implicit step and the history row made from them (``pfem_imp_probe_energy``):
        ``(row, part)`` with ``part`` of shape ``3 x gv``."""
        code = self._scheme(scheme, 0.25, 0.5, None)[0]
        (f, m, u, v, w), n = self._vectors((f, m, u, v, w))
        pr = np.ascontiguousarray(probes, dtype=np.int32).ravel()
        row, part = np.empty(4 + 2 * pr.size), np.empty(3 * self.MAX_GRID)
        gv = C.c_int(0)
        L.check(L.lib().pfem_imp_probe_energy(self._h, code, n, _p(f), _p(m), _p(u), _p(v), _p(w), pr.size, _p(pr) if pr.size else None, float(t), _p(row),
                                              _p(part), C.byref(gv)), "pfem_imp_probe_energy")
        return row, part[:3 * gv.value].reshape(3, gv.value).copy()

    def stepperProbeStep(self, dt, f, m, minv, w, u, up, alpha=0.0, t0=0.0, curve=None, step=0, run_start=0, sample_every=0, probes=(), use_ctl=False,
                         ctl_step=(-7, -7)):
        """One launch of the explicit step ``step -> step + 1`` of a run begun at ``run_start`` and, after a sampled step, of the
        kernel that writes its history row (``pfem_dyn_probe_step``): ``(un, row or None, part, ctl_step)`` with ``part`` the
        ``3 x nb`` partials of parity ``step & 1`` (NaN after a step that is not sampled).  ``use_ctl``: the step index comes
        from ``ctl_step[step & 1]``, as in a replayed graph."""
        (f, m, minv, w, u, up), n = self._vectors((f, m, minv, w, u, up))
        nc, ct, cl = self._curve(curve)
        pr = np.ascontiguousarray(probes, dtype=np.int32).ravel()
        un, row, part = np.empty(n), np.empty(4 + 2 * pr.size), np.empty(3 * ((n + 1023) // 1024))
        have, nb = C.c_int(0), C.c_int(0)
        cs = np.array(ctl_step, dtype=np.int64)
        L.check(L.lib().pfem_dyn_probe_step(self._h, n, float(dt), float(alpha), float(t0), nc, _p(ct), _p(cl), int(step), int(run_start), int(sample_every),
                                            pr.size, _p(pr) if pr.size else None, int(bool(use_ctl)), _p(f), _p(m), _p(minv), _p(w), _p(u), _p(up), _p(un),
                                            _p(row), C.byref(have), _p(part), C.byref(nb), _p(cs)), "pfem_dyn_probe_step")
        return un, (row if have.value else None), part.reshape(3, nb.value), (int(cs[0]), int(cs[1]))

    def reordered(self):
        """Whether the mesh on the device is held under the internal renumbering (``pfem_solver_reordered``)."""
        v = C.c_int(0)
        L.check(L.lib().pfem_solver_reordered(self._h, C.byref(v)), "pfem_solver_reordered")
        return bool(v.value)

    def benchModalSpmm(self, mb, reps=50):
        """Microseconds of one block product of ``mb`` vectors and of ``mb`` single products (``pfem_modal_bench_spmm``)."""
        a = C.c_double(0); b = C.c_double(0)
        L.check(L.lib().pfem_modal_bench_spmm(self._h, int(mb), int(reps), C.byref(a), C.byref(b)), "pfem_modal_bench_spmm")
        return a.value, b.value

    def postTimings(self):
        """Kernel milliseconds of the last ``elementFields`` / ``nodalForces`` call (HIP events, host copies excluded)."""
        a = C.c_double(0); b = C.c_double(0)
        L.check(L.lib().pfem_post_timings(self._h, C.byref(a), C.byref(b)), "pfem_post_timings")
        return {"elements_ms": a.value, "nodal_forces_ms": b.value}

    def matrixInfo(self):
        a, b, c, d = (C.c_int64(0) for _ in range(4))
        L.check(L.lib().pfem_matrix_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "pfem_matrix_info")
        return {"n_owned": a.value, "n_local": b.value, "nnz": c.value, "stored": d.value}

    def localToGlobal(self):
        g = np.empty(self.matrixInfo()["n_local"], np.int64)
        L.check(L.lib().pfem_get_local_to_global(self._h, _p(g)), "pfem_get_local_to_global")
        return g

    def getCSR(self, values=True):
        info = self.matrixInfo()
        rowptr = np.empty(info["n_local"] + 1, np.int64)
        cols = np.empty(info["nnz"], np.int32)
        vals = np.empty(info["nnz"]) if values else None
        L.check(L.lib().pfem_get_csr(self._h, _p(rowptr), _p(cols), _p(vals)), "pfem_get_csr")
        return rowptr, cols, vals

    def loadCSR(self, rowptr, cols, vals, values_only=False):
        """A whole CSR matrix through the MatSetValues compat calls, one row per call (pfem_load_csr): the INSERT_VALUES pass that
        records the pattern, setZero, an INSERT_VALUES pass with the values (every bit pattern arrives as given); ``values_only``:
        setZero and the value pass on the standing pattern.  The values are staged on the host like those of MatSetValues: the
        next solve pushes them to the device."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); cols = _i32(cols); vals = _f64(vals)
        if len(rowptr) != self.size_global + 1 or len(cols) != rowptr[-1] or len(vals) != rowptr[-1]:
            raise ValueError("loadCSR: rowptr, cols and vals do not describe one matrix of size_global rows")
        L.check(L.lib().pfem_load_csr(self._h, len(rowptr) - 1, _p(rowptr), _p(cols), _p(vals), int(bool(values_only))), "pfem_load_csr")

    def getRHS(self):
        r = np.empty(self.matrixInfo()["n_local"])
        L.check(L.lib().pfem_get_rhs(self._h, _p(r)), "pfem_get_rhs")
        return r

    def spmv(self, x):
        x = _f64(x)
        y = np.empty_like(x)
        L.check(L.lib().pfem_spmv(self._h, _p(x), _p(y)), "pfem_spmv")
        return y

    def benchSpmv(self, reps=20):
        ms = C.c_double(0)
        L.check(L.lib().pfem_bench_spmv(self._h, reps, C.byref(ms)), "pfem_bench_spmv")
        return ms.value

    def profileSpmv(self, enable=True):
        L.check(L.lib().pfem_solver_profile_spmv(self._h, int(enable)), "pfem_solver_profile_spmv")

    def timings(self):
        t = L.Timings()
        L.check(L.lib().pfem_get_timings(self._h, C.byref(t)), "pfem_get_timings")
        return {k: getattr(t, k) for k, _ in t._fields_}

    # ---- multi-GPU plumbing ----------------------------------------------------------
    def ghosts(self):
        n = C.c_int64(0)
        L.check(L.lib().pfem_get_ghosts(self._h, C.byref(n), None), "pfem_get_ghosts")
        g = np.empty(n.value, np.int64)
        L.check(L.lib().pfem_get_ghosts(self._h, C.byref(n), _p(g)), "pfem_get_ghosts")
        return g

    def setNeighbours(self, peers, peer_off, shared_gid):
        """Install the neighbour plan (``host.neighbour_plan``)."""
        pe = _i32(peers); off = np.ascontiguousarray(peer_off, dtype=np.int64); g = np.ascontiguousarray(shared_gid, dtype=np.int64)
        L.check(L.lib().pfem_solver_set_neighbours(self._h, len(pe), _p(pe), _p(off), _p(g)), "pfem_solver_set_neighbours")

    def setCommRccl(self, rank, nranks, unique_id: bytes):
        """RCCL bound inside the library; ``unique_id`` = the bytes of ``rccl_unique_id()`` from rank 0."""
        assert len(unique_id) == L.RCCL_ID_BYTES
        buf = C.create_string_buffer(bytes(unique_id), L.RCCL_ID_BYTES)
        L.check(L.lib().pfem_solver_set_comm_rccl(self._h, rank, nranks, buf), "pfem_solver_set_comm_rccl")

    def setCommHost(self, rank, nranks, allreduce_cb, exchange_cb):
        """Host-memory hooks (gloo, MPI): ``allreduce_cb(ctx, buf, count)``, ``exchange_cb(ctx, n, peers, off, send, recv)``."""
        a = L.HOST_ALLREDUCE_FN(allreduce_cb) if allreduce_cb is not None else L.HOST_ALLREDUCE_FN()
        e = L.HOST_EXCHANGE_FN(exchange_cb) if exchange_cb is not None else L.HOST_EXCHANGE_FN()
        self._keep.extend([a, e])
        L.check(L.lib().pfem_solver_set_comm_host(self._h, rank, nranks, a, e, None), "pfem_solver_set_comm_host")

    def setCommPeer(self, rank, nranks, allreduce_cb, exchange_cb=None):
        """Peer-memory transport (ranks map each other's receive boxes through hipIpc*; kernels write into them directly): the
        device-side path between processes that share a GPU.  The host hooks carry the bring-up and oversized all-reduces."""
        a = L.HOST_ALLREDUCE_FN(allreduce_cb) if allreduce_cb is not None else L.HOST_ALLREDUCE_FN()
        e = L.HOST_EXCHANGE_FN(exchange_cb) if exchange_cb is not None else L.HOST_EXCHANGE_FN()
        self._keep.extend([a, e])
        L.check(L.lib().pfem_solver_set_comm_peer(self._h, rank, nranks, a, e, None), "pfem_solver_set_comm_peer")

    def commSelftest(self, count=1000):
        """Collective transport check (stamped exchange with every other rank + a known all-reduce): wrong entries."""
        bad = C.c_int64(0)
        L.check(L.lib().pfem_solver_comm_selftest(self._h, count, C.byref(bad)), "pfem_solver_comm_selftest")
        return bad.value

    def commBench(self, count, reps=200, allreduce_count=4, slab_neighbours=False):
        """Collective transport timing: (ms per exchange of ``count`` doubles with every other rank -- ``slab_neighbours``: with rank - 1
        and rank + 1 only --, ms per all-reduce of ``allreduce_count`` doubles)."""
        a, b = C.c_double(0), C.c_double(0)
        L.check(L.lib().pfem_solver_comm_bench_sizes(self._h, count, allreduce_count, reps, 1 if slab_neighbours else 0, C.byref(a), C.byref(b)),
                "pfem_solver_comm_bench_sizes")
        return a.value, b.value

    def commInfo(self):
        npe = C.c_int(0); d = C.c_int64(0); b = C.c_int64(0); t = C.c_int64(0)
        L.check(L.lib().pfem_solver_comm_info(self._h, C.byref(npe), C.byref(d), C.byref(b), C.byref(t)), "pfem_solver_comm_info")
        return {"n_peers": npe.value, "doubles_per_exchange": d.value, "boundary_slices": b.value, "total_slices": t.value}


    def commDescribe(self):
        """What carries the multi-rank solve, as the transport reports it: backend ("rccl" / "host" / "none"), the rank
        count / device / version of the bound RCCL communicators (ncclCommCount, ncclCommCuDevice, ncclGetVersion; -1
        for host hooks), the solver's device, the agreed SpMV form (0 in order, 1 overlapped, -1 not voted yet)."""
        name = C.create_string_buffer(32)
        r, d, v, sd, ov = (C.c_int(0) for _ in range(5))
        L.check(L.lib().pfem_solver_comm_describe(self._h, name, 32, C.byref(r), C.byref(d), C.byref(v), C.byref(sd), C.byref(ov)),
                "pfem_solver_comm_describe")
        return {"backend": name.value.decode(), "backend_ranks": r.value, "backend_device": d.value, "backend_version": v.value,
                "solver_device": sd.value, "overlapped_form": ov.value}


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it and broadcasts the bytes)."""
    buf = C.create_string_buffer(L.RCCL_ID_BYTES)
    L.check(L.lib().pfem_rccl_unique_id(buf), "pfem_rccl_unique_id")
    return buf.raw
