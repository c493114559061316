"""The reference's driver programs on top of the C ABI.

``tetrapoissonparallelimpl1`` / ``tetraelasticityparallelimpl1`` / ``triapoissonserialimpl1``
follow the PROGRAMs of the same name step by step (file:line cited inline): read or take a
mesh, Dirichlet bookkeeping, (re)numbering, ElemDofArray, pattern, element loop, solve,
gather.  Two element-loop modes:

* ``mode="batched"`` (default): the element loop is one device call (``pfem_assemble``).
* ``mode="compat"``: the loop is spelled out exactly like the Fortran -- one
  ``StiffnessResidual*`` call per element, ``MatSetValues`` / ``VecSetValues`` with
  ADD_VALUES, Dirichlet lifting on the host -- and only the solve runs on the GPU.  This
  is what an unchanged Fortran driver does through the Fortran shim.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from . import host as H
from .solver import ADD_VALUES, INSERT_VALUES, PetscSolver


@dataclass
class Result:
    kind: int
    mesh: H.Mesh
    dm: H.DofMap
    solver: PetscSolver
    soln_free: np.ndarray            # solution by free dof (NEW numbering), what temp.dat lists
    solnVTK: np.ndarray              # (nNode, ndof) by OLD node id, Dirichlet values filled in
    its: int
    reason: int
    rnorm: float
    timers: dict = field(default_factory=dict)
    elemData: np.ndarray | None = None   # what the element loop ran with (post-processing of the solution): one vector, or
    elem_mat: np.ndarray | None = None   # -- with a material id per element (the mesh's element order) -- the (n_mat, stride) table

    def temp_dat(self):
        """Rows of the reference's ``temp.dat`` dump (tetrapoissonparallelimpl1.F:935-942):
        (ii, old node id, value), 1-based like the file (ndof=1) ."""
        assy = H.assy_for_soln(self.dm.NodeDofArrayNew)
        ndof = self.dm.NodeDofArrayNew.shape[1]
        if ndof == 1:
            ind = self.dm.node_map_get_old[assy] + 1
        else:   # tetraelasticityparallelimpl1.F:1034-1050
            ind = self.dm.node_map_get_old[assy // ndof] * ndof + assy % ndof + 1
        return np.arange(1, len(assy) + 1), ind, self.soln_free

    def write_outputs(self, directory=".", elem_procid=None, fields=False):
        """The output step of the drivers: ``temp.dat`` (:935-942 / elasticity :1031-1046) and the
        legacy VTK file through the writervtk.F-compatible writer (:944-966).  ``fields=True`` also writes
        ``<name>-fields.vtk``: the same file with the element flux / stress, its scalar and the Zienkiewicz-Zhu indicator
        ``eta = sqrt(eta2)`` as cell arrays and the recovered nodal flux / stress and its scalar as point arrays, by OLD node id
        like ``solnVTK`` (one rank and ``mode="batched"``: the library's PFEM_ERR_STATE otherwise).  A run with several materials
        (``elem_mat``) evaluates them with its table, and the file carries the cell scalar ``material``."""
        import os
        ndof = self.dm.NodeDofArrayNew.shape[1]
        ii, ind, val = self.temp_dat()
        H.write_temp_dat(os.path.join(directory, "temp.dat"), val, *((ii, ind) if ndof == 1 else (None, None)))
        name = "Poisson-soln.vtk" if ndof == 1 else "Elasticity-soln.vtk"
        pid = np.zeros(self.mesh.nElem, np.int32) if elem_procid is None else elem_procid
        H.writeoutputvtk(self.mesh.xyz.shape[0], self.mesh.xyz, self.mesh.conn, pid, self.solnVTK, os.path.join(directory, name),
                         ndof=ndof)
        if fields:
            s, old = self.solver, self.dm.node_map_get_old
            _, flux, scalar = s.elementFields(self.elemData)
            eta2, _, _ = s.errorIndicator(self.elemData)
            nodal, nscalar, _ = s.nodalRecovery(self.elemData)

            def by_old(a):                   # the solver's nodes are the NEW ids: back to the file's, as _finish does
                out = np.empty_like(a)
                out[old] = a
                return out

            f, sc = ("flux", "flux_magnitude") if ndof == 1 else ("stress", "von_mises")
            cells = {f: flux.T, sc: scalar, "eta": np.sqrt(eta2)}
            if self.elem_mat is not None:
                cells["material"] = np.asarray(self.elem_mat, np.float64)
            H.writeoutputvtk_fields(self.mesh.xyz.shape[0], self.mesh.xyz, self.mesh.conn, pid, self.solnVTK,
                                    os.path.join(directory, name[:-4] + "-fields.vtk"), ndof=ndof,
                                    cell_fields=cells,
                                    point_fields={f + "_recovered": by_old(nodal), sc + "_recovered": by_old(nscalar)},
                                    voigt=() if ndof == 1 else (f, f + "_recovered"))
        return os.path.join(directory, name)


def _setup(kind, mesh: H.Mesh, nParts=1, node_proc_id=None):
    ndof = L.NDOF[kind]
    # NodeTypeOld / solnApplied / NodeDofArray*, node maps  (:316-367, :393-679)
    dm = H.dof_numbering(mesh.nNode, ndof, mesh.bc_node, mesh.bc_dof, mesh.bc_val, nParts, node_proc_id)
    conn_new, xyz_new = H.renumber_mesh(mesh, dm)                         # :659-664, :832-838
    edof = H.elem_dof_array(conn_new, dm.NodeDofArrayNew)                # :698-713
    return dm, conn_new, xyz_new, edof


def _finish(kind, mesh, dm, solver, its, reason, rnorm, timers, u_free, elemData=None, elem_mat=None):
    ndof = L.NDOF[kind]
    full = dm.solnApplied.reshape(-1, ndof).copy()                       # :914-918 applied BC values
    assy = H.assy_for_soln(dm.NodeDofArrayNew)                           # :722-734
    full.reshape(-1)[assy] = u_free                                      # :936-941
    solnVTK = np.empty_like(full)
    solnVTK[dm.node_map_get_old] = full
    return Result(kind, mesh, dm, solver, u_free, solnVTK, its, reason, rnorm, timers, elemData, elem_mat)


def _materials(mesh, elemData, elem_mat):
    """``(table, ids)`` of a run with several materials: ``elem_mat[e]`` names the row of the 2-D ``elemData`` that element
    ``e`` of ``mesh.conn`` uses; ``(elemData, None)`` without ``elem_mat``."""
    if elem_mat is None:
        return elemData, None
    if elemData is None:
        raise ValueError("elem_mat needs the elemData table, one row per material")
    table = np.ascontiguousarray(elemData, dtype=np.float64)
    ids = np.ascontiguousarray(elem_mat, dtype=np.int32).ravel()
    if table.ndim != 2:
        raise ValueError("with elem_mat, elemData is a 2-D (n_mat, stride) table")
    if ids.size != mesh.nElem or (ids.size and (ids.min() < 0 or ids.max() >= table.shape[0])):
        raise ValueError("elem_mat: one id in 0 .. n_mat-1 per element of the mesh")
    return table, ids


def _thermal(solver, dm, mesh, thermal, elemData):
    """``thermal=(alpha, theta)`` of the elastic drivers: ``theta (nNode,)`` = T - T_ref by the MESH's node ids, ``alpha`` a number
    or one per material row.  Sets the state on the handle (the solver's nodes are the NEW ids) and adds the load to the rhs."""
    alpha, theta = thermal
    theta = np.asarray(theta, dtype=np.float64).ravel()
    if theta.size != mesh.nNode:
        raise ValueError(f"thermal: theta of {theta.size} entries, one per node ({mesh.nNode}) wanted")
    solver.setThermal(alpha, theta[dm.node_map_get_old])
    solver.addThermalLoad(elemData)


def _run(kind, mesh, elemData, timeData, mode, rtol, maxits, verbose, pc=None, elem_mat=None, surface_loads=None, thermal=None):
    elemData, elem_mat = _materials(mesh, elemData, elem_mat)
    if surface_loads and mode != "batched":
        raise ValueError("surface_loads need mode=\"batched\": the sides are integrated on the device")
    if thermal is not None and mode != "batched":
        raise ValueError("thermal needs mode=\"batched\": the load is integrated on the device")
    dm, conn_new, xyz_new, edof = _setup(kind, mesh)
    N = dm.size_global
    nsize = edof.shape[0]
    ndof = L.NDOF[kind]
    timers = {}
    solver = PetscSolver()
    n1 = min(50, N)                                                      # :762-773 (accepted, unused)
    solver.initialise(N, N, np.full(N, n1, np.int32), np.full(N, min(25, N), np.int32))   # :779
    solver.setTolerances(rtol=rtol, maxits=maxits)
    if pc:                                                               # KSPSetFromOptions: -pc_type (solverpetsc.F:191-206)
        solver.setPreconditioner(pc)
    if mode == "batched":
        solver.uploadMesh(kind, conn_new, xyz_new, edof, dm.solnApplied)
        if elem_mat is not None:                                         # (the renumbering moves nodes, not elements)
            solver.setMaterials(elem_mat, n_mat=elemData.shape[0], stride=elemData.shape[1])
        solver.buildPattern()                                            # :786-802
        t0 = time.perf_counter()                                         # tstart :826
        solver.assemble(elemData, timeData)                              # setZero :817 + loop :828-884
        timers["assembly_s"] = time.perf_counter() - t0                  # :893
    elif mode == "compat":
        Kzero = np.zeros(nsize * nsize)
        for e in range(mesh.nElem):                                      # LoopElem :791-802
            f = edof[:, e]
            solver.MatSetValues(f, f, Kzero, INSERT_VALUES)
        solver.setZero()                                                 # :817
        valC = np.zeros(nsize)
        t0 = time.perf_counter()
        for e in range(mesh.nElem):                                      # :828-884
            nd = conn_new[:, e]
            xN, yN = xyz_new[0, nd], xyz_new[1, nd]
            ed = elemData if elem_mat is None else elemData[elem_mat[e]]  # the element's own row of the table
            if kind == L.POISSON_TET:
                K, F = H.StiffnessResidualPoissonLinearTetra(xN, yN, xyz_new[2, nd], ed, timeData, valC)
            elif kind == L.ELAST_TET:
                K, F = H.StiffnessResidualElasticityLinearTetra(xN, yN, xyz_new[2, nd], ed, timeData, valC)
            elif kind == L.POISSON_TRIA:
                K, F = H.StiffnessResidualPoissonLinearTria(xN, yN, ed, timeData, valC)
            elif kind == L.ELAST_TRIA:
                K, F = H.StiffnessResidualElasticityLinearTria(xN, yN, ed, timeData, valC)
            else:
                raise ValueError("compat mode needs a module element routine")
            f = edof[:, e]
            solver.MatSetValues(f, f, K.ravel(order="F"), ADD_VALUES)    # Fortran memory, read row-major
            for ii in range(nsize):                                      # LoopI/LoopJ :859-870
                if f[ii] == -1:
                    fact = dm.solnApplied[nd[ii // ndof] * ndof + ii % ndof]
                    for jj in range(nsize):
                        if f[jj] != -1:
                            F[jj] = F[jj] - K[jj, ii] * fact
            solver.VecSetValues(f, F, ADD_VALUES)                        # :880
        timers["assembly_s"] = time.perf_counter() - t0
    else:
        raise ValueError(mode)
    if mesh.force_node is not None and ndof > 1:                         # nodal forces :971-982, with the intended
        gdof = dm.NodeDofArrayNew[dm.node_map_get_new[mesh.force_node], mesh.force_dof]   # row = NodeDofArrayNew(n,d)-1
        if mode == "batched":
            solver.addNodalForces(gdof, mesh.force_val)
        else:
            for g, v in zip(gdof, mesh.force_val):
                solver.VecSetValues([g], [v], ADD_VALUES)
    for sl in surface_loads or ():                                       # loads on sides (elem, side) of mesh.conn's elements:
        solver.addSurfaceLoad(sl["elem"], sl["side"], sl["load"], sl["values"], sl.get("layout"), elemData)   # not in the reference
    if thermal is not None:                                              # thermal strains: state on the handle, load on the rhs
        _thermal(solver, dm, mesh, thermal, elemData)
    t0 = time.perf_counter()                                             # :898
    its, reason, rnorm = solver.factoriseAndSolve()                      # :900
    timers["solve_s"] = time.perf_counter() - t0                         # :902
    if verbose:                                                          # solverpetsc.F:481-488
        print("Divergence." if reason < 0 else f" Convergence in {its} iterations.")
    u = solver.getSolution()                                             # VecScatterCreateToAll + VecGetArray :922-932
    timers.update(solver.timings())
    return _finish(kind, mesh, dm, solver, its, reason, rnorm, timers, u, elemData, elem_mat)


def run_parallel(kind, mesh: H.Mesh, elem_proc_id, node_proc_id, dist, torch, elemData=None, timeData=None, rtol=1e-5,
                 maxits=10000, staged=False, device=None, pc=None, spmv=None) -> Result:
    """The parallel branch of the driver PROGRAMs (tetrapoissonparallelimpl1.F:423-679 renumbering from
    (elem_proc_id, node_proc_id), :779 row blocks, :828-884 element loop over ``elem_proc_id == this_mpi_proc``,
    :898-902 solve, :922-932 VecScatterCreateToAll) on an initialised ``torch.distributed`` group, one rank per
    GPU.  ``staged``: ranks share a device and the group reduces host memory (gloo) -- tests only.
    Every rank returns the gathered Result (``soln_free`` is the whole solution, like vec_SEQ)."""
    from . import distributed as PD
    rank, world = dist.get_rank(), dist.get_world_size()
    ndof = L.NDOF[kind]
    if elemData is None:
        elemData = {L.ELAST_TET: H.ELAST_ELEMDATA, L.ELAST_TRIA: H.ELAST2D_ELEMDATA}.get(kind, H.POISSON_ELEMDATA)
    timeData = H.TIMEDATA if timeData is None else timeData
    dm = H.dof_numbering(mesh.nNode, ndof, mesh.bc_node, mesh.bc_dof, mesh.bc_val, world, node_proc_id)
    conn_new, xyz_new = H.renumber_mesh(mesh, dm)                         # :659-664, :832-838
    mine = np.nonzero(np.asarray(elem_proc_id) == rank)[0]                # :829
    conn_loc = np.ascontiguousarray(conn_new[:, mine])
    edof = H.elem_dof_array(conn_loc, dm.NodeDofArrayNew)                # :698-713 for the rank's elements
    rs, re = int(dm.row_start[rank]), int(dm.row_end[rank])
    if device is None:
        device = torch.device("cuda", 0 if staged else rank % max(1, torch.cuda.device_count()))
    solver = PetscSolver().initialise(re - rs, dm.size_global, row_start=rs, device=device.index)   # :779
    solver.setTolerances(rtol=rtol, maxits=maxits)
    if pc:
        solver.setPreconditioner(pc)
    if spmv:
        solver.setSpmvFormat(spmv)
    timers = {}
    solver.uploadMesh(kind, conn_loc, xyz_new, edof, dm.solnApplied)
    hooks = PD.attach(solver, dist, torch, staged=staged)
    solver.buildPattern()                                                # :786-802
    t0 = time.perf_counter()
    solver.assemble(elemData, timeData)                                  # :817-884
    timers["assembly_s"] = time.perf_counter() - t0
    if mesh.force_node is not None and ndof > 1:                         # nodal forces :971-982 (intended row: see _run);
        gdof = dm.NodeDofArrayNew[dm.node_map_get_new[mesh.force_node], mesh.force_dof]   # every rank offers all of them,
        solver.addNodalForces(gdof, mesh.force_val)                      # the library keeps those of the rank's own rows
    t0 = time.perf_counter()
    its, reason, rnorm = solver.factoriseAndSolve()                      # :898-902
    timers["solve_s"] = time.perf_counter() - t0
    if hooks is not None and hooks.error is not None:
        raise hooks.error
    parts = [None] * world                                               # VecScatterCreateToAll (:922-932)
    dist.all_gather_object(parts, (rs, solver.getSolution()))
    u = np.empty(dm.size_global)
    for r0, x in parts:
        u[r0:r0 + len(x)] = x
    timers.update(solver.timings())
    return _finish(kind, mesh, dm, solver, its, reason, rnorm, timers, u, elemData)


@dataclass
class ExplicitResult:
    kind: int
    mesh: H.Mesh
    dm: H.DofMap
    solver: PetscSolver
    t: float                         # time reached
    dt: float
    soln_free: np.ndarray            # u(t) by free dof (NEW numbering)
    velo_free: np.ndarray            # v at t - dt/2
    solnVTK: np.ndarray              # (nNode, ndof) by OLD node id, Dirichlet values filled in
    history: np.ndarray              # rows [t, T, S, W, u at the probes, v at the probes] (PetscSolver.dynamicsRun)
    total_mass: float
    stable_dt: float
    timers: dict = field(default_factory=dict)
    iterations: np.ndarray | None = None   # CG iterations of every implicit step; None for central differences


def _run_explicit(kind, mesh, elemData, density, dt, n_steps, load_curve, alpha, sample_every, probes, u0, v0, elem_mat, surface_loads,
                  check_dt, integrator="central", implicit=None, rtol=1e-5, maxits=10000, thermal=None):
    """The explicit PROGRAMs on one rank: the set-up of ``_run(mode="batched")`` up to the assembled K and load, the lumped
    mass, then the time loop on the device in place of the solve: central differences, or -- ``integrator`` "newmark" /
    "theta" with the keywords of ``PetscSolver.implicitRun`` in ``implicit`` -- implicit steps, to which ``check_dt`` does not
    apply."""
    if integrator not in ("central", "newmark", "theta"):
        raise ValueError(f"integrator {integrator!r}: 'central', 'newmark' or 'theta'")
    elemData, elem_mat = _materials(mesh, elemData, elem_mat)
    dm, conn_new, xyz_new, edof = _setup(kind, mesh)
    N = dm.size_global
    ndof = L.NDOF[kind]
    timers = {}
    solver = PetscSolver()
    solver.initialise(N, N, np.full(N, min(50, N), np.int32), np.full(N, min(25, N), np.int32))
    solver.uploadMesh(kind, conn_new, xyz_new, edof, dm.solnApplied)
    if elem_mat is not None:
        solver.setMaterials(elem_mat, n_mat=elemData.shape[0], stride=elemData.shape[1])
    solver.buildPattern()
    t0 = time.perf_counter()
    solver.assemble(elemData, H.TIMEDATA)
    if mesh.force_node is not None and ndof > 1:
        solver.addNodalForces(dm.NodeDofArrayNew[dm.node_map_get_new[mesh.force_node], mesh.force_dof], mesh.force_val)
    for sl in surface_loads or ():
        solver.addSurfaceLoad(sl["elem"], sl["side"], sl["load"], sl["values"], sl.get("layout"), elemData)
    if thermal is not None:
        _thermal(solver, dm, mesh, thermal, elemData)
    total_mass = solver.dynamicsSetup(elemData, density)                  # MassMatrixLinear* loop (triaelasticityexplicit.F:883-922)
    timers["assembly_s"] = time.perf_counter() - t0
    stable = solver.stableDt()
    if integrator == "central" and check_dt and dt > stable:
        raise ValueError(f"dt = {dt:g} is above the stable step {stable:g} of this mesh and material (pass a smaller dt)")
    if load_curve is not None:
        solver.setLoadCurve(*load_curve)
    if probes is not None:                                               # (node, dof) pairs by the mesh's node ids
        pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
        g = dm.NodeDofArrayNew[dm.node_map_get_new[pr[:, 0]], pr[:, 1]]
        if (g < 0).any():
            raise ValueError("a probe sits on a constrained dof")
        solver.setProbes(g)
    solver.setDynamicsState(0.0, u0, v0)                                  # disp = velo = 0 (:951-953)
    t0 = time.perf_counter()
    its = None
    if integrator == "central":
        hist = solver.dynamicsRun(dt, n_steps, alpha, sample_every)       # the time loop (:970 ff.)
    else:
        solver.setTolerances(rtol=rtol, maxits=maxits)
        hist, its = solver.implicitRun(dt, n_steps, scheme=integrator, alpha=alpha, sample_every=sample_every, **(implicit or {}))
    timers["run_s"] = time.perf_counter() - t0
    t, u, v = solver.dynamicsState()
    r = _finish(kind, mesh, dm, solver, 0, 0, 0.0, timers, u, elemData, elem_mat)
    return ExplicitResult(kind, mesh, dm, solver, t, dt, u, v, r.solnVTK, hist, total_mass, stable, timers, its)


_EXPLICIT_NOTE = """
    The internal force is this library's ``K u`` -- the product of the assembled stiffness, consistent with the pinned
    element matrices and with ``PetscSolver.nodalForces`` -- and the mass is ``MassMatrixLinear*`` lumped (``density`` an
    argument of its own).  The reference's ``Residual*`` routines are NOT reproduced: they differ from the reference's own
    stiffness routines (tensor shear strains against a ``G`` modulus, a plane-strain ``D`` in the triangle, ``dens`` read
    from the thickness slot), so no golden fixture of these PROGRAMs is taken.  ``load_curve=(t, lam)`` scales the whole
    assembled load (the Dirichlet lift included); ``alpha`` is mass-proportional damping; ``probes`` are ``(node, dof)``
    pairs; ``history`` has a row every ``sample_every`` steps.  ``dt`` above ``PetscSolver.stableDt()`` is a ``ValueError``
    unless ``check_dt=False``.  One rank, ``mode="batched"`` only.  ``thermal=(alpha, theta)`` adds the thermal load of
    ``theta`` = T - T_ref per mesh node to the assembled load (scaled by the load curve with the rest) and leaves the state on the
    handle for the post-processing calls.

    ``integrator="central"`` (the default) is the PROGRAM's scheme.  ``integrator="newmark"`` takes the same steps with Newmark
    (``beta``, ``gamma``; ``PetscSolver.implicitRun``): unconditionally stable for ``gamma >= 1/2``, ``beta >= (gamma + 1/2)^2 / 4``,
    so ``check_dt`` does not apply and the PROGRAM's own ``dt`` runs; every step is a Jacobi-PCG solve to ``rtol`` within
    ``maxits`` iterations, ``iterations`` of the result holds their counts (``None`` for central differences) and ``velo_free``
    is then v at ``t``, not at ``t - dt/2``."""


def tetraelasticityexplicit(mesh: H.Mesh | str, dt=0.01, n_steps=100, elemData=None, density=7800.0, load_curve=None, alpha=0.0,
                            sample_every=0, probes=None, u0=None, v0=None, elem_mat=None, surface_loads=None,
                            check_dt=True, integrator="central", beta=0.25, gamma=0.5,
                            rtol=1e-5, maxits=10000, thermal=None) -> ExplicitResult:
    """PROGRAM of tetraelasticityexplicit.F on one rank: central differences on a lumped mass, E = 207e9, nu = 0.3, density
    7800, no body force, dt = 0.01 and stepsMax = 100 steps as the PROGRAM sets them (:910-934: its loop runs while
    ``stepsCompleted < stepsMax .OR. timeNow < 10 dt``; its dt is far above the stable step of any steel mesh of metre size:
    give your own)."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    ed = np.array([207.0e9, H._f32(0.3), 1.0, 0.0, 0.0, 0.0]) if elemData is None else elemData
    return _run_explicit(L.ELAST_TET, mesh, ed, density, dt, n_steps, load_curve, alpha, sample_every, probes, u0, v0, elem_mat,
                         surface_loads, check_dt, integrator, {"beta": beta, "gamma": gamma} if integrator == "newmark" else None, rtol, maxits,
                         thermal)


def triaelasticityexplicit(mesh: H.Mesh | str, dt=0.0002, n_steps=50000, elemData=None, density=10.0, load_curve="reference", alpha=0.0,
                           sample_every=0, probes=None, u0=None, v0=None, elem_mat=None, surface_loads=None,
                           check_dt=True, integrator="central", beta=0.25, gamma=0.5,
                           rtol=1e-5, maxits=10000, thermal=None) -> ExplicitResult:
    """PROGRAM of triaelasticityexplicit.F on one rank: E = 200, nu = 0.3, density 10, unit thickness, body force (1, 0) while
    t <= 0.1 (:872-876, :974-977), dt = 2e-4, 50 000 steps (:958-962).  ``load_curve="reference"`` is that switch as a curve:
    lambda = 1 up to t = 0.1, 0 from the next step on."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    ed = np.array([200.0, H._f32(0.3), 1.0, 1.0, 0.0]) if elemData is None else elemData
    if isinstance(load_curve, str):
        if load_curve != "reference":
            raise ValueError(load_curve)
        load_curve = ([0.1, 0.1 + 0.5 * dt], [1.0, 0.0])
    return _run_explicit(L.ELAST_TRIA, mesh, ed, density, dt, n_steps, load_curve, alpha, sample_every, probes, u0, v0, elem_mat,
                         surface_loads, check_dt, integrator, {"beta": beta, "gamma": gamma} if integrator == "newmark" else None, rtol, maxits,
                         thermal)


tetraelasticityexplicit.__doc__ += _EXPLICIT_NOTE
triaelasticityexplicit.__doc__ += _EXPLICIT_NOTE


def poissontransient(mesh: H.Mesh | str, dt, n_steps, theta=1.0, capacity=1.0, u0=None, elemData=None, load_curve=None, sample_every=0,
                     probes=None, elem_mat=None, surface_loads=None, rtol=1e-5, maxits=10000) -> ExplicitResult:
    """Transient heat conduction ``capacity u' + K u = lambda(t) f`` on a triangle or tet Poisson mesh by the theta-method
    (``PetscSolver.implicitRun(scheme="theta")``; ``theta = 1`` backward Euler, ``1/2`` Crank-Nicolson) on the lumped capacity:
    K and f are those of ``triapoissonparallelimpl1`` / ``tetrapoissonparallelimpl1`` (the Dirichlet lift in f), ``capacity`` is
    rho c -- a number, or one per material row with ``elem_mat`` --, ``u0`` the initial field by free dof (zeros).  Not part of
    the reference, which has no diffusion stepper.  ``elem_mat`` / ``surface_loads`` / ``probes`` / ``load_curve`` /
    ``sample_every`` as the explicit drivers take them; every step is a Jacobi-PCG solve to ``rtol``.  Returns an
    ``ExplicitResult``: ``velo_free`` is ``(u_n - u_{n-1}) / dt``, the T column of ``history`` is ``1/2 sum m u^2``."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    npe = mesh.conn.shape[0]
    if npe not in (3, 4):
        raise ValueError("poissontransient takes triangle and tet meshes")
    kind = L.POISSON_TET if npe == 4 else L.POISSON_TRIA
    ed = (H.POISSON_ELEMDATA if npe == 4 else np.array([1.0, 1.0])) if elemData is None else elemData
    return _run_explicit(kind, mesh, ed, capacity, dt, n_steps, load_curve, 0.0, sample_every, probes, u0, None, elem_mat, surface_loads,
                         False, "theta", {"theta": theta}, rtol, maxits)


def tetrapoissonparallelimpl1(mesh: H.Mesh | str, mode="batched", rtol=1e-5, maxits=10000, verbose=False, pc=None, elem_mat=None,
                              elemData=None, surface_loads=None) -> Result:
    """PROGRAM TetraMeshPoissonEquation (tetrapoissonparallelimpl1.F) on one rank / one GPU.  ``elemData``: another vector than
    the PROGRAM's, or -- with ``elem_mat``, one material id per element -- the ``(n_mat, stride)`` table of a body of several
    materials (all five drivers; not part of the reference, whose drivers hard-code one material).  ``surface_loads``: a list of
    dicts ``{"elem", "side", "load", "values"[, "layout"]}`` handed to ``PetscSolver.addSurfaceLoad`` after the nodal forces (all
    five drivers, ``mode="batched"`` only: ``ValueError`` with ``"compat"``; sides as ``PetscSolver.boundaryFaces`` names them,
    elements in the order of ``mesh.conn``)."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    ed = H.POISSON_ELEMDATA if elemData is None else elemData
    return _run(L.POISSON_TET, mesh, ed, H.TIMEDATA, mode, rtol, maxits, verbose, pc, elem_mat, surface_loads)   # :822-824


def tetraelasticityparallelimpl1(mesh: H.Mesh | str, mode="batched", rtol=1e-5, maxits=10000, verbose=False, pc=None, elem_mat=None,
                                 elemData=None, surface_loads=None, thermal=None) -> Result:
    """PROGRAM of tetraelasticityparallelimpl1.F (body force only; DESIGN.md 'deviations').  ``thermal=(alpha, theta)`` (both
    elastic drivers; not part of the reference): ``theta (nNode,)`` = T - T_ref by the mesh's node ids and the expansion
    coefficient (one per material row with ``elem_mat``), handed to ``PetscSolver.setThermal`` / ``addThermalLoad`` after the
    surface loads; the state stays on the handle, so ``write_outputs(fields=True)`` and the post-processing calls of the result's
    solver give the stress ``D (strain - alpha thetabar)``."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    ed = H.ELAST_ELEMDATA if elemData is None else elemData
    return _run(L.ELAST_TET, mesh, ed, H.TIMEDATA, mode, rtol, maxits, verbose, pc, elem_mat, surface_loads, thermal)       # :894-902


def triapoissonserialimpl1(mesh: H.Mesh | str, rtol=1e-5, maxits=10000, verbose=False, pc=None, elem_mat=None, elemData=None,
                           surface_loads=None) -> Result:
    """PROGRAM of triapoissonserialimpl1.F: inline Ke = area*B*B^T (:573-594), Laplace.  The inline element has no material:
    ``elem_mat`` (with its table) is the library's PFEM_ERR_ARG, ``elemData`` without it is ignored."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    return _run(L.POISSON_TRIA_INLINE, mesh, elemData if elem_mat is not None else None, H.TIMEDATA, "batched", rtol, maxits, verbose, pc,
                elem_mat, surface_loads)


def triapoissonparallelimpl1(mesh: H.Mesh | str, mode="batched", rtol=1e-5, maxits=10000, verbose=False, pc=None, elem_mat=None,
                             elemData=None, surface_loads=None) -> Result:
    """PROGRAM of triapoissonparallelimpl1.F on one rank: the module routine
    StiffnessResidualPoissonLinearTria (:862), kx = ky = 1, no source (next row 8f.1)."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    ed = np.array([1.0, 1.0]) if elemData is None else elemData
    return _run(L.POISSON_TRIA, mesh, ed, H.TIMEDATA, mode, rtol, maxits, verbose, pc, elem_mat, surface_loads)


def triaelasticityparallelimpl1(mesh: H.Mesh | str, mode="batched", rtol=1e-5, maxits=10000, verbose=False, pc=None, elem_mat=None,
                                elemData=None, surface_loads=None, thermal=None) -> Result:
    """PROGRAM of triaelasticityparallelimpl1.F on one rank with its intended semantics (the committed
    driver USEs a module that does not exist and reads thick/bforce uninitialised: SURVEY A.3#7, 8f.1):
    plane stress, E = 240.565, nu = 0.3 (REAL(4) literals), unit thickness, nodal forces from ForceBC."""
    if isinstance(mesh, str):
        mesh = H.read_mesh(mesh)
    ed = H.ELAST2D_ELEMDATA if elemData is None else elemData
    return _run(L.ELAST_TRIA, mesh, ed, H.TIMEDATA, mode, rtol, maxits, verbose, pc, elem_mat, surface_loads, thermal)
