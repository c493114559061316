"""The N>1 path: one process per rank, 127.0.0.1 rendezvous.

CPU (gloo, world_size 2 and 3): pins the product's host logic of the sub-assembled layout -- slab / irregular
partition, reference renumbering, ghost detection, the NEIGHBOUR PLAN (pfem_neighbour_plan) and the host hooks
(exchange = isend/irecv per neighbour, all-reduce = reduce + broadcast) -- by summing each rank's sub-assembled
diagonal and right-hand side (oracle, this rank's elements only) over the plan and comparing with the serially
assembled global ones.  No restatement of the CG loop lives here: the device loop is tested on the GPU, below.

GPU: 2-3 ranks share cuda:0; the library stages its packed buffers through pinned host memory and the hooks move
them with gloo (what the MPI flavour does with MPI): the real C++/HIP multi-rank loop (SpMV -> neighbour exchange ->
rank-ordered sums -> two scalar all-reduces; in order, and in its overlapped form with boundary slices first)
against the ORACLE's direct solve and iteration count.  RCCL itself refuses two ranks on one device: it is exercised with world_size 1
(communicator, all-reduce, grouped send/recv to self, a solve whose scalars go through ncclAllReduce).
"""
import os
import socket

import numpy as np
import pytest


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _partition(mesh, world, how, H):
    """(elem_proc_id, node_proc_id): z-slabs, or an irregular METIS-like one -- elements by the
    angular sector of their centroid, every node given to a pseudo-random part among those of the
    elements touching it (so interface nodes are shared by up to `world` ranks and the owned row
    blocks interleave in space).  Deterministic: every rank computes the same arrays."""
    if how == "slabs":
        return H.partition_box_slabs(*mesh.box, world)
    if how in ("xslabs", "yslabs"):    # slabs of hex layers across x / y: the renumbering is no longer the identity
        return H.partition_box_slabs(*mesh.box, world, axis="xyz".index(how[0]))
    if how == "rcb":                   # the build's own geometric partitioner (pfem_partition_rcb)
        return H.partition_rcb(mesh, world)
    if how == "stairs":
        # z-slabs whose border planes step up by one layer of cells halfway along x: no rank's dofs fill a box of the lattice
        # (what a METIS partition of a structured mesh looks like locally), yet almost every 2x2x2 brick has one owner
        nz = mesh.box[2]
        x0, x1, z0, z1 = mesh.xyz[0].min(), mesh.xyz[0].max(), mesh.xyz[2].min(), mesh.xyz[2].max()

        def part_of(xyz):
            step = (xyz[0] > 0.5 * (x0 + x1) + 1e-9).astype(np.float64)
            layer = np.floor((xyz[2] - z0) / (z1 - z0) * nz - 1e-9) - step
            return np.clip(np.floor(layer * world / nz), 0, world - 1).astype(np.int32)
        return part_of(mesh.xyz[:, mesh.conn].mean(axis=1)), part_of(mesh.xyz)
    if how == "idle":                  # the last rank gets nothing: no elements, no nodes, no rows
        return H.partition_box_slabs(*mesh.box, world - 1)
    if how == "foreign":               # slabs, but some nodes deep inside slab 0 are OWNED by the last rank, which has no
        epid, npid = H.partition_box_slabs(*mesh.box, world)         # element touching them: owned rows with an empty
        inner = np.nonzero(npid == 0)[0]                             # local pattern, ghosts on the rank that assembles them
        npid = npid.copy()
        npid[inner[len(inner) // 3::17]] = world - 1
        return epid, npid
    cen = mesh.xyz[:, mesh.conn].mean(axis=1)
    ang = np.arctan2(cen[1] - cen[1].mean() + 0.013, cen[0] - cen[0].mean() + 0.007)
    epid = np.minimum(((ang + np.pi) / (2 * np.pi) * world).astype(np.int32), world - 1)
    touch = np.zeros((world, mesh.nNode), bool)
    for a in range(mesh.conn.shape[0]):
        touch[epid, mesh.conn[a]] = True
    rng = np.random.default_rng(12345)
    pick = rng.random((world, mesh.nNode)) * touch
    return epid, pick.argmax(axis=0).astype(np.int32)


def _mesh_args(kind_name, partition):
    a = ({"box": (-1, 1, 6, -1, 1, 5, -1, 1, 7), "bc_mode": 0, "ndof": 1} if kind_name == "poisson" else
         {"box": (-0.5, 0.5, 2, 0.0, 3.0, 6, -0.5, 0.5, 4), "bc_mode": 1, "ndof": 3})
    a["partition"] = partition
    return a


def _rank_setup(rank, world, mesh_args, H):
    """Everything a rank does before the element loop (bench.py does the same)."""
    mesh = H.gen_box_tets(*mesh_args["box"], bc_mode=mesh_args["bc_mode"], ndof=mesh_args["ndof"])
    epid, npid = _partition(mesh, world, mesh_args.get("partition", "slabs"), H)
    ndof = mesh_args["ndof"]
    dm = H.dof_numbering(mesh.nNode, ndof, mesh.bc_node, mesh.bc_dof, mesh.bc_val, world, npid)
    conn_new, xyz_new = H.renumber_mesh(mesh, dm)                         # :659-664, :832-838
    mine = np.nonzero(epid == rank)[0]                       # elem_proc_id(ee)==this_mpi_proc (:829)
    conn_loc = np.ascontiguousarray(conn_new[:, mine])
    edof_loc = H.elem_dof_array(conn_loc, dm.NodeDofArrayNew)
    rs, re = int(dm.row_start[rank]), int(dm.row_end[rank])
    return mesh, dm, conn_loc, xyz_new, edof_loc, rs, re


# ---------------------------------------------------------------------------------------
def _cpu_worker(rank, world, port, kind_name, mesh_args, out_dir):
    import ctypes as C
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import pfem_oracle as O
        from pfemfort_amd import distributed as PD
        from pfemfort_amd import host as H
        kind = O.POISSON_TET if kind_name == "poisson" else O.ELAST_TET
        mesh, dm, conn_loc, xyz_new, edof_g, rs, re = _rank_setup(rank, world, mesh_args, H)
        n_owned = re - rs
        ghosts = H.find_ghosts(edof_g, rs, n_owned)
        lists = PD.gather_ghost_lists(ghosts, dist)
        ranges = [None] * world
        dist.all_gather_object(ranges, (rs, re))
        peers, off, gid = H.neighbour_plan(rank, ranges, lists)
        # local numbering exactly as the device does it (k_localize_dofs): owned first, ghosts after
        n_loc = n_owned + len(ghosts)
        e = edof_g.astype(np.int64)
        loc = np.where((e >= rs) & (e < re), e - rs, n_owned + np.searchsorted(ghosts, e))
        edof_l = np.where(e < 0, -1, loc).astype(np.int32)
        lidx = np.where((gid >= rs) & (gid < re), gid - rs, n_owned + np.searchsorted(ghosts, gid))
        # this rank's sub-assembled operator and rhs from the oracle (own elements only)
        ed = O.ELAST_ELEMDATA if kind == O.ELAST_TET else O.POISSON_ELEMDATA
        rowptr, cols = O.csr_pattern(edof_l, n_loc)
        vals, rhs = O.assemble(kind, xyz_new, conn_loc, edof_l, dm.solnApplied, ed, n_loc, rowptr, cols)
        diag = np.array([vals[rowptr[i]:rowptr[i + 1]][cols[rowptr[i]:rowptr[i + 1]] == i].sum() for i in range(n_loc)])

        hooks = PD.HostHooks(dist, torch)
        hooks.log = []
        pp = (C.c_int * max(len(peers), 1))(*peers)
        oo = (C.c_int64 * (len(peers) + 1))(*off)

        def exchange_sum(v):
            """what the library does around the hook: pack, exchange, add in ascending rank order"""
            send = np.ascontiguousarray(v[lidx])
            recv = np.full_like(send, np.nan)
            assert hooks.exchange(None, len(peers), pp, oo, send.ctypes.data_as(C.POINTER(C.c_double)),
                                  recv.ctypes.data_as(C.POINTER(C.c_double))) == 0
            out = v.copy()
            for l in np.unique(lidx):
                terms = [(rank, v[l])] + [(int(peers[k]), recv[i]) for k in range(len(peers))
                                          for i in range(off[k], off[k + 1]) if lidx[i] == l]
                acc = 0.0
                for _, t in sorted(terms):
                    acc += t
                out[l] = acc
            return out

        # the plan is symmetric: what peer q receives from us is our list for q, and vice versa
        send = gid.astype(np.float64)
        recv = np.full_like(send, -1.0)
        assert hooks.exchange(None, len(peers), pp, oo, send.ctypes.data_as(C.POINTER(C.c_double)),
                              recv.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert np.array_equal(send, recv)
        red = np.array([1.0, rank + 1.0])
        assert hooks.allreduce(None, red.ctypes.data_as(C.POINTER(C.c_double)), 2) == 0
        assert hooks.error is None, hooks.error
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), diag=exchange_sum(diag)[:n_owned], rhs=exchange_sum(rhs)[:n_owned],
                 rs=rs, re=re, peers=peers, n_send=len(gid), red=red, calls=hooks.calls,
                 ghost_sum_ok=np.isfinite(exchange_sum(diag)).all())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind_name,world,partition", [("poisson", 2, "slabs"), ("elast", 2, "slabs"),
                                                       ("poisson", 3, "sectors"), ("elast", 3, "sectors"),
                                                       ("poisson", 3, "rcb")])
def test_gloo_neighbour_plan_sums_subassembled_rows(tmp_path, kind_name, world, partition):
    import torch.multiprocessing as mp
    from oracle import pfem_oracle as O
    from pfemfort_amd import host as H
    kind = O.POISSON_TET if kind_name == "poisson" else O.ELAST_TET
    mesh_args = _mesh_args(kind_name, partition)
    mp.spawn(_cpu_worker, args=(world, _free_port(), kind_name, mesh_args, str(tmp_path)), nprocs=world, join=True)
    # serial truth: oracle assembly of the SAME (renumbered) global problem
    mesh = H.gen_box_tets(*mesh_args["box"], bc_mode=mesh_args["bc_mode"], ndof=mesh_args["ndof"])
    _, npid = _partition(mesh, world, partition, H)
    prob = O.setup_problem(kind, O.Mesh(mesh.xyz, mesh.conn, mesh.bc_node, mesh.bc_dof, mesh.bc_val), nParts=world,
                           node_proc_id=npid)
    N = prob.dm.size_global
    diag = np.array([prob.vals[prob.rowptr[i]:prob.rowptr[i + 1]][prob.cols[prob.rowptr[i]:prob.rowptr[i + 1]] == i].sum()
                     for i in range(N)])
    tot = 0
    for r in range(world):
        d = np.load(tmp_path / f"rank{r}.npz")
        rs, re = int(d["rs"]), int(d["re"])
        tot += re - rs
        assert np.abs(d["diag"] - diag[rs:re]).max() <= 1e-13 * np.abs(diag).max()
        assert np.abs(d["rhs"] - prob.rhs[rs:re]).max() <= 1e-13 * max(1.0, np.abs(prob.rhs).max())
        assert len(d["peers"]) >= 1 and int(d["n_send"]) > 0 and bool(d["ghost_sum_ok"])
        assert np.array_equal(d["red"], [world, world * (world + 1) / 2])
    assert tot == N


def _id_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pfemfort_amd as pf
        from pfemfort_amd import distributed as PD

        def broken():                  # only ever called on rank 0
            raise pf.PfemError(9, "pfem_rccl_unique_id", "injected: librccl.so.1 could not be loaded")
        seen = None
        try:
            PD.broadcast_rccl_id(dist, make_id=broken)
        except pf.PfemError as e:
            seen = str(e)
        # the very next collective must still line up on every rank (bench.py's vote)
        votes = [None] * world
        dist.all_gather_object(votes, seen)
        ok = PD.broadcast_rccl_id(dist, make_id=lambda: b"x" * 256)      # and a healthy rank 0 reaches everybody
        np.savez(os.path.join(out_dir, f"id{rank}.npz"), seen=str(seen), votes=np.array([str(v) for v in votes]), ok=len(ok))
    finally:
        dist.destroy_process_group()


def test_rccl_id_failure_on_rank0_alone_reaches_every_rank(tmp_path):
    """Round-2 advisory: the unique id is created on rank 0 only; if that fails there, rank 0 used to leave the
    broadcast the others were waiting in and the job hung.  Now a (status, id) pair is always broadcast: every rank
    raises the same error, and the next collective (the fallback vote of bench.py) lines up."""
    import torch.multiprocessing as mp
    mp.spawn(_id_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        d = np.load(tmp_path / f"id{r}.npz")
        assert "injected" in str(d["seen"]) and "rank 0" in str(d["seen"])
        assert all("injected" in v for v in d["votes"]) and int(d["ok"]) == 256


def test_neighbour_plan_small_example():
    from pfemfort_amd import host as H
    # rank0 owns [0,5), rank1 [5,9), rank2 [9,12); ghosts are what each touches but does not own
    lists = [np.array([5, 6]), np.array([3, 4, 9]), np.array([6, 8])]
    ranges = [(0, 5), (5, 9), (9, 12)]
    local = [set(range(a, b)) | set(g.tolist()) for (a, b), g in zip(ranges, lists)]
    plans = [H.neighbour_plan(r, ranges, lists) for r in range(3)]
    for r, (peers, off, gid) in enumerate(plans):
        assert peers.tolist() == [q for q in range(3) if q != r and local[r] & local[q]]
        for k, q in enumerate(peers):
            assert gid[off[k]:off[k + 1]].tolist() == sorted(local[r] & local[q])
    assert plans[1][0].tolist() == [0, 2] and plans[1][2].tolist() == [3, 4, 5, 6, 6, 8, 9]
    # a rank that shares nothing has no peers; malformed input is refused
    peers, off, gid = H.neighbour_plan(0, [(0, 4), (4, 8)], [np.empty(0, np.int64), np.empty(0, np.int64)])
    assert len(peers) == 0 and off.tolist() == [0] and len(gid) == 0
    import pfemfort_amd as pf
    with pytest.raises(pf.PfemError):
        H.neighbour_plan(0, [(0, 4), (4, 8)], [np.array([6, 5]), np.empty(0, np.int64)])        # not ascending


# ---------------------------------------------------------------------------------------
def _gpu_worker(rank, world, port, mesh_args, out_dir):
    import faulthandler
    faulthandler.dump_traceback_later(240, exit=True)     # a stuck rank reports where and exits non-zero
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pfemfort_amd as pf
        from pfemfort_amd import distributed as PD
        from pfemfort_amd import host as H
        kind = pf.POISSON_TET if mesh_args["ndof"] == 1 else pf.ELAST_TET
        if mesh_args.get("overlap"):        # the overlapped form of the iteration (boundary slices, second stream)
            os.environ["PFEM_MULTI_OVERLAP"] = "1"
        if mesh_args.get("amg_block"):      # -pc_type gamg as block Jacobi over the ranks even where one hierarchy across them is possible
            os.environ["PFEM_AMG_COUPLED"] = "0"
        if mesh_args.get("amg_distributed"):    # every level of the coupled hierarchy spread over the ranks (test meshes are small enough
            os.environ["PFEM_AMG_REPLICATE_ROWS"] = "0"      # for every rank to hold level 1 whole, which is what happens by default)
        if mesh_args.get("reorder"):        # the owned dofs renumbered inside the library (the plan is translated)
            os.environ["PFEM_REORDER"] = "1"
        devgen = mesh_args.get("mode") == "devgen"     # the rank's slab generated on the device (bench.py's path), any axis
        if devgen:
            b = mesh_args["box"]
            cells = (b[2], b[5], b[8])
            axis = "xyz".index(mesh_args["partition"][0]) if mesh_args["partition"] in ("xslabs", "yslabs") else 2
            sz = H.box_slab_sizes(*cells, mesh_args["bc_mode"], mesh_args["ndof"], world, rank, axis=axis)
            rs, re = sz["row_start"], sz["row_start"] + sz["size_local"]
            s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"], row_start=rs, device=0)
        else:
            mesh, dm, conn_loc, xyz_new, edof_g, rs, re = _rank_setup(rank, world, mesh_args, H)
            s = pf.PetscSolver().initialise(re - rs, dm.size_global, row_start=rs, device=0)
        s.setTolerances(rtol=1e-10)
        if mesh_args.get("pc"):
            s.setPreconditioner(mesh_args["pc"])
        s.setSpmvFormat(mesh_args.get("spmv", "auto"))
        if mesh_args.get("single"):         # KSPCGUseSingleReduction: one all-reduce (of three scalars) per iteration
            s.setSingleReduction(True)
        ed = H.ELAST_ELEMDATA if kind == pf.ELAST_TET else H.POISSON_ELEMDATA
        if devgen:
            s.generateBoxMesh(kind, *mesh_args["box"], bc_mode=mesh_args["bc_mode"], nparts=world, part=rank, axis=axis)
            hooks = PD.attach(s, dist, torch, staged=True, peer=bool(mesh_args.get("peer")))
            s.buildPattern()
            s.assemble(ed, H.TIMEDATA)
        elif mesh_args.get("mode", "batched") == "batched":
            s.uploadMesh(kind, conn_loc, xyz_new, edof_g, dm.solnApplied)
            hooks = PD.attach(s, dist, torch, staged=True, peer=bool(mesh_args.get("peer")))
            s.buildPattern()
            s.assemble(ed, H.TIMEDATA)
        else:
            # the Fortran driver's own loops (tetrapoissonparallelimpl1.F:786-884) with GLOBAL indices: pattern by
            # INSERT_VALUES, setZero, then per-element routine + lifting + ADD_VALUES for this rank's elements
            from pfemfort_amd.solver import ADD_VALUES, INSERT_VALUES
            ndof, nsize = mesh_args["ndof"], edof_g.shape[0]
            for e in range(conn_loc.shape[1]):
                s.MatSetValues(edof_g[:, e], edof_g[:, e], np.zeros(nsize * nsize), INSERT_VALUES)
            s.setZero()
            hooks = PD.attach(s, dist, torch, staged=True, peer=bool(mesh_args.get("peer")))
            fn = H.StiffnessResidualElasticityLinearTetra if kind == pf.ELAST_TET else H.StiffnessResidualPoissonLinearTetra
            for e in range(conn_loc.shape[1]):
                nd = conn_loc[:, e]
                K, F = fn(xyz_new[0, nd], xyz_new[1, nd], xyz_new[2, nd], ed, H.TIMEDATA, np.zeros(nsize))
                f = edof_g[:, e]
                s.MatSetValues(f, f, K.ravel(order="F"), ADD_VALUES)
                for ii in np.nonzero(f == -1)[0]:
                    fact = dm.solnApplied[nd[ii // ndof] * ndof + ii % ndof]
                    F = F - np.where(f != -1, K[:, ii] * fact, 0.0)
                s.VecSetValues(f, F, ADD_VALUES)
        assert s.commSelftest(257) == 0
        hooks.log = []
        its, reason, rn = s.factoriseAndSolve()
        x1 = s.getSolution()
        assert hooks.error is None, hooks.error
        extra = {}
        if mesh_args.get("resolve"):
            # a second solve after more right-hand side arrives through VecSetValues, without setZero (compat path):
            # the freshly staged sub-assembled rhs must be summed over the interface again
            from pfemfort_amd.solver import ADD_VALUES
            own = np.arange(rs, re, dtype=np.int32)
            s.VecSetValues(own, 0.25 * np.ones(len(own)), ADD_VALUES)
            its2, reason2, _ = s.factoriseAndSolve()
            extra = {"x2": s.getSolution(), "its2": its2, "reason2": reason2}
        if mesh_args.get("pc") == "gamg":
            # the rank's own hierarchy, for the oracle's restatement: its owned diagonal block as assembled here, its aggregates
            if mesh_args.get("mode", "batched") in ("batched", "devgen"):
                # the same values assembled again, solved again: aggregates, plans and merge maps are reused, every number is redone
                # (Galerkin sums, the replicated level's values through the all-reduce, bounds, bottom inverse) -- and comes out the same
                s.assemble(ed, H.TIMEDATA)
                its_b, reason_b, _ = s.factoriseAndSolve()
                assert (its_b, reason_b) == (its, reason) and np.array_equal(s.getSolution(), x1)
            ai = s.amgInfo()
            lay = s.amgLayout()
            extra.update(amg_coupled=int(lay["coupled"]), amg_distributed=lay["distributed_levels"], amg_exchanges=lay["exchanges_per_cycle"],
                         amg_allreduces=lay["allreduces_per_cycle"], amg_first=np.array(lay["first_dof"]), amg_lam=np.array(ai["lambda_max"]),
                         amg_local_rows=np.array(lay["local_rows"]))
            rp, cc, vv = s.getCSR()
            no = re - rs
            keep = np.zeros(len(cc), bool)
            for i in range(no):
                keep[rp[i]:rp[i + 1]] = cc[rp[i]:rp[i + 1]] < no
            brp = np.concatenate([[0], np.cumsum([keep[rp[i]:rp[i + 1]].sum() for i in range(no)])]).astype(np.int64)
            extra.update(blk_rowptr=brp, blk_cols=cc[:rp[no]][keep[:rp[no]]], blk_vals=vv[:rp[no]][keep[:rp[no]]], amg_levels=ai["levels"],
                         amg_rows=np.array(ai["rows"]), amg_opts=np.array([ai["cheb_degree"], ai["eig_ratio"], ai["coarse_scale"], ai["fine_degree"]]),
                         **{f"agg{l}": s.amgAggregates(l, ai["rows"][l]) for l in range(ai["levels"] - 1)},
                         # rigid-body modes: [rbm, dofs per node, dofs per coarse node, dimension] of every transfer
                         amg_kinds=np.array(s.amgAggregation()),
                         amg_transfer=np.array([[int(t["rbm"]), t["fine_bs"], t["coarse_bs"], t["dim"]]
                                                for t in (s.amgTransfer(l) for l in range(ai["levels"] - 1))]).reshape(-1, 4))
        info = s.commInfo()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), x=x1, rs=rs, re=re, its=its, reason=reason,
                 pc=s.preconditioner(), calls=hooks.calls, log=np.array([f"{k}{c}" for k, c in hooks.log]), transport=s.commDescribe()["backend"],
                 n_peers=info["n_peers"], n_send=info["doubles_per_exchange"], slices_b=info["boundary_slices"],
                 slices=info["total_slices"], **extra)
        s.free()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("kind_name,world,partition,mode", [("poisson", 2, "slabs", "batched"), ("elast", 2, "slabs", "batched"),
                                                            ("poisson", 3, "sectors", "batched"), ("elast", 3, "sectors", "batched"),
                                                            ("poisson", 2, "slabs", "compat"), ("elast", 3, "sectors", "compat"),
                                                            ("elast", 2, "slabs", "pbjacobi"), ("elast", 3, "sectors", "pbjacobi"),
                                                            ("poisson", 2, "slabs", "pbjacobi"), ("poisson", 3, "sectors", "int32"),
                                                            ("poisson", 3, "idle", "batched"), ("elast", 3, "idle", "pbjacobi"),
                                                            ("poisson", 2, "slabs", "overlap"), ("elast", 3, "sectors", "overlap"),
                                                            ("poisson", 2, "foreign", "batched"), ("elast", 3, "foreign", "compat"),
                                                            ("poisson", 3, "rcb", "batched"), ("elast", 3, "rcb", "overlap"),
                                                            ("poisson", 2, "slabs", "single"), ("elast", 3, "sectors", "single"),
                                                            ("poisson", 3, "rcb", "single_overlap"), ("elast", 3, "idle", "single"),
                                                            ("poisson", 3, "yslabs", "batched"), ("elast", 3, "yslabs", "devgen"),
                                                            ("poisson", 2, "xslabs", "devgen"), ("poisson", 3, "slabs", "devgen"),
                                                            ("elast", 2, "xslabs", "batched"),
                                                            ("poisson", 2, "slabs", "gamg"), ("poisson", 3, "rcb", "gamg"),
                                                            ("elast", 3, "yslabs", "gamg"), ("poisson", 3, "idle", "gamg_overlap"),
                                                            ("poisson", 2, "slabs", "gamg_block"), ("elast", 3, "yslabs", "gamg_block"),
                                                            ("poisson", 3, "xslabs", "gamg"), ("elast", 2, "slabs", "gamg_overlap"),
                                                            ("poisson", 2, "slabs", "gamg_distributed"), ("elast", 3, "yslabs", "gamg_distributed"),
                                                            ("poisson", 3, "idle", "gamg_distributed"), ("poisson", 3, "rcb", "gamg_distributed"),
                                                            ("elast", 3, "sectors", "gamg"), ("elast", 3, "rcb", "gamg_distributed"),
                                                            ("poisson", 3, "foreign", "gamg"), ("poisson", 5, "sectors", "gamg_distributed"),
                                                            ("elast", 4, "rcb", "gamg"), ("poisson", 5, "rcb", "gamg"),
                                                            ("poisson", 3, "sectors", "reorder"), ("elast", 2, "slabs", "reorder_gamg"),
                                                            ("poisson", 2, "slabs", "gamg_single"), ("elast", 3, "yslabs", "gamg_single"),
                                                            ("poisson", 3, "stairs", "gamg"), ("poisson", 3, "stairs", "gamg_distributed"),
                                                            ("elast", 3, "yslabs", "gamg_cubic"), ("elast", 2, "xslabs", "gamg_cubic"),
                                                            ("elast", 4, "rcb", "gamg_cubic_distributed")])
def test_gpu_ranks_on_one_device_match_oracle(tmp_path, kind_name, world, partition, mode, peer=False):
    """2-3 ranks share cuda:0 (host-staged exchange over gloo): the product's multi-rank device loop against the
    ORACLE -- a direct solve of the oracle-assembled global system in the partition's new numbering, and the oracle's
    Jacobi-PCG iteration count.  ``peer``: the same over the peer-memory transport (see test_gpu_peer_memory_transport)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import torch.multiprocessing as mp
    from oracle import pfem_oracle as O
    from pfemfort_amd import host as H
    mesh_args = ({"box": (-1, 1, 12, -1, 1, 10, -1, 1, 14), "bc_mode": 0, "ndof": 1} if kind_name == "poisson" else
                 {"box": (-0.5, 0.5, 3, 0.0, 3.0, 8, -0.5, 0.5, 6), "bc_mode": 1, "ndof": 3})
    mesh_args["partition"] = partition
    mesh_args["mode"] = mode
    mesh_args["peer"] = peer
    if mode in ("reorder", "reorder_gamg"):     # internal Morton renumbering forced on: neighbour plan, solution, CSR in the caller's numbering
        mesh_args["reorder"] = True
        mode = "gamg" if mode == "reorder_gamg" else "batched"
        mesh_args["mode"] = mode
    if mode == "gamg_single":          # the hierarchy across the ranks inside the single-reduction form of the loop: 2 all-reduces per iteration
        mesh_args["single"] = True
        mode = "gamg"
    if mode in ("gamg_cubic", "gamg_cubic_distributed"):
        # cubic cells: every coupling inside a brick is strong, so the displacement problem takes its NODE bricks in one step across
        # the ranks (the default beam's cells are 1.5 x longer along y: the check refuses them and the pairing passes keep the level)
        mesh_args["box"], mesh_args["cubic"] = (-0.5, 0.5, 6, 0.0, 4.0, 24, -0.5, 0.5, 6), True
        mode = "gamg" if mode == "gamg_cubic" else "gamg_distributed"
    if mode in ("gamg", "gamg_overlap", "gamg_block", "gamg_distributed"):
        # -pc_type gamg on several ranks: one hierarchy across the ranks where the partition allows it (slabs: every coarse dof
        # has at most two holders), else -- or when asked, "gamg_block" -- block Jacobi over the ranks, every block its own hierarchy
        mesh_args["mode"], mesh_args["pc"], mesh_args["overlap"] = ("devgen" if partition in ("yslabs", "xslabs") else "batched"), "gamg", mode == "gamg_overlap"
        mesh_args["amg_block"] = mode == "gamg_block"
        mesh_args["amg_distributed"] = mode == "gamg_distributed"     # no replicated levels: every level keeps its neighbour plan, global dense bottom
        if kind_name == "elast" and partition == "yslabs" and mode == "gamg" and not mesh_args.get("cubic"):
            # a longer beam: its level 1 (3 dofs per aggregate) is above the dense limit and gets replicated, nodes and all
            mesh_args["box"], mesh_args["long_beam"] = (-0.5, 0.5, 6, 0.0, 6.0, 24, -0.5, 0.5, 6), True
    if mode == "devgen":              # bench.py's path: every rank generates its slab (along the partition's axis) on the device
        mesh_args["mode"] = "devgen"
    if world == 3 or mode != "batched":   # the row-group SpMV forms ("auto" keeps systems this small in the row form)
        mesh_args["spmv"] = "grouped"
    if mode == "pbjacobi":            # node-block Jacobi on several ranks (blocks of shared nodes summed, groups voted)
        mesh_args["mode"], mesh_args["pc"] = "batched", "pbjacobi"
    if mode == "overlap":             # boundary slices first, exchange on the second stream under the interior slices
        mesh_args["mode"], mesh_args["overlap"] = "batched", True
    if mode in ("single", "single_overlap"):      # the single-reduction form of the iteration, in order / overlapped
        mesh_args["mode"], mesh_args["single"], mesh_args["overlap"] = "batched", True, mode == "single_overlap"
    if mode == "int32":               # the int32-column SpMV form through the boundary / interior slice lists
        mesh_args["mode"], mesh_args["spmv"] = "batched", "int32"
    if mode == "compat":
        mesh_args["resolve"] = True
        if kind_name == "poisson":
            mesh_args["box"] = (-1, 1, 6, -1, 1, 5, -1, 1, 7)
    mp.spawn(_gpu_worker, args=(world, _free_port(), mesh_args, str(tmp_path)), nprocs=world, join=True)
    mesh = H.gen_box_tets(*mesh_args["box"], bc_mode=mesh_args["bc_mode"], ndof=mesh_args["ndof"])
    kind = O.POISSON_TET if kind_name == "poisson" else O.ELAST_TET
    _, npid = _partition(mesh, world, partition, H)
    prob = O.setup_problem(kind, O.Mesh(mesh.xyz, mesh.conn, mesh.bc_node, mesh.bc_dof, mesh.bc_val), nParts=world,
                           node_proc_id=npid)
    lu = spl.splu(sp.csr_matrix((prob.vals, prob.cols, prob.rowptr)).tocsc())
    u = lu.solve(prob.rhs)
    single = bool(mesh_args.get("single"))
    _, its_oracle, reason_oracle, *_ = (O.pcg_jacobi_single_reduction if single else O.pcg_jacobi)(
        prob.rowptr, prob.cols, prob.vals, prob.rhs, rtol=1e-10)
    assert reason_oracle == 2
    its_tol = 3
    if mesh_args.get("pc") == "gamg":
        # the oracle's restatement of the block preconditioner (every rank's V-cycle on its own block, its own aggregates)
        blocks = []
        for r in range(world):
            d = np.load(tmp_path / f"rank{r}.npz")
            assert str(d["pc"]) == "gamg"
            aggs = [d[f"agg{l}"] for l in range(int(d["amg_levels"]) - 1)]
            blocks.append((int(d["rs"]), (d["blk_rowptr"], d["blk_cols"], d["blk_vals"]), aggs))
            deg, ratio, scale, fdeg = np.load(tmp_path / "rank0.npz")["amg_opts"]
        its_jacobi = its_oracle
        d0 = np.load(tmp_path / "rank0.npz")
        coupled = bool(int(d0["amg_coupled"]))
        ds = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
        assert all(bool(int(d["amg_coupled"])) == coupled for d in ds)
        assert coupled == (not mesh_args["amg_block"])       # (any partition: dofs and aggregates with three holders too -- "rcb")
        if coupled:
            # ONE hierarchy across the ranks: the oracle's restatement of the cycle on the assembled GLOBAL matrix with the
            # global aggregates the ranks formed (a rank's piece of level l starts at its first dof of that level)
            nl, nd = int(d0["amg_levels"]), int(d0["amg_distributed"])
            assert all(int(d["amg_levels"]) == nl and int(d["amg_distributed"]) == nd for d in ds)
            # (test meshes: level 1 is small enough to be replicated -- the little beam's is even below the dense limit, where
            # the global dense inverse takes over and nothing is left to replicate; the longer beam's is not)
            print(f"gamg levels {kind_name} x{world} {partition} {mode}: {nl} levels, {nd} distributed, owned rows per level "
                  f"{[[int(d['amg_rows'][l]) for d in ds] for l in range(nl)]}")
            assert (nd == nl) if mesh_args["amg_distributed"] else (1 <= nd <= nl)
            aggs, rows_glob = [], []
            for l in range(nl):          # distributed levels: the ranks' owned rows add up; replicated levels: every rank holds all rows
                rows_glob.append(sum(int(d["amg_rows"][l]) for d in ds) if l < nd else int(d0["amg_rows"][l]))
                assert l < nd or all(int(d["amg_rows"][l]) == rows_glob[l] for d in ds)
            for l in range(nl - 1):
                if l < nd:
                    a = np.full(rows_glob[l], -1, np.int64)
                    for d in ds:
                        f = int(d["amg_first"][l])
                        a[f:f + int(d["amg_rows"][l])] = d[f"agg{l}"]
                else:                    # the replicated part of the hierarchy is the same on every rank
                    a = d0[f"agg{l}"].astype(np.int64)
                    assert all(np.array_equal(d[f"agg{l}"], a) for d in ds)
                tr = d0["amg_transfer"][l]
                assert all(np.array_equal(d["amg_transfer"], d0["amg_transfer"]) for d in ds)
                if tr[0]:
                    # rigid-body modes: the oracle's OWN prolongator from the global node aggregates (the device reports the
                    # translation part of P) and the node coordinates -- the mesh's free nodes in the partition's numbering on
                    # level 0, below it the centroids the oracle computed itself
                    fb, cb, dim = int(tr[1]), int(tr[2]), int(tr[3])
                    a2 = a.reshape(-1, fb)
                    assert not (a2[:, 0] % cb).any() and all(np.array_equal(a2[:, c], a2[:, 0] + c) for c in range(fb))
                    if l == 0:
                        nda = prob.dm.NodeDofArrayNew.reshape(-1, fb)
                        free = np.where(nda[:, 0] >= 0)[0]
                        assert np.array_equal(nda[free, 0], fb * np.arange(len(free)))
                        cen = np.zeros((3, len(free)))
                        cen[:prob.xyz_new.shape[0]] = prob.xyz_new[:, free]
                    P, cen = O.rbm_prolongator(a2[:, 0] // cb, cen, dim, fb)
                    assert P.shape[1] == rows_glob[l + 1]
                    aggs.append(P)
                    continue
                assert a.min() >= 0 and a.max() == rows_glob[l + 1] - 1 and len(np.unique(a)) == rows_glob[l + 1]
                aggs.append(a)
            if kind_name == "poisson":
                # bricks in one step ACROSS the ranks: the oracle forms the aggregates itself, from the coordinates and the dofs'
                # owners alone (global positions, the planes between the ranks padded onto brick borders, every rank numbering its
                # own bricks; the replicated levels plain bricks of those positions), and the device's equal them entry for entry --
                # wherever every rank's dofs fill a box of the lattice; elsewhere (sectors, foreign) the pairing passes keep the level
                nda = prob.dm.NodeDofArrayNew.reshape(-1)
                free = np.where(nda >= 0)[0]
                assert np.array_equal(nda[free], np.arange(len(free)))
                owner = np.zeros(len(free), np.int64)
                for r in range(world):
                    owner[int(prob.dm.row_start[r]):int(prob.dm.row_end[r])] = r
                own_aggs = O.lattice_brick_aggregates(prob.xyz_new, prob.xyz_new[:, free], owner=owner,
                                                      replicate_rows=0 if mesh_args["amg_distributed"] else 150000)
                assert (own_aggs is not None) == (partition in ("slabs", "xslabs", "yslabs", "rcb", "idle")), partition
                if own_aggs is None:
                    # ranks whose dofs do not fill boxes (round 6): the bricks are split between their owners -- the oracle restates
                    # those aggregates too (owner x brick); the device takes them where every rank's check of its own rows passes and
                    # the level shrinks (the stairs always; sectors / foreign scatter single dofs and keep the pairing passes)
                    own_split = O.lattice_brick_aggregates(prob.xyz_new, prob.xyz_new[:, free], owner=owner, split=True,
                                                           replicate_rows=0 if mesh_args["amg_distributed"] else 150000)
                    kinds = [str(k) for k in d0["amg_kinds"]]
                    taken = kinds[0] == "split-bricks"
                    if partition == "stairs":
                        assert taken and own_split is not None, (kinds, rows_glob)
                    if taken:
                        own_aggs = own_split
                        print(f"split bricks across ranks: {kind_name} x{world} {partition} {mode}, rows per level {rows_glob}")
                    if partition == "stairs":
                        # ... and the hierarchy is as good as the one-rank bricks of the same mesh: iterations within +2 of the
                        # oracle's own solve with ITS one-rank bricks, nearly the same rows on the first coarse level
                        one = O.lattice_brick_aggregates(prob.xyz_new, prob.xyz_new[:, free])
                        _, its_one, reason_one, *_ = O.pcg_amg(prob.rowptr, prob.cols, prob.vals, prob.rhs, one, rtol=1e-10, cheb_degree=int(deg),
                                                               eig_ratio=float(ratio), coarse_scale=float(scale), fine_degree=int(fdeg))
                        assert reason_one == 2 and int(d0["its"]) <= its_one + 2, (int(d0["its"]), its_one)
                        assert rows_glob[1] <= 1.1 * (int(one[0].max()) + 1)
                if own_aggs is not None:
                    kinds = [str(k) for k in d0["amg_kinds"]]
                    n_cmp = len(aggs)
                    if kinds[0] != "split-bricks":
                        assert len(own_aggs) == len(aggs), ([len(np.unique(x)) for x in own_aggs], rows_glob, kinds)
                    else:
                        # (split bricks: the owners' slivers of a brick that the border cuts couple weakly to their siblings on the coarser
                        # levels, whose check may hand them to the pairing passes: the levels formed as bricks are compared)
                        n_cmp = next((l for l, k in enumerate(kinds) if k not in ("bricks", "split-bricks")), len(kinds))
                        assert n_cmp >= 1 and len(own_aggs) >= n_cmp
                    for lv, (x, y) in enumerate(zip(own_aggs[:n_cmp], aggs[:n_cmp])):
                        bad = np.nonzero(x != y)[0]
                        assert not len(bad), (f"level {lv}: {len(bad)} of {len(x)} aggregates differ, first at dof {bad[0]}: oracle {x[bad[:12]].tolist()} "
                                              f"device {y[bad[:12]].tolist()}; rows {rows_glob}")
                    print(f"bricks across ranks == the oracle's own: {kind_name} x{world} {partition} {mode}, rows per level {rows_glob}")
            if kind_name == "elast" and not mesh_args.get("reorder"):
                # node bricks in one step ACROSS the ranks (round 6): where every rank's nodes fill a box of the lattice the oracle
                # forms the node aggregates itself, from the coordinates and the nodes' owners alone (bricks cut where the owner
                # changes, every rank numbering the bricks of its own box; the replicated levels plain node bricks again), and the
                # device's equal them entry for entry; elsewhere (sectors, foreign) the pairing passes keep the levels
                nda = prob.dm.NodeDofArrayNew.reshape(-1, 3)
                free = np.where(nda[:, 0] >= 0)[0]
                owner = np.zeros(len(free), np.int64)
                for r in range(world):
                    owner[int(prob.dm.row_start[r]) // 3:int(prob.dm.row_end[r]) // 3] = r
                own_nodes = O.lattice_node_brick_aggregates(prob.xyz_new, prob.xyz_new[:, free], owner=owner,
                                                            replicate_rows=0 if mesh_args["amg_distributed"] else 150000)
                if partition in ("slabs", "xslabs", "yslabs", "idle"):
                    assert own_nodes is not None
                if partition in ("sectors", "foreign"):
                    assert own_nodes is None
                # (cells that are not cubic: the device's check of the couplings inside a brick may refuse the bricks -- the passes
                # keep the level then, with other aggregates; the cases with cubic cells must take them)
                kinds = [str(k) for k in d0["amg_kinds"]]
                assert all([str(k) for k in d["amg_kinds"]] == kinds for d in ds)
                if mesh_args.get("cubic"):
                    assert own_nodes is not None and kinds[0] == "node-bricks", kinds
                if own_nodes is not None and kinds[0] == "node-bricks":
                    tr_all = d0["amg_transfer"]
                    dev_nodes = []
                    for l in range(nl - 1):
                        if not tr_all[l][0] or kinds[l] != "node-bricks":
                            break
                        fb, cb = int(tr_all[l][1]), int(tr_all[l][2])
                        if l < nd:
                            a = np.full(rows_glob[l], -1, np.int64)
                            for d in ds:
                                f = int(d["amg_first"][l])
                                a[f:f + int(d["amg_rows"][l])] = d[f"agg{l}"]
                        else:
                            a = d0[f"agg{l}"].astype(np.int64)
                        dev_nodes.append(a.reshape(-1, fb)[:, 0] // cb)
                    assert len(own_nodes) >= len(dev_nodes) >= 1, ([len(np.unique(x)) for x in own_nodes], rows_glob, kinds)
                    if mesh_args.get("cubic"):
                        assert len(own_nodes) == len(dev_nodes), ([len(np.unique(x)) for x in own_nodes], rows_glob, kinds)
                    for lv, (x, y) in enumerate(zip(own_nodes, dev_nodes)):
                        bad = np.nonzero(x != y)[0]
                        assert not len(bad), (f"level {lv}: {len(bad)} of {len(x)} node aggregates differ, first at node {bad[0]}: oracle "
                                              f"{x[bad[:12]].tolist()} device {y[bad[:12]].tolist()}; rows {rows_glob}")
                    print(f"node bricks across ranks == the oracle's own: x{world} {partition} {mode}, rows per level {rows_glob}")
            # the last level takes the dense inverse, or the coarsening stalled just above its limit (Chebyshev bottom)
            assert rows_glob[0] == len(prob.rhs) and rows_glob[-1] <= 256
            if not mesh_args["amg_distributed"]:
                # replication starts at the first level of at most 150000 rows over all ranks -- on these meshes level 1 -- unless
                # that level is already small enough for the dense inverse of the all-reduced operator
                assert (nd == 1 and 128 < rows_glob[1] <= 150000) if nd < nl else rows_glob[-1] <= 128
            if mesh_args.get("long_beam"):
                assert nd < nl              # (this case keeps the replication of a 3-dof level covered)
            lam = d0["amg_lam"]
            assert all(np.array_equal(d["amg_lam"], lam) for d in ds)
            lam_true = [0.0] * nl
            _, its_oracle, reason_oracle, *_ = O.pcg_amg(prob.rowptr, prob.cols, prob.vals, prob.rhs, aggs, rtol=1e-10, cheb_degree=int(deg),
                                                         eig_ratio=float(ratio), coarse_scale=float(scale), fine_degree=int(fdeg),
                                                         lam_given=lam, lam_true_out=lam_true, single_reduction=single)
            # the ranks' bound (sum of the shares' absolute values) is one: never below the assembled matrix's row sums, seldom far above
            assert all(t * (1 - 1e-12) <= g <= 1.6 * t for t, g in zip(lam_true, lam)), (lam_true, lam.tolist())
            assert all(abs(g - t) <= 1e-12 * t for t, g in zip(lam_true[nd:], lam[nd:]))        # assembled levels: the bound itself
            # ... and the count stays near the one-rank hierarchy's, far below block Jacobi over the ranks
            assert its_oracle < its_jacobi
            # what the library says one cycle costs in communication is what the hooks saw (two ranks: both take part in every
            # exchange; two solves + the set-up's exchanges, a few per level)
            ex, ar = int(d0["amg_exchanges"]), int(d0["amg_allreduces"])
            assert ex >= nd and ar == (1 if rows_glob[-1] <= 128 or nd < nl else 0)
            if world == 2 and not peer:
                n_x = sum(1 for k in d0["log"] if k[0] == "x")
                assert 2 * int(d0["its"]) * (1 + ex) <= n_x <= 2 * (int(d0["its"]) + 2) * (1 + ex) + 40 * nl
        else:
            _, its_oracle, reason_oracle, *_ = O.pcg_bjacobi_amg(prob.rowptr, prob.cols, prob.vals, prob.rhs, blocks, rtol=1e-10, cheb_degree=int(deg),
                                                                 eig_ratio=float(ratio), coarse_scale=float(scale), fine_degree=int(fdeg))
        print(f"gamg {kind_name} x{world} {partition} {mode}: {'coupled' if coupled else 'per-rank'} hierarchy, {int(d0['amg_levels'])} levels "
              f"({int(d0['amg_distributed'])} distributed), "
              f"{int(d0['its'])} iterations (oracle {its_oracle}, point Jacobi {its_jacobi})")
        assert reason_oracle == 2 and (its_oracle < its_jacobi or kind_name == "elast")     # (tiny beam blocks: no gain to expect)
        its_tol = max(2, its_oracle // 25)          # (runs of a hundred and more iterations on the little beam, whose CG stalls on plateaus: +-4 %)
        if single:                                   # (p,Ap) by recurrence: the plateaus of the little beam end an iteration or three apart
            its_tol = max(4, its_oracle // 12)
        if kind_name == "elast" and mesh_args.get("pc") == "gamg":
            # the little beam's count moves with the ORDER of the restriction's sums alone: 49..56 around the oracle's 54 / 55 between
            # the one-thread and the 16-lane form of k_rbm_restrict (PFEM_RBM_RESTRICT_WIDE=0 / 1, same aggregates, same operators)
            its_tol = max(its_tol, its_oracle // 10)
    if mode == "pbjacobi":
        want = "pbjacobi" if kind_name == "elast" else "jacobi"      # Poisson has no multi-row groups: all ranks fall back
        assert all(str(np.load(tmp_path / f"rank{r}.npz")["pc"]) == want for r in range(world))
        if kind_name == "elast":
            d0 = np.load(tmp_path / "rank0.npz")
            assert int(d0["its"]) < its_oracle                       # fewer iterations than point Jacobi ...
            its_tol = 10 ** 9                                        # ... so the count is not compared below
    got = np.full_like(u, np.nan)
    got2 = np.full_like(u, np.nan)
    for r in range(world):
        d = np.load(tmp_path / f"rank{r}.npz")
        assert (int(d["rs"]), int(d["re"])) == (int(prob.dm.row_start[r]), int(prob.dm.row_end[r]))
        got[int(d["rs"]):int(d["re"])] = d["x"]
        assert int(d["reason"]) == 2 and abs(int(d["its"]) - its_oracle) <= its_tol
        # per iteration: one exchange and two all-reduces; every rank issued the same KIND of call in the same order
        idle = int(d["n_peers"]) == 0                        # a rank without neighbours has nothing to exchange
        assert str(d["transport"]) == ("peer-ipc" if peer else "host")
        if peer:                                              # the hooks saw the bring-up and the oversized all-reduces only
            assert int(d["calls"]) < 3 * int(d["its"]) or int(d["its"]) < 8
        else:
            assert int(d["calls"]) >= (2 if idle else 3) * int(d["its"]) if not single else True
        if single and not peer and mesh_args.get("pc") == "gamg":
            # the multigrid loop in its single-reduction form: the CG's ONE all-reduce + the cycle's own (the replicated level's
            # right-hand side / the global dense bottom) per step; the two-reduction loop makes three
            n_all = sum(1 for s in d["log"] if s[0] == "a")
            steps = int(d["its"]) + 1
            assert 2 * steps <= n_all <= 2 * (steps + 4) + 150       # + the tail of the last chunk of 4 + the collectives of the symbolic and numeric set-up
        elif single and not peer:                            # ONE all-reduce per step; steps = its + 1 (the last one judges)
            n_all = sum(1 for s in d["log"] if s[0] == "a")
            setup_allreduces = 0                              # point Jacobi: the set-up exchanges need no all-reduce
            assert n_all - setup_allreduces <= int(d["its"]) + 1 + 32     # + the tail of the last 32-step chunk
            assert n_all >= int(d["its"]) + 1
        kinds = [s[0] for s in d["log"]]
        kinds0 = [s[0] for s in np.load(tmp_path / "rank0.npz")["log"]]
        if idle:
            kinds0 = [k for k in kinds0 if k == "a"]
        assert kinds == kinds0 or peer
        if partition == "idle" and r == world - 1:      # an idle rank owns nothing and shares nothing, but takes part in
            assert int(d["n_peers"]) == 0 and int(d["re"]) == int(d["rs"])       # every all-reduce and agrees on the verdict
        else:
            assert int(d["n_peers"]) >= 1
            if mode in ("overlap", "pbjacobi") or mesh_args.get("pc"):
                assert 0 < int(d["slices_b"]) <= int(d["slices"])
        if "x2" in d.files:
            got2[int(d["rs"]):int(d["re"])] = d["x2"]
            assert int(d["reason2"]) == 2
    assert np.abs(got - u).max() <= 1e-8 * max(1.0, np.abs(u).max())
    if mesh_args.get("resolve"):
        u2 = lu.solve(prob.rhs + 0.25)
        assert np.abs(got2 - u2).max() <= 1e-8 * max(1.0, np.abs(u2).max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind_name,world,partition,mode", [("poisson", 2, "slabs", "batched"), ("elast", 3, "sectors", "batched"),
                                                            ("poisson", 2, "slabs", "compat"), ("elast", 2, "slabs", "pbjacobi"),
                                                            ("poisson", 3, "idle", "batched"), ("elast", 3, "sectors", "overlap"),
                                                            ("poisson", 3, "rcb", "single_overlap"), ("elast", 3, "yslabs", "devgen"),
                                                            ("poisson", 2, "slabs", "gamg"), ("elast", 3, "yslabs", "gamg"),
                                                            ("poisson", 3, "idle", "gamg_overlap"), ("poisson", 3, "rcb", "gamg_distributed"),
                                                            ("elast", 3, "sectors", "gamg"), ("poisson", 5, "rcb", "gamg"),
                                                            ("elast", 2, "slabs", "reorder_gamg")])
def test_gpu_peer_memory_transport(tmp_path, kind_name, world, partition, mode):
    """The same multi-rank cases with the DEVICE-SIDE transport between the ranks that share cuda:0: every rank maps the
    others' receive boxes (hipIpcGetMemHandle / hipIpcOpenMemHandle), exchange and small all-reduces are kernels that write
    into the neighbour's box and flag it (pfem_solver_set_comm_peer) -- no host in the data path, which RCCL cannot offer
    with two ranks on one device.  Against the oracle's direct solve and iteration count like the host-staged runs; the
    host hooks see the bring-up only."""
    test_gpu_ranks_on_one_device_match_oracle(tmp_path, kind_name, world, partition, mode, peer=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind_name,world,partition,mode", [("poisson", 3, "rcb", "gamg_distributed"), ("elast", 3, "yslabs", "gamg"),
                                                            ("poisson", 2, "slabs", "gamg_overlap")])
def test_gpu_coupled_cycle_fused_equals_separate_kernels(tmp_path, monkeypatch, kind_name, world, partition, mode):
    """The cycle of the hierarchy across the ranks as it is run -- the shared rows packed by the coarse SpMV / the restriction
    itself, the holders' shares summed inside the vector step that uses the product -- against the same cycle with a pack and
    an unpack-sum kernel around every exchange (PFEM_AMG_COUPLED_FUSED=0): same arithmetic in the same order, so iteration
    counts and solutions agree bit for bit on every rank."""
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("PFEM_AMG_COUPLED_FUSED", fused)
        d = tmp_path / f"fused{fused}"
        d.mkdir()
        test_gpu_ranks_on_one_device_match_oracle(d, kind_name, world, partition, mode)
        out[fused] = [np.load(d / f"rank{r}.npz") for r in range(world)]
    for a, b in zip(out["1"], out["0"]):
        assert int(a["its"]) == int(b["its"]) and np.array_equal(a["x"], b["x"])
        # ... and the fused form made fewer hook-visible calls?  no: the exchanges are the same, only the kernels around them differ
        assert int(a["calls"]) == int(b["calls"])


def _rccl_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)       # only carries the unique id
    try:
        import pfemfort_amd as pf
        from pfemfort_amd import distributed as PD
        from pfemfort_amd import host as H
        mesh = H.gen_box_tets(-1, 1, 12, -1, 1, 10, -1, 1, 14)
        dm = H.dof_numbering(mesh.nNode, 1, mesh.bc_node, mesh.bc_dof, mesh.bc_val)
        conn, xyz = H.renumber_mesh(mesh, dm)
        edof = H.elem_dof_array(conn, dm.NodeDofArrayNew)
        s = pf.PetscSolver().initialise(dm.size_global, dm.size_global, device=0)
        s.setTolerances(rtol=1e-10)
        s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
        PD.attach(s, dist)                                             # RCCL inside the library, world size 1
        bad = s.commSelftest(4096)                                     # ncclSend/ncclRecv to self in one group + ncclAllReduce
        s.buildPattern()
        s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
        os.environ["PFEM_FORCE_MULTI"] = "1"                          # one rank, but through the multi-rank loop
        its, reason, _ = s.factoriseAndSolve()
        x = s.getSolution()
        # the same through -pc_type gamg's multi-rank form: the hierarchy ACROSS the ranks (here one), whose set-up and cycle
        # all-reduce vectors of other lengths (level sizes, eigenvalue bounds, the dense bottom operator and its right-hand side)
        s.setPreconditioner("gamg")
        its_g, reason_g, _ = s.factoriseAndSolve()
        np.savez(os.path.join(out_dir, "rccl.npz"), its=its, reason=reason, x=x, bad=bad, its_g=its_g, reason_g=reason_g, x_g=s.getSolution(),
                 coupled=int(s.amgLayout()["coupled"]), levels=s.amgInfo()["levels"])
        s.free()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_rccl_backend_world_size_1(tmp_path):
    """Only one GPU per box here, and RCCL refuses two ranks on one device: this pins what CAN be pinned of the
    backend bench.py uses for N>1 -- librccl found and bound at run time, communicator from a broadcast unique id,
    grouped ncclSend/ncclRecv (to self) and ncclAllReduce on the communication stream with the event hand-over to
    the compute stream, and a solve that takes the multi-rank loop (all scalars through ncclAllReduce)."""
    import torch.multiprocessing as mp
    import pfemfort_amd as pf
    from pfemfort_amd import host as H
    mp.spawn(_rccl_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    d = np.load(tmp_path / "rccl.npz")
    ref = pf.tetrapoissonparallelimpl1(H.gen_box_tets(-1, 1, 12, -1, 1, 10, -1, 1, 14), rtol=1e-10)
    assert int(d["bad"]) == 0
    assert int(d["reason"]) == 2 and abs(int(d["its"]) - ref.its) <= 1
    assert np.abs(d["x"] - ref.soln_free).max() <= 1e-9
    ref_g = pf.tetrapoissonparallelimpl1(H.gen_box_tets(-1, 1, 12, -1, 1, 10, -1, 1, 14), rtol=1e-10, pc="gamg")      # the one-rank loop
    assert int(d["coupled"]) == 1 and int(d["levels"]) >= 2 and int(d["reason_g"]) == 2 and abs(int(d["its_g"]) - ref_g.its) <= 1
    assert np.abs(d["x_g"] - ref_g.soln_free).max() <= 1e-9


def test_neighbour_plan_against_brute_force_random_layouts():
    """pfem_neighbour_plan on random layouts (row blocks of random sizes, including empty ones, random ghost sets) against
    the definition: shared(r, q) = local(r) & local(q), peers = the ranks with a non-empty intersection."""
    from hypothesis import given, settings, strategies as st
    from pfemfort_amd import host as H

    @settings(max_examples=150, deadline=None)
    @given(st.integers(1, 6), st.integers(0, 60), st.integers(0, 2 ** 31 - 1))
    def check(world, n, seed):
        rng = np.random.default_rng(seed)
        cuts = np.sort(rng.integers(0, n + 1, world - 1))
        bounds = np.concatenate([[0], cuts, [n]])
        ranges = [(int(bounds[r]), int(bounds[r + 1])) for r in range(world)]
        ghosts = []
        for r in range(world):
            outside = np.array([g for g in range(n) if not ranges[r][0] <= g < ranges[r][1]], np.int64)
            k = int(rng.integers(0, len(outside) + 1)) if len(outside) else 0
            ghosts.append(np.sort(rng.choice(outside, k, replace=False)) if k else np.empty(0, np.int64))
        local = [set(range(*ranges[r])) | set(ghosts[r].tolist()) for r in range(world)]
        for r in range(world):
            peers, off, gid = H.neighbour_plan(r, ranges, ghosts)
            want = [q for q in range(world) if q != r and local[r] & local[q]]
            assert peers.tolist() == want
            for k, q in enumerate(peers):
                assert gid[off[k]:off[k + 1]].tolist() == sorted(local[r] & local[q])

    check()
