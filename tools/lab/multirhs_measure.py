"""What several right-hand sides in one solve cost (pfem_solver_solve_multi) against as many single solves, on one MI355X:
device events around work that ends in a synchronise, one warm-up box, five boxes, median and range; the two sides alternate in
every box (the method of modal_measure.py).

For nrhs = 1, 4, 8, 16, 32 under the point Jacobi, a fixed number of iterations (rtol far below reach, maxits = ITS, so that both
sides do the same work whatever rounding does to the stopping iteration): the device time of one multi solve of the assembled
right-hand side scaled by j + 1 (benchSolveMany: per panel from after its upload to the last copy of its control block) against
nrhs x the solve_ms of one pfem_solver_solve on the same handle in the same box.  Per case also: one block product k_spmm<8>
(the product of the multi solve without its epilogue) and one single product, for the product's share, and the bytes a
panel-iteration moves at best, from the shapes.

Cases: BASELINE config 3 (the 200^3 Poisson box), config 4 (the 50 x 300 x 50 beam), a Poisson box whose free nodes are moved
by 0.2 of the smallest cell edge (no value dictionary: the single product streams fp64 values; 100^3, the host generator's
reach in reasonable time) and a 20^3 box (launch-bound).

`python tools/lab/multirhs_measure.py [out.json] [--small] [--md]` (--small: meshes of a few thousand dofs, to try the script;
--md: the table of DESIGN.md section 16 on stdout at the end)."""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

BOXES, ITS, NRHS = 5, 30, (1, 4, 8, 16, 32)
small = "--small" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "boxes": v}


def jittered(box, jitter):
    """bench.py's --jitter: the nodes without a Dirichlet value moved inside a ball of radius jitter x (smallest cell edge) / sqrt 3"""
    m = H.gen_box_tets(*box)
    hmin = min((box[1] - box[0]) / box[2], (box[4] - box[3]) / box[5], (box[7] - box[6]) / box[8])
    d = np.random.default_rng(7).uniform(-1.0, 1.0, size=m.xyz.shape) * (jitter * hmin / np.sqrt(3.0))
    d[:, np.unique(m.bc_node)] = 0.0
    return H.Mesh(m.xyz + d, m.conn, m.bc_node, m.bc_dof, m.bc_val, box=m.box)


def handle(kind, box, bc, ndof, ed, jitter):
    if jitter == 0.0:
        sz = H.box_slab_sizes(box[2], box[5], box[8], bc, ndof)
        s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
        s.generateBoxMesh(kind, *box, bc_mode=bc)
    else:
        mesh = jittered(box, jitter)
        dm = H.dof_numbering(mesh.nNode, ndof, mesh.bc_node, mesh.bc_dof, mesh.bc_val)
        conn, xyz = H.renumber_mesh(mesh, dm)
        s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
        s.uploadMesh(kind, conn, xyz, H.elem_dof_array(conn, dm.NodeDofArrayNew), dm.solnApplied)
    s.buildPattern()
    s.assemble(ed, H.TIMEDATA)
    return s


cases = (("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA, 0.0),
         ("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA, 0.0),
         ("poisson_100_jitter0.2", pf.POISSON_TET, (-1, 1, 100, -1, 1, 100, -1, 1, 100), 0, 1, H.POISSON_ELEMDATA, 0.2),
         ("poisson_20", pf.POISSON_TET, (-1, 1, 20, -1, 1, 20, -1, 1, 20), 0, 1, H.POISSON_ELEMDATA, 0.0))
if small:
    cases = (("small_poisson_20", pf.POISSON_TET, (-1, 1, 20, -1, 1, 20, -1, 1, 20), 0, 1, H.POISSON_ELEMDATA, 0.0),
             ("small_beam_5x30x5", pf.ELAST_TET, (-0.5, 0.5, 5, 0.0, 6.0, 30, -0.5, 0.5, 5), 1, 3, H.ELAST_ELEMDATA, 0.0),
             ("small_poisson_12_jitter0.2", pf.POISSON_TET, (-1, 1, 12, -1, 1, 12, -1, 1, 12), 0, 1, H.POISSON_ELEMDATA, 0.2))
out = {}
for name, kind, box, bc, ndof, ed, jitter in cases:
    s = handle(kind, box, bc, ndof, ed, jitter)
    info = s.matrixInfo()
    n = info["n_owned"]
    s.setPreconditioner("jacobi")
    s.setTolerances(rtol=1e-300, maxits=ITS)
    res = {"dof": n, "nnz": info["nnz"], "stored": info["stored"], "iterations": ITS, "row_form_bytes": 12 * info["stored"],
           "spmv_form_bytes": s.spmvFormatBytes()}
    single, multi = {k: [] for k in NRHS}, {k: [] for k in NRHS}
    for box_no in range(BOXES + 1):                      # (box 0: the warm-up, dropped)
        for k in NRHS:
            its, why, _ = s.factoriseAndSolve()
            assert its == ITS and why == -3, (its, why)
            t_single = s.timings()["solve_ms"]
            ms, its_m = s.benchSolveMany(k, 1)
            assert (its_m == ITS).all(), its_m
            if box_no:
                single[k].append(t_single)
                multi[k].append(float(ms[0]))
    res["value_dictionary"] = s.spmvValueDictionary()    # (after the solves: the first one builds it)
    s.benchSpmv(20)
    res["spmv_us"] = summary([1e3 * s.benchSpmv(100) for _ in range(BOXES)])
    s.benchModalSpmm(8, 20)
    res["spmm8_us"] = summary([s.benchModalSpmm(8, 20)[0] for _ in range(BOXES)])
    for k in NRHS:
        a, b = summary(single[k]), summary(multi[k])
        panels = [8] * (k // 8) + ([4] if 0 < k % 8 <= 4 else [8] if k % 8 else [])
        us_multi = 1e3 * b["median"] / (ITS * k)
        res[f"nrhs{k}"] = {"single_solve_ms": a, "multi_ms": b, "multi_over_nrhs_single": b["median"] / (k * a["median"]),
                           "us_per_column_iteration_single": 1e3 * a["median"] / ITS, "us_per_column_iteration_multi": us_multi, "panels": panels}
    res["product_share_of_a_panel_of_8"] = res["spmm8_us"]["median"] / (8 * res["nrhs8"]["us_per_column_iteration_multi"])
    # a panel-iteration at best: the row form once; the product reads P and writes W; the update reads W and R and writes R; the
    # direction reads X, P and R and writes X and P; the inverse diagonal twice
    res["panel8_iteration_min_bytes"] = 12 * info["stored"] + (2 + 3 + 5) * 8 * n * 8 + 2 * 8 * n
    out[name] = res
    print(name, json.dumps(res), flush=True)
    s.free()
if args:
    json.dump(out, open(args[0], "w"), indent=1)
if "--md" in sys.argv:
    print("| case | dofs | nrhs | nrhs single solves [ms] (min..max of one) | one multi solve [ms] (min..max) | multi / (nrhs x single) | us per column-iteration: single | multi |")
    print("|---|---|---|---|---|---|---|---|")
    for name, r in out.items():
        for k in NRHS:
            q = r[f"nrhs{k}"]
            a, b = q["single_solve_ms"], q["multi_ms"]
            print(f"| {name} | {r['dof']} | {k} | {k * a['median']:.2f} ({a['min']:.3f}..{a['max']:.3f}) | {b['median']:.2f} ({b['min']:.2f}..{b['max']:.2f}) | "
                  f"{q['multi_over_nrhs_single']:.2f} | {q['us_per_column_iteration_single']:.1f} | {q['us_per_column_iteration_multi']:.1f} |")
