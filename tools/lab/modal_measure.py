"""What the modal analysis costs (pfem_modal_solve), on one MI355X; events, one warm-up box, five boxes, median and range (the
method of dynamics_measure.py):

  * microseconds of one block product k_spmm<MB> against MB launches of the SpMV form in effect, MB = 4, 8, 16, same handle, same
    session (benchModalSpmm), on BASELINE config 3 (the 200^3 Poisson box) and config 4 (the 50 x 300 x 50 beam), beside one
    single product (benchSpmv) and the bytes of the row form;
  * wall time per LOBPCG iteration for n_modes = 6 (MB = 8) under the point Jacobi, over a fixed number of iterations, the
    residual reached, and the bytes of the passes over the six blocks; iterations to tol 1e-6 where the cap allows it; the same
    with the cycle of a gamg solve as T.

`python tools/lab/modal_measure.py [out.json] [--small]` (--small: meshes of a few thousand dofs, to try the script)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

BOXES, REPS, CAP = 5, 20, 200
small = "--small" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "boxes": v}


out = {}
cases = (("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA),
         ("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA))
if small:
    cases = (("small_poisson_20", pf.POISSON_TET, (-1, 1, 20, -1, 1, 20, -1, 1, 20), 0, 1, H.POISSON_ELEMDATA),
             ("small_beam_5x30x5", pf.ELAST_TET, (-0.5, 0.5, 5, 0.0, 6.0, 30, -0.5, 0.5, 5), 1, 3, H.ELAST_ELEMDATA))
for name, kind, box, bc, ndof, ed in cases:
    sz = H.box_slab_sizes(box[2], box[5], box[8], bc, ndof)
    s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    s.generateBoxMesh(kind, *box, bc_mode=bc)
    s.buildPattern()
    s.assemble(ed, H.TIMEDATA)
    s.dynamicsSetup(ed, 7.8)
    info = s.matrixInfo()
    n = info["n_owned"]
    res = {"dof": n, "nnz": info["nnz"], "stored": info["stored"], "row_form_bytes": 12 * info["stored"], "spmv_form_bytes": s.spmvFormatBytes()}
    s.benchSpmv(REPS)
    res["spmv_us"] = summary([1e3 * s.benchSpmv(10 * REPS) for _ in range(BOXES)])
    for mb in (4, 8, 16):
        s.benchModalSpmm(mb, REPS)                               # warm-up box
        boxes = [s.benchModalSpmm(mb, REPS) for _ in range(BOXES)]
        a, b = summary([x[0] for x in boxes]), summary([x[1] for x in boxes])
        res[f"mb{mb}"] = {"spmm_us": a, "mb_spmv_us": b, "spmm_over_mb_spmv": a["median"] / b["median"],
                          "spmm_over_one_spmv": a["median"] / res["spmv_us"]["median"],
                          "block_bytes": 8 * n * mb, "spmm_min_bytes": 12 * info["stored"] + 2 * 8 * n * mb}
    s.setPreconditioner("jacobi")
    s.modalSolve(6, tol=1e-6, max_iterations=10, modes=False)     # buffers, warm-up
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = s.modalSolve(6, tol=1e-6, max_iterations=CAP, modes=False)
        walls.append(time.perf_counter() - t0)
    res["lobpcg_n_modes6_jacobi"] = {"iterations": r.iterations, "reason": r.reason, "restarts": r.restarts, "largest_residual": float(r.residuals.max()),
                                     "pc": r.pc, "omega": r.omega.tolist(), "wall_s": summary(walls),
                                     "ms_per_iteration": 1e3 * statistics.median(walls) / max(r.iterations, 1),
                                     # gram reads 6 blocks; update reads 6 and writes 4; residual reads 2 and writes 1; the product reads 1, writes 1
                                     "block_pass_bytes_per_iteration": (6 + 10 + 3 + 2) * 8 * n * 8}
    # ... and with the multigrid cycle of a gamg solve as T (eight cycles an iteration, one a column)
    s.setPreconditioner("gamg")
    its_solve = s.factoriseAndSolve()[0]
    s.modalSolve(6, tol=1e-6, max_iterations=2, modes=False)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        g = s.modalSolve(6, tol=1e-6, max_iterations=CAP, modes=False)
        walls.append(time.perf_counter() - t0)
    res["lobpcg_n_modes6_gamg"] = {"pc": g.pc, "iterations": g.iterations, "reason": g.reason, "restarts": g.restarts,
                                   "largest_residual": float(g.residuals.max()), "omega": g.omega.tolist(), "wall_s": summary(walls),
                                   "ms_per_iteration": 1e3 * statistics.median(walls) / max(g.iterations, 1), "gamg_solve_iterations": its_solve}
    out[name] = res
    print(name, json.dumps(res), flush=True)
    s.free()
if args:
    json.dump(out, open(args[0], "w"), indent=1)
